// dwt_ext3d_level.hpp -- one level of the 3-D boundary-mode transform, of its inverse and of the adjoint of the forward on a contiguous
// stack of V volumes, written once: the level entries (dwt_ext3d.hip, dwt_ext3d_adj.hip) run a step with V = 1 and the one-volume z
// jobs, the stack drivers (dwt_ext3db.hip) once per level with the stack jobs (STACK picks the jobs, and with them the kernels that a
// translation unit instantiates).  The argument checks and the layout of the scratch stay with each entry; a step is given the four
// quadrant stacks (sq = V * nz * hr * hc elements apart) and, for the adjoint, the frames of the planes.
//   x-y passes   a V x nz x nr x nc stack is V * nz planes: k_ext3_fwd_xy / k_ext3_inv_xy (run_ext3_xy) and the 2-D level adjoint
//                (adj2_forward_level) take the plane on grid z, so they run on chunks of at most 65535 planes; a chunk may begin inside
//                a volume.  The source, the quadrants and the frames of the adjoint are offset by whole planes.
//   z passes     the kernels of z_stages.hpp over the 4 V (volume, quadrant) pairs, in chunks of at most 65535 pairs.
// One volume is one chunk of either kind (nz <= 65535).
#pragma once
#include <type_traits>

#include "dwt_ext3d_xy.hpp"
#include "z_stages.hpp"

namespace pdwt {

template <typename T>
struct Ext3Step {
    size_t V;
    int nz, nr, nc, hlen;
    T* quads;  // scratch: the four quadrant stacks
    int hz() const { return ext_half(nz, hlen); }
    int hr() const { return ext_half(nr, hlen); }
    int hc() const { return ext_half(nc, hlen); }
    size_t sq() const { return V * nz * hr() * hc(); }
    size_t planes() const { return V * nz; }
};

// the x-y pass over the planes of the stack: vol is the stack of nr x nc planes (the source of the forward, the result of the inverse)
template <typename T>
static int ext3_step_xy(const Ext3Step<T>& s, bool fwd, const T* src, T* dst, int mode, const Taps2<T>& taps)
{
    const int hr = s.hr(), hc = s.hc();
    return z_chunks(s.planes(), [&](size_t p0, int cnt) {
        Ext3XYJob<T> xy{};
        xy.src = src ? src + p0 * s.nr * s.nc : nullptr;
        xy.dst = dst ? dst + p0 * s.nr * s.nc : nullptr;
        for (int q = 0; q < 4; q++) xy.q[q] = s.quads + q * s.sq() + p0 * hr * hc;
        xy.nr = s.nr, xy.nc = s.nc, xy.hr = hr, xy.hc = hc, xy.mode = mode;
        return run_ext3_xy<T>(s.hlen, fwd, xy, cnt, taps);
    });
}

// lev: the eight band stacks of the level (aaa, aad, ... ddd).  x-y into the quadrants (reads the input), then z into the bands (band aaa
// may be the input's own buffer: already read)
template <bool STACK, typename T>
static int ext3_forward_step(const Ext3Step<T>& s, const T* src, T* const* lev, int mode, const Taps2<T>& taps)
{
    if (const int rc = ext3_step_xy<T>(s, true, src, nullptr, mode, taps); rc != PDWT_OK) return rc;
    std::conditional_t<STACK, ZStackJob<T>, ZJob<T>> zj{};
    for (int q = 0; q < 4; q++) {
        zj.src[q] = s.quads + q * s.sq();
        zj.lo[q] = lev[ext3_band(q, 0)];
        zj.hi[q] = lev[ext3_band(q, 1)];
    }
    zj.nin = s.nz, zj.nout = s.hz(), zj.plane = s.hr() * s.hc(), zj.mode = mode;
    return run_z<false, T>(s.hlen, true, zj, 4 * s.V, taps);
}

// z into the quadrants (reads the bands), then x-y into the output (may be the buffer of band aaa: already read)
template <bool STACK, typename T>
static int ext3_inverse_step(const Ext3Step<T>& s, T* dst, T* const* lev, const Taps2<T>& taps)
{
    std::conditional_t<STACK, ZStackJob<T>, ZJob<T>> zj{};
    for (int q = 0; q < 4; q++) {
        zj.src[q] = lev[ext3_band(q, 0)];
        zj.src2[q] = lev[ext3_band(q, 1)];
        zj.lo[q] = s.quads + q * s.sq();
    }
    zj.nin = s.hz(), zj.nout = s.nz, zj.plane = s.hr() * s.hc(), zj.mode = 0;
    if (const int rc = run_z<false, T>(s.hlen, false, zj, 4 * s.V, taps); rc != PDWT_OK) return rc;
    return ext3_step_xy<T>(s, false, nullptr, dst, 0, taps);
}

// the adjoint of the forward step: z (taps: taps_adj of f), then the 2-D level adjoint on the planes -- the quadrants q = 2 * x band + y
// band are its A, H, V, D in that order; a chunk of planes has its own frames
template <bool STACK, typename T>
static int ext3_adjoint_step(const Ext3Step<T>& s, T* dst, T* const* lev, int mode, const typename FiltersOf<T>::type* f, const Taps2<T>& taps, T* frames)
{
    std::conditional_t<STACK, Adj3ZStackJob<T>, Adj3ZJob<T>> zj{};
    for (int q = 0; q < 4; q++) {
        zj.lo[q] = lev[ext3_band(q, 0)];
        zj.hi[q] = lev[ext3_band(q, 1)];
        zj.q[q] = s.quads + q * s.sq();
    }
    zj.nz = s.nz, zj.hz = s.hz(), zj.plane = s.hr() * s.hc();
    if (const int rc = run_z_adjoint<T>(s.hlen, zj, 4 * s.V, taps, adj3_z_halo<T>(s.nz, s.hlen, mode, taps)); rc != PDWT_OK) return rc;
    const size_t sq = s.sq(), fe = adj_frame_elems(s.nr, s.nc, s.hlen), img = (size_t)s.nr * s.nc, qp = (size_t)s.hr() * s.hc();
    return z_chunks(s.planes(), [&](size_t p0, int cnt) {
        const T* q = s.quads + p0 * qp;
        return adj2_forward_level<T>(dst + p0 * img, q, q + sq, q + 2 * sq, q + 3 * sq, cnt, s.nr, s.nc, mode, f, frames + p0 * fe);
    });
}

}  // namespace pdwt
