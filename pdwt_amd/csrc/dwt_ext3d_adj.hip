// dwt_ext3d_adj.hip -- the adjoint operators of one level of the 3-D transform with signal-extension boundary modes (include/pdwt_hip.h
// "Adjoints of the 3-D boundary-mode DWT"): what a gradient method needs of pdwt_ext3d_forward_level_* / pdwt_ext3d_inverse_level_*.
//   adjoint of the forward (a mode): the forward runs x-y, then z, so the adjoint runs z, then x-y
//     k_ext3_adj_z         the eight cotangent bands -> the four quadrant cotangents (nz, hr, hc) in scratch: the geometry of k_ext3_syn_z
//                          (lanes across the expanded plane, blockIdx.y = a chunk of 16 samples along z, blockIdx.z = the quadrant) with
//                          the reversed analysis taps, and the fold of the extension along z in the same launch (dwt_ext3d_adj.hpp)
//     adj2_forward_level   the 2-D level adjoint of dwt_ext_adj.hip on B = nz planes: the quadrants are its A, H, V, D stacks
//   adjoint of the inverse (no mode): the forward level in mode zero with the bank L' = reversed IL, H' = reversed IH; no kernel.
// Traffic of the z pass per level: the eight band stacks read once, the four quadrant stacks written once; a border chunk re-reads at
// most (2F - 3) F band elements per column.
#include "dwt_ext3d_adj.hpp"
#include "dwt_ext3d_xy.hpp"

namespace pdwt {

template <typename T, int HL>
__global__ __launch_bounds__(kA3ZThreads) void k_ext3_adj_z(Adj3ZJob<T> job, Taps2<T> taps, Adj3ZHalo<T> hm)
{
    const int k = blockIdx.x * kA3ZThreads + threadIdx.x;
    if (k >= job.plane) return;
    ext3_adj_z_lane<T, HL>(job, taps, hm, blockIdx.z, blockIdx.y * A3ZC, k);
}

template <typename T, int HL>
static int launch_ext3_adj_z(const Adj3ZJob<T>& zj, const Taps2<T>& taps, const Adj3ZHalo<T>& hm)
{
    const dim3 grid(idiv_up(zj.plane, kA3ZThreads), idiv_up(zj.nz, A3ZC), 4);
    hipLaunchKernelGGL((k_ext3_adj_z<T, HL>), grid, dim3(kA3ZThreads), 0, stream(), zj, taps, hm);
    PDWT_HIP_TRY(hipGetLastError());
    return PDWT_OK;
}

static bool adj3_level_ok(int nz, int nr, int nc, int hlen) { return ext3_level_ok(nz, nr, nc, hlen) && adj2_level_ok(nz, nr, nc, hlen); }

// scratch of a level: [the four quadrant cotangents, padded | the frames of the nz planes of the x-y adjoint]
static size_t adj3_quad_elems(int nz, int nr, int nc, int hlen) { return pad64(4 * (size_t)nz * ext_half(nr, hlen) * ext_half(nc, hlen)); }

template <typename T>
static int adj3_forward_level(T* dst, T* const* b, int nz, int nr, int nc, int mode, const typename FiltersOf<T>::type* f, T* tmp)
{
    if (!dst || !b || !f || !tmp || mode < 0 || mode >= EXT_NUM_MODES || !adj3_level_ok(nz, nr, nc, f->hlen)) return PDWT_EINVAL;
    for (int k = 0; k < 8; k++)
        if (!b[k]) return PDWT_EINVAL;
    const int hlen = f->hlen, hz = ext_half(nz, hlen), hr = ext_half(nr, hlen), hc = ext_half(nc, hlen);
    const size_t sq = (size_t)nz * hr * hc;
    Adj3ZJob<T> zj{};
    for (int q = 0; q < 4; q++) {
        zj.lo[q] = b[ext3_band(q, 0)];
        zj.hi[q] = b[ext3_band(q, 1)];
        zj.q[q] = tmp + q * sq;
    }
    zj.nz = nz, zj.hz = hz, zj.plane = hr * hc;
    const Taps2<T> taps = taps_adj<T>(f);
    const Adj3ZHalo<T> hm = adj3_z_halo<T>(nz, hlen, mode, taps);
    if (const int rc = with_filter_length(hlen, [&](auto hl) { return launch_ext3_adj_z<T, decltype(hl)::value>(zj, taps, hm); }); rc != PDWT_OK) return rc;
    // the quadrants q = 2 * x band + y band are A, H, V, D of the 2-D adjoint in that order
    return adj2_forward_level<T>(dst, zj.q[0], zj.q[1], zj.q[2], zj.q[3], nz, nr, nc, mode, f, tmp + adj3_quad_elems(nz, nr, nc, hlen));
}

}  // namespace pdwt

using namespace pdwt;

extern "C" {
long long pdwt_ext3d_adjoint_level_tmp_elems(int nz, int nr, int nc, int hlen)
{
    if (!adj3_level_ok(nz, nr, nc, hlen)) return PDWT_EINVAL;
    return (long long)adj3_quad_elems(nz, nr, nc, hlen) + (long long)nz * (long long)adj_frame_elems(nr, nc, hlen);
}
int pdwt_ext3d_adjoint_z_run(int nz, int hlen, int mode, int* z0, int* z1)
{
    if (hlen < 2 || hlen > PDWT_MAX_FILTER_WIDTH || (hlen & 1) || nz < 1 || nz < hlen - 1 || nz > 65535 || mode < 0 || mode >= EXT_NUM_MODES) return PDWT_EINVAL;
    const Adj3ZHalo<float> hm = adj3_z_halo<float>(nz, hlen, mode, Taps2<float>{});
    if (z0) *z0 = hm.z0;
    if (z1) *z1 = hm.z1;
    return PDWT_OK;
}
int pdwt_ext3d_forward_adjoint_level_f32(float* d_dst, float* const* d_bands, int nz, int nr, int nc, int mode, const pdwt_filters_f32* f, float* d_tmp)
{
    return adj3_forward_level<float>(d_dst, d_bands, nz, nr, nc, mode, f, d_tmp);
}
int pdwt_ext3d_forward_adjoint_level_f64(double* d_dst, double* const* d_bands, int nz, int nr, int nc, int mode, const pdwt_filters_f64* f, double* d_tmp)
{
    return adj3_forward_level<double>(d_dst, d_bands, nz, nr, nc, mode, f, d_tmp);
}
int pdwt_ext3d_inverse_adjoint_level_f32(const float* d_src, float* const* d_bands, int nz, int nr, int nc, const pdwt_filters_f32* f, float* d_tmp)
{
    pdwt_filters_f32 g;
    if (!adj_inverse_bank<float>(g, f) || !adj3_level_ok(nz, nr, nc, f->hlen)) return PDWT_EINVAL;
    return pdwt_ext3d_forward_level_f32(d_src, d_bands, nz, nr, nc, EXT_ZERO, &g, d_tmp);
}
int pdwt_ext3d_inverse_adjoint_level_f64(const double* d_src, double* const* d_bands, int nz, int nr, int nc, const pdwt_filters_f64* f, double* d_tmp)
{
    pdwt_filters_f64 g;
    if (!adj_inverse_bank<double>(g, f) || !adj3_level_ok(nz, nr, nc, f->hlen)) return PDWT_EINVAL;
    return pdwt_ext3d_forward_level_f64(d_src, d_bands, nz, nr, nc, EXT_ZERO, &g, d_tmp);
}
}
