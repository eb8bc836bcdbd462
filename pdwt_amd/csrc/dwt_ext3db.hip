// dwt_ext3db.hip -- the 3-D transform with signal-extension boundary modes and its adjoints on a STACK of V volumes, every level in one
// driver call (include/pdwt_hip.h "Batched 3-D DWT with boundary modes").  Volume v of every result holds the bits that the chain of
// level entries of dwt_ext3d.hip / dwt_ext3d_adj.hip gives on volume v alone: the same x-y kernels run, and z kernels that do the work
// of the one-volume ones per lane; only the grid differs.
//   x-y passes   a contiguous V x nz x nr x nc stack is V * nz planes: k_ext3_fwd_xy / k_ext3_inv_xy (run_ext3_xy) and the 2-D level
//                adjoint (adj2_forward_level) take the plane on grid z, so they run as they are on chunks of at most 65535 planes; a
//                chunk may begin inside a volume.  The source, the quadrants and the frames of the adjoint are offset by whole planes.
//   z passes     k_ext3b_ana_z / k_ext3b_syn_z / k_ext3b_adj_z: lanes across the expanded plane, grid y = a chunk of 16 outputs along
//                z, grid z = a (volume, quadrant) pair p = 4 * v + q, in chunks of at most 65535 pairs (a chunk may begin inside a
//                volume).  Per lane the work is that of k_ext3_ana_z / k_ext3_syn_z (dwt_ext3d.hip, restated here) and ext3_adj_z_lane
//                (dwt_ext3d_adj.hpp, called) on column pointers offset by the volume: quadrant stack q is V x nz x hr x hc, band stack k is
//                V x hz x hr x hc, volume v of either starts v * planes * plane elements in.
// Every output element is written once by one thread; no atomics.  Nothing synchronises with the host between levels or chunks.
// Scratch: [the four quadrant stacks of level 1 | two approximation stacks of level 1 in turn (levels > 1) | the frames of the planes
// (forward adjoint)]; the quadrants and approximations of a deeper level are no larger (n >= hlen - 1 gives (n + hlen - 1) / 2 <= n);
// of the frames the level that needs most is taken.
#include "dwt_ext3db.hpp"
#include "dwt_ext3d_xy.hpp"
#include "vol3d.hpp"

namespace pdwt {

constexpr int kX3bChunk = 65535;  // planes of an x-y launch, pairs of a z launch: a grid dimension
constexpr int kX3ZThreads = 256;  // (the z kernels of dwt_ext3d.hip: the same lanes, the same chunk along z)
constexpr int X3ZC = 16;

// ---- z passes: the bodies of k_ext3_ana_z / k_ext3_syn_z of dwt_ext3d.hip, restated on the columns of volume v ------------------------
// (Restated, not shared through a lane function: a bank handed to a function by reference is copied at the kernel's entry, which hoists
// all 2 * HL scalar tap loads in front of the loops -- for the 40-tap double bank 1600 lane reads of spilled SGPRs that the kernels
// of dwt_ext3d.hip do not have.  Read in place, as here and there, the taps are loaded where they are used.)
template <typename T, int HL>
__global__ __launch_bounds__(kX3ZThreads) void k_ext3b_ana_z(Ext3bZJob<T> job, Taps2<T> taps)
{
    const int k = blockIdx.x * kX3ZThreads + threadIdx.x;
    if (k >= job.plane) return;
    const X3bPair p = x3b_pair(job.pair0, blockIdx.z);
    const int e = p.e, i0 = blockIdx.y * X3ZC;
    constexpr int W = 2 * X3ZC + HL - 2;
    const int n = job.nin, s0 = 2 * i0 + 2 - HL;
    const size_t pl = (size_t)job.plane;
    const T* __restrict__ x = job.src[e] + x3b_offset(p.v, job.nin, pl) + k;
    T v[W];
    if (s0 >= 0 && s0 + W <= n) {
#pragma unroll
        for (int w = 0; w < W; w++) v[w] = x[(size_t)(s0 + w) * pl];
    } else {
#pragma unroll
        for (int w = 0; w < W; w++) {
            const int s = ext_index(s0 + w, n, job.mode);
            v[w] = s < 0 ? T(0) : x[(size_t)s * pl];
        }
    }
    T* __restrict__ lo = job.lo[e] + x3b_offset(p.v, job.nout, pl) + k;
    T* __restrict__ hi = job.hi[e] + x3b_offset(p.v, job.nout, pl) + k;
#pragma unroll
    for (int u = 0; u < X3ZC; u++) {
        if (i0 + u < job.nout) {
            T sl = T(0), sh = T(0);
#pragma unroll
            for (int j = 0; j < HL; j++) {
                sl = fma_t<T>(v[2 * u + j], taps.a[HL - 1 - j], sl);
                sh = fma_t<T>(v[2 * u + j], taps.b[HL - 1 - j], sh);
            }
            lo[(size_t)(i0 + u) * pl] = sl;
            hi[(size_t)(i0 + u) * pl] = sh;
        }
    }
}

template <typename T, int HL>
__global__ __launch_bounds__(kX3ZThreads) void k_ext3b_syn_z(Ext3bZJob<T> job, Taps2<T> taps)
{
    const int k = blockIdx.x * kX3ZThreads + threadIdx.x;
    if (k >= job.plane) return;
    const X3bPair p = x3b_pair(job.pair0, blockIdx.z);
    const int e = p.e, g0 = blockIdx.y * X3ZC;  // even
    constexpr int h2 = HL / 2, W = X3ZC / 2 + h2 - 1;
    const int nin = job.nin, q0 = g0 / 2;
    const size_t pl = (size_t)job.plane;
    const T* __restrict__ a = job.src[e] + x3b_offset(p.v, job.nin, pl) + k;
    const T* __restrict__ d = job.src2[e] + x3b_offset(p.v, job.nin, pl) + k;
    T va[W], vd[W];
#pragma unroll
    for (int w = 0; w < W; w++) {
        const bool in = q0 + w < nin;
        const size_t s = (size_t)(q0 + w) * pl;
        va[w] = in ? a[s] : T(0);
        vd[w] = in ? d[s] : T(0);
    }
    T* __restrict__ out = job.lo[e] + x3b_offset(p.v, job.nout, pl) + k;
#pragma unroll
    for (int u = 0; u < X3ZC; u++) {
        if (g0 + u < job.nout) {
            const int lp = u >> 1, odd = u & 1;  // compile-time after unrolling
            T sa = T(0), sd = T(0);
#pragma unroll
            for (int m = 0; m < h2; m++) {
                sa = fma_t<T>(va[lp + m], taps.a[HL - 2 + odd - 2 * m], sa);
                sd = fma_t<T>(vd[lp + m], taps.b[HL - 2 + odd - 2 * m], sd);
            }
            out[(size_t)(g0 + u) * pl] = sa + sd;
        }
    }
}

template <typename T, int HL>
__global__ __launch_bounds__(kA3ZThreads) void k_ext3b_adj_z(Adj3bZJob<T> job, Taps2<T> taps, Adj3ZHalo<T> hm)
{
    const int k = blockIdx.x * kA3ZThreads + threadIdx.x;
    if (k >= job.j.plane) return;
    ext3b_adj_z_lane<T, HL>(job, taps, hm, blockIdx.z, blockIdx.y * A3ZC, k);
}

// ---- geometry (host, no device) ---------------------------------------------------------------------------------------------------
struct X3bGeom {
    int nz[kVolMaxLevels + 1], nr[kVolMaxLevels + 1], nc[kVolMaxLevels + 1];  // [0]: the volume; [l]: the bands of level l
    size_t V;
    size_t quads() const { return 4 * V * nz[0] * nr[1] * nc[1]; }
    size_t approx() const { return V * nz[1] * nr[1] * nc[1]; }
};

// What every entry refuses: V < 1, levels outside 1 .. 13, a level that the level entries refuse (adjoint: also what the 2-D level
// adjoint refuses on a chunk of planes), and a stack of 2^31 planes or 2^40 elements or more (plane counts are ints; every product of
// the scratch formulas stays far below 2^64).
static bool ext3db_geom(X3bGeom& g, int V, int Nz, int Nr, int Nc, int hlen, int levels, bool adjoint)
{
    if (V < 1 || levels < 1 || levels > kVolMaxLevels) return false;
    g.V = (size_t)V, g.nz[0] = Nz, g.nr[0] = Nr, g.nc[0] = Nc;
    for (int l = 0; l < levels; l++) {
        if (!ext3_level_ok(g.nz[l], g.nr[l], g.nc[l], hlen)) return false;
        const long long planes = (long long)V * g.nz[l];
        if (adjoint && !adj2_level_ok(planes < kX3bChunk ? planes : kX3bChunk, g.nr[l], g.nc[l], hlen)) return false;
        g.nz[l + 1] = ext_half(g.nz[l], hlen), g.nr[l + 1] = ext_half(g.nr[l], hlen), g.nc[l + 1] = ext_half(g.nc[l], hlen);
    }
    const unsigned long long planes = (unsigned long long)V * (unsigned long long)Nz;
    if (planes >= (1ull << 31)) return false;
    return planes * ((unsigned long long)Nr * (unsigned long long)Nc) < (1ull << 40);  // (Nr * Nc < 2^31: no overflow)
}

static size_t ext3db_tmp(const X3bGeom& g, int levels) { return g.quads() + (levels > 1 ? 2 * g.approx() : 0); }
// the frames of the planes of the level that needs most
static size_t ext3db_frames(const X3bGeom& g, int hlen, int levels)
{
    size_t most = 0;
    for (int l = 0; l < levels; l++) {
        const size_t e = g.V * g.nz[l] * adj_frame_elems(g.nr[l], g.nc[l], hlen);
        most = e > most ? e : most;
    }
    return most;
}

template <typename T>
static bool ext3db_table_ok(T* const* b, int levels)
{
    if (!b || levels < 1 || levels > kVolMaxLevels) return false;
    for (int k = 0; k < 7 * levels + 1; k++)
        if (!b[k]) return false;
    return true;
}

// ---- launches ----------------------------------------------------------------------------------------------------------------------
template <typename T, int HL>
static int launch_ext3b_z(bool fwd, const Ext3bZJob<T>& zj, unsigned pairs, const Taps2<T>& taps)
{
    const dim3 grid(idiv_up(zj.plane, kX3ZThreads), idiv_up(zj.nout, X3ZC), pairs);
    return launch_lds(fwd ? k_ext3b_ana_z<T, HL> : k_ext3b_syn_z<T, HL>, grid, dim3(kX3ZThreads), 0, zj, taps);
}
template <typename T, int HL>
static int launch_ext3b_adj_z(const Adj3bZJob<T>& zj, unsigned pairs, const Taps2<T>& taps, const Adj3ZHalo<T>& hm)
{
    const dim3 grid(idiv_up(zj.j.plane, kA3ZThreads), idiv_up(zj.j.nz, A3ZC), pairs);
    return launch_lds(k_ext3b_adj_z<T, HL>, grid, dim3(kA3ZThreads), 0, zj, taps, hm);
}

// the z pass of a level over the 4 V pairs, in chunks of a grid dimension
template <typename T>
static int run_ext3b_z(int hlen, bool fwd, Ext3bZJob<T> zj, size_t V, const Taps2<T>& taps)
{
    for (size_t p0 = 0; p0 < 4 * V; p0 += kX3bChunk) {
        const unsigned cnt = (unsigned)(4 * V - p0 < (size_t)kX3bChunk ? 4 * V - p0 : (size_t)kX3bChunk);
        zj.pair0 = p0;
        if (const int rc = with_filter_length(hlen, [&](auto hl) { return launch_ext3b_z<T, decltype(hl)::value>(fwd, zj, cnt, taps); }); rc != PDWT_OK) return rc;
    }
    return PDWT_OK;
}
template <typename T>
static int run_ext3b_adj_z(int hlen, Adj3bZJob<T> zj, size_t V, const Taps2<T>& taps, const Adj3ZHalo<T>& hm)
{
    for (size_t p0 = 0; p0 < 4 * V; p0 += kX3bChunk) {
        const unsigned cnt = (unsigned)(4 * V - p0 < (size_t)kX3bChunk ? 4 * V - p0 : (size_t)kX3bChunk);
        zj.pair0 = p0;
        if (const int rc = with_filter_length(hlen, [&](auto hl) { return launch_ext3b_adj_z<T, decltype(hl)::value>(zj, cnt, taps, hm); }); rc != PDWT_OK) return rc;
    }
    return PDWT_OK;
}

// the x-y pass of a level over the `planes` planes of a stack, in chunks of a grid dimension: vol is the stack of nr x nc planes (the
// source of the forward, the result of the inverse), q0 the first of the four quadrant stacks, sq elements apart
template <typename T>
static int run_ext3b_xy(int hlen, bool fwd, const T* src, T* dst, T* q0, size_t sq, size_t planes, int nr, int nc, int mode, const Taps2<T>& taps)
{
    const int hr = ext_half(nr, hlen), hc = ext_half(nc, hlen);
    for (size_t p0 = 0; p0 < planes; p0 += kX3bChunk) {
        const int cnt = (int)(planes - p0 < (size_t)kX3bChunk ? planes - p0 : (size_t)kX3bChunk);
        Ext3XYJob<T> xy{};
        xy.src = src ? src + p0 * nr * nc : nullptr;
        xy.dst = dst ? dst + p0 * nr * nc : nullptr;
        for (int q = 0; q < 4; q++) xy.q[q] = q0 + q * sq + p0 * hr * hc;
        xy.nr = nr, xy.nc = nc, xy.hr = hr, xy.hc = hc, xy.mode = mode;
        if (const int rc = run_ext3_xy<T>(hlen, fwd, xy, cnt, taps); rc != PDWT_OK) return rc;
    }
    return PDWT_OK;
}

// ---- drivers -------------------------------------------------------------------------------------------------------------------
// Level l = 1 .. levels reads the stack of shape [l - 1] and gives the eight band stacks of shape [l]: aaa of the last level is band 0
// of the table, of any other one of the two approximation stacks in turn; the details are the bands 1 + 7 * (levels - l) ...
template <typename T>
static T* ext3db_approx(T* ping, size_t stack, int l) { return ping + (size_t)((l - 1) & 1) * stack; }  // aaa of level l < levels

template <typename T>
static int ext3db_forward(const T* src, T* const* b, int V, int Nz, int Nr, int Nc, int levels, int mode, const typename FiltersOf<T>::type* f, T* tmp, bool adjoint)
{
    X3bGeom g;
    if (!src || !f || !tmp || mode < 0 || mode >= EXT_NUM_MODES || !ext3db_table_ok(b, levels) || !ext3db_geom(g, V, Nz, Nr, Nc, f->hlen, levels, adjoint))
        return PDWT_EINVAL;
    const int hlen = f->hlen;
    const Taps2<T> taps = taps_fwd<T>(f);
    T* const ping = tmp + g.quads();
    for (int l = 1; l <= levels; l++) {
        const int nz = g.nz[l - 1], nr = g.nr[l - 1], nc = g.nc[l - 1], hz = g.nz[l], hr = g.nr[l], hc = g.nc[l];
        const size_t sq = g.V * nz * hr * hc;
        const T* in = l == 1 ? src : ext3db_approx(ping, g.approx(), l - 1);
        T* lev[8];
        lev[0] = l == levels ? b[0] : ext3db_approx(ping, g.approx(), l);
        for (int k = 0; k < 7; k++) lev[1 + k] = b[band3(levels, l, k)];
        if (const int rc = run_ext3b_xy<T>(hlen, true, in, nullptr, tmp, sq, g.V * nz, nr, nc, mode, taps); rc != PDWT_OK) return rc;
        Ext3bZJob<T> zj{};
        for (int q = 0; q < 4; q++) {
            zj.src[q] = tmp + q * sq;
            zj.lo[q] = lev[ext3_band(q, 0)];
            zj.hi[q] = lev[ext3_band(q, 1)];
        }
        zj.nin = nz, zj.nout = hz, zj.plane = hr * hc, zj.mode = mode;
        if (const int rc = run_ext3b_z<T>(hlen, true, zj, g.V, taps); rc != PDWT_OK) return rc;
    }
    return PDWT_OK;
}

// mode < 0: the inverse; a mode: the adjoint of the forward transform.  Coarse to fine: the result of level l is aaa of level l - 1.
template <typename T>
static int ext3db_backward(T* dst, T* const* b, int V, int Nz, int Nr, int Nc, int levels, int mode, const typename FiltersOf<T>::type* f, T* tmp)
{
    const bool adjoint = mode >= 0;
    X3bGeom g;
    if (!dst || !f || !tmp || mode >= EXT_NUM_MODES || !ext3db_table_ok(b, levels) || !ext3db_geom(g, V, Nz, Nr, Nc, f->hlen, levels, adjoint)) return PDWT_EINVAL;
    const int hlen = f->hlen;
    const Taps2<T> taps = adjoint ? taps_adj<T>(f) : taps_inv<T>(f);
    T* const ping = tmp + g.quads();
    T* const frames = ping + (levels > 1 ? 2 * g.approx() : 0);
    for (int l = levels; l >= 1; l--) {
        const int nz = g.nz[l - 1], nr = g.nr[l - 1], nc = g.nc[l - 1], hz = g.nz[l], hr = g.nr[l], hc = g.nc[l];
        const size_t sq = g.V * nz * hr * hc;
        T* out = l == 1 ? dst : ext3db_approx(ping, g.approx(), l - 1);
        T* lev[8];
        lev[0] = l == levels ? b[0] : ext3db_approx(ping, g.approx(), l);
        for (int k = 0; k < 7; k++) lev[1 + k] = b[band3(levels, l, k)];
        if (!adjoint) {
            Ext3bZJob<T> zj{};
            for (int q = 0; q < 4; q++) {
                zj.src[q] = lev[ext3_band(q, 0)];
                zj.src2[q] = lev[ext3_band(q, 1)];
                zj.lo[q] = tmp + q * sq;
            }
            zj.nin = hz, zj.nout = nz, zj.plane = hr * hc, zj.mode = 0;
            if (const int rc = run_ext3b_z<T>(hlen, false, zj, g.V, taps); rc != PDWT_OK) return rc;
            if (const int rc = run_ext3b_xy<T>(hlen, false, nullptr, out, tmp, sq, g.V * nz, nr, nc, 0, taps); rc != PDWT_OK) return rc;
            continue;
        }
        Adj3bZJob<T> zj{};
        for (int q = 0; q < 4; q++) {
            zj.j.lo[q] = lev[ext3_band(q, 0)];
            zj.j.hi[q] = lev[ext3_band(q, 1)];
            zj.j.q[q] = tmp + q * sq;
        }
        zj.j.nz = nz, zj.j.hz = hz, zj.j.plane = hr * hc;
        if (const int rc = run_ext3b_adj_z<T>(hlen, zj, g.V, taps, adj3_z_halo<T>(nz, hlen, mode, taps)); rc != PDWT_OK) return rc;
        // the quadrants q = 2 * x band + y band are A, H, V, D of the 2-D level adjoint; a chunk of planes has its own frames
        const size_t planes = g.V * nz, fe = adj_frame_elems(nr, nc, hlen), img = (size_t)nr * nc, qp = (size_t)hr * hc;
        for (size_t p0 = 0; p0 < planes; p0 += kX3bChunk) {
            const int cnt = (int)(planes - p0 < (size_t)kX3bChunk ? planes - p0 : (size_t)kX3bChunk);
            const T* q = tmp + p0 * qp;
            if (const int rc = adj2_forward_level<T>(out + p0 * img, q, q + sq, q + 2 * sq, q + 3 * sq, cnt, nr, nc, mode, f, frames + p0 * fe); rc != PDWT_OK) return rc;
        }
    }
    return PDWT_OK;
}

template <typename T>
static int ext3db_inverse_adjoint(const T* src, T* const* b, int V, int Nz, int Nr, int Nc, int levels, const typename FiltersOf<T>::type* f, T* tmp)
{
    typename FiltersOf<T>::type g;
    if (!adj_inverse_bank<T>(g, f)) return PDWT_EINVAL;
    return ext3db_forward<T>(src, b, V, Nz, Nr, Nc, levels, EXT_ZERO, &g, tmp, true);
}

}  // namespace pdwt

using namespace pdwt;

extern "C" {
long long pdwt_ext3db_tmp_elems(int V, int Nz, int Nr, int Nc, int hlen, int levels)
{
    X3bGeom g;
    if (!ext3db_geom(g, V, Nz, Nr, Nc, hlen, levels, false)) return PDWT_EINVAL;
    return (long long)ext3db_tmp(g, levels);
}
long long pdwt_ext3db_adjoint_tmp_elems(int V, int Nz, int Nr, int Nc, int hlen, int levels)
{
    X3bGeom g;
    if (!ext3db_geom(g, V, Nz, Nr, Nc, hlen, levels, true)) return PDWT_EINVAL;
    return (long long)(ext3db_tmp(g, levels) + ext3db_frames(g, hlen, levels));
}
int pdwt_ext3db_forward_f32(const float* d_src, float* const* d_bands, int V, int Nz, int Nr, int Nc, int levels, int mode, const pdwt_filters_f32* f, float* d_tmp)
{
    return ext3db_forward<float>(d_src, d_bands, V, Nz, Nr, Nc, levels, mode, f, d_tmp, false);
}
int pdwt_ext3db_forward_f64(const double* d_src, double* const* d_bands, int V, int Nz, int Nr, int Nc, int levels, int mode, const pdwt_filters_f64* f, double* d_tmp)
{
    return ext3db_forward<double>(d_src, d_bands, V, Nz, Nr, Nc, levels, mode, f, d_tmp, false);
}
int pdwt_ext3db_inverse_f32(float* d_dst, float* const* d_bands, int V, int Nz, int Nr, int Nc, int levels, const pdwt_filters_f32* f, float* d_tmp)
{
    return ext3db_backward<float>(d_dst, d_bands, V, Nz, Nr, Nc, levels, -1, f, d_tmp);
}
int pdwt_ext3db_inverse_f64(double* d_dst, double* const* d_bands, int V, int Nz, int Nr, int Nc, int levels, const pdwt_filters_f64* f, double* d_tmp)
{
    return ext3db_backward<double>(d_dst, d_bands, V, Nz, Nr, Nc, levels, -1, f, d_tmp);
}
int pdwt_ext3db_forward_adjoint_f32(float* d_dst, float* const* d_bands, int V, int Nz, int Nr, int Nc, int levels, int mode, const pdwt_filters_f32* f, float* d_tmp)
{
    if (mode < 0) return PDWT_EINVAL;
    return ext3db_backward<float>(d_dst, d_bands, V, Nz, Nr, Nc, levels, mode, f, d_tmp);
}
int pdwt_ext3db_forward_adjoint_f64(double* d_dst, double* const* d_bands, int V, int Nz, int Nr, int Nc, int levels, int mode, const pdwt_filters_f64* f, double* d_tmp)
{
    if (mode < 0) return PDWT_EINVAL;
    return ext3db_backward<double>(d_dst, d_bands, V, Nz, Nr, Nc, levels, mode, f, d_tmp);
}
int pdwt_ext3db_inverse_adjoint_f32(const float* d_src, float* const* d_bands, int V, int Nz, int Nr, int Nc, int levels, const pdwt_filters_f32* f, float* d_tmp)
{
    return ext3db_inverse_adjoint<float>(d_src, d_bands, V, Nz, Nr, Nc, levels, f, d_tmp);
}
int pdwt_ext3db_inverse_adjoint_f64(const double* d_src, double* const* d_bands, int V, int Nz, int Nr, int Nc, int levels, const pdwt_filters_f64* f, double* d_tmp)
{
    return ext3db_inverse_adjoint<double>(d_src, d_bands, V, Nz, Nr, Nc, levels, f, d_tmp);
}
}
