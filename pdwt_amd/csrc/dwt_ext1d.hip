// dwt_ext1d.hip -- the batched 1-D transform with signal-extension boundary modes (include/pdwt_hip.h "Batched 1-D DWT with boundary
// modes"; the class: BoundaryWavelets1D, include/wt_ext.h): pywt.wavedec(x, w, mode, level, axis=-1) of an Nr x Nc batch of rows.  The
// stages are the functions of dwt_ext1d.hpp; the kernels place the buffers and the barriers.
//   k_ext1d_fwd_fused  ALL levels of a pack of R rows in one launch: the rows are staged into LDS once (16-byte loads), every level is
//                      computed LDS -> LDS, its extension written into the halo cells of the line first (one barrier), the detail band
//                      goes from registers to HBM and only A_L leaves at the end.  Traffic: one read of the batch, one write of each band.
//   k_ext1d_inv_fused  coarse to fine the same way: A_L and each D_l are staged into LDS, the last level writes the rows to HBM.
//   k_ext1d_fwd / k_ext1d_inv  ONE level per launch over (tile of the row, row) flattened on grid.x, the bank length a run-time
//                      argument: rows that do not fit LDS, and the level entries of the C ABI.
// Both forms run ext1d_fwd_item / ext1d_inv_item: bit-identical results.  Barriers between LDS stages are LDS-only (lgkmcnt), so the
// detail stores of a level are not waited for (dwt1d_fused.hip).
//
// Row packing.  A workgroup takes R consecutive rows, R = the power of two >= 256 / N_1 (every thread has a position at level 1),
// at most 64 and as many as fit 32 KiB of LDS; long rows get R = 1.  Packs are grid.x; the last one may hold fewer rows.
// LDS rule.  Per row: forward stride(Nc) + stride(N_1) elements (ext1d_stride: line + halos, rounded to 16 bytes), inverse 3 * ru4(N_1)
// (approximation in, detail in, output).  The fused path is taken when the larger of the two, for ONE row, fits 160 KiB.
#include <algorithm>

#include "dwt_ext1d.hpp"

namespace pdwt {

constexpr size_t kExt1dLdsMax = 160 * 1024;   // the hard ceiling of a workgroup (a literal: tests/test_newer_bank_matrix_cpu.py reads it)
constexpr size_t kExt1dPackLds = 32 * 1024;   // packs of several rows stay below this
static_assert(kExt1dLdsMax == kLdsMax, "one ceiling for every whole-signal kernel");

template <typename T, int HL>
__global__ __launch_bounds__(kExt1dThreads) void k_ext1d_fwd_fused(const T* __restrict__ src, Ext1dBands<T> b, int Nr, int R, int mode, Taps2<T> taps)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int NT = kExt1dThreads, off = ((HL - 2) + 3) & ~3;
    const int tid = threadIdx.x;
    const size_t row0 = (size_t)blockIdx.x * R;
    const int rows = (size_t)Nr - row0 < (size_t)R ? (int)((size_t)Nr - row0) : R;
    int n = b.n[0], cs = ext1d_stride(n, HL);
    T* cur = reinterpret_cast<T*>(smem);           // R lines of stride(n_0), later of n_2, n_4, ...
    T* nxt = cur + (size_t)R * cs;                 // R lines of stride(n_1), later of n_3, ...
    ext1d_stage_rows<T, NT>(cur, cs, off, src + row0 * (size_t)n, rows, n, tid);
    lds_barrier();
    ext1d_fill_halo<T, NT>(cur, cs, off, rows, n, HL, mode, tid);
    lds_barrier();
    for (int lev = 1; lev <= b.nlev; lev++) {
        const int N = b.n[lev], ns = ext1d_stride(N, HL);
        const bool last = lev == b.nlev;
        ext1d_fwd_level<T, HL, NT>(cur, cs, nxt, ns, off, rows, n, HL, taps, b.p[lev] + row0 * (size_t)N, last ? b.p[0] + row0 * (size_t)N : nullptr, tid);
        if (last) break;
        lds_barrier();
        ext1d_fill_halo<T, NT>(nxt, ns, off, rows, N, HL, mode, tid);
        lds_barrier();
        T* t = cur;
        cur = nxt, nxt = t;
        n = N, cs = ns;
    }
}

template <typename T, int HL>
__global__ __launch_bounds__(kExt1dThreads) void k_ext1d_inv_fused(T* __restrict__ dst, Ext1dBands<T> b, int Nr, int R, Taps2<T> taps)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int NT = kExt1dThreads;
    const int tid = threadIdx.x;
    const size_t row0 = (size_t)blockIdx.x * R;
    const int rows = (size_t)Nr - row0 < (size_t)R ? (int)((size_t)Nr - row0) : R;
    const size_t cap = (size_t)R * ext1d_ru4(b.n[1]);  // three buffers of R lines of up to N_1 coefficients
    T* a = reinterpret_cast<T*>(smem);
    T* o = a + cap;
    T* d = o + cap;
    const int L = b.nlev;
    ext1d_stage_rows<T, NT>(a, ext1d_ru4(b.n[L]), 0, b.p[0] + row0 * (size_t)b.n[L], rows, b.n[L], tid);
    for (int lev = L; lev >= 1; lev--) {
        const int N = b.n[lev], n = b.n[lev - 1], st = ext1d_ru4(N);
        ext1d_stage_rows<T, NT>(d, st, 0, b.p[lev] + row0 * (size_t)N, rows, N, tid);
        lds_barrier();
        if (lev == 1) {
            ext1d_inv_level<T, HL, NT>(a, st, d, st, dst + row0 * (size_t)n, n, rows, n, HL, taps, tid);
            break;
        }
        ext1d_inv_level<T, HL, NT>(a, st, d, st, o, ext1d_ru4(n), rows, n, HL, taps, tid);
        lds_barrier();  // the output is complete and every read of a and d is done before d is staged again
        T* t = a;
        a = o, o = t;
    }
}

template <typename T>
__global__ __launch_bounds__(kExt1dThreads) void k_ext1d_fwd(const T* __restrict__ src, T* __restrict__ a, T* __restrict__ d, int n, int N, int tiles, int mode, int hlen, Taps2<T> taps)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    T* win = reinterpret_cast<T*>(smem);  // [2 * kExt1dTile + hlen - 2]
    const int tid = threadIdx.x;
    const unsigned row = blockIdx.x / (unsigned)tiles, tile = blockIdx.x - row * (unsigned)tiles;
    const int i0 = (int)tile * kExt1dTile, cnt = N - i0 < kExt1dTile ? N - i0 : kExt1dTile;
    ext1d_stage_window<T, kExt1dThreads>(win, src + (size_t)row * n, n, 2 * i0 + 2 - hlen, 2 * cnt + hlen - 2, mode, tid);
    lds_barrier();
    const size_t o = (size_t)row * N + i0;
    ext1d_fwd_tile<T, kExt1dThreads>(win, cnt, hlen, taps, a + o, d + o, tid);
}

template <typename T>
__global__ __launch_bounds__(kExt1dThreads) void k_ext1d_inv(T* __restrict__ dst, const T* __restrict__ a, const T* __restrict__ d, int n, int N, int tiles, int hlen, Taps2<T> taps)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int WMAX = kExt1dTile + PDWT_MAX_FILTER_WIDTH / 2;
    T* wa = reinterpret_cast<T*>(smem);  // [kExt1dTile + hlen / 2 - 1]
    T* wd = wa + WMAX;
    const int tid = threadIdx.x;
    const unsigned row = blockIdx.x / (unsigned)tiles, tile = blockIdx.x - row * (unsigned)tiles;
    const int P = (n + 1) >> 1, p0 = (int)tile * kExt1dTile, cntp = P - p0 < kExt1dTile ? P - p0 : kExt1dTile;
    const int w = cntp + hlen / 2 - 1;  // p0 + w <= N: the last pair reads up to the last coefficient
    const size_t o = (size_t)row * N + p0;
    for (int k = tid; k < w; k += kExt1dThreads) {
        wa[k] = a[o + k];
        wd[k] = d[o + k];
    }
    lds_barrier();
    ext1d_inv_tile<T, kExt1dThreads>(wa, wd, cntp, n - 2 * p0, hlen, taps, dst + (size_t)row * n + 2 * p0, tid);
}

// ---- geometry and the plan of the fused path (host, no device) ------------------------------------------------------------------------
// what every entry refuses: a bad bank length, a row shorter than hlen - 1 (the halo must fold at most once per period), sizes the
// 32-bit indices cannot take
static bool ext1d_ok(long long nr, long long nc, int hlen)
{
    if (hlen < 2 || hlen > PDWT_MAX_FILTER_WIDTH || (hlen & 1)) return false;
    if (nr < 1 || nc < 1 || nc < hlen - 1 || nc > (1 << 30)) return false;
    return (unsigned long long)nr * (unsigned long long)nc < (1ull << 31);
}
static bool ext1d_levels_ok(int levels) { return levels >= 1 && levels <= kExt1dMaxLev; }

struct Ext1dPlan {
    bool fused;
    int R;
    size_t lds_fwd, lds_inv;  // of a workgroup (R rows)
};
static Ext1dPlan ext1d_plan(int nc, int hlen, int levels, size_t elem)
{
    const int n1 = ext_half(nc, hlen);
    const size_t fwd = ((size_t)ext1d_stride(nc, hlen) + ext1d_stride(n1, hlen)) * elem, inv = 3 * (size_t)ext1d_ru4(n1) * elem;
    const size_t row = std::max(fwd, inv);
    Ext1dPlan p{row <= kExt1dLdsMax, 1, fwd, inv};
    if (!p.fused) return p;
    int R = 1;
    while (R < 64 && R * n1 < kExt1dThreads && 2 * R * row <= kExt1dPackLds) R *= 2;
    p.R = R, p.lds_fwd = R * fwd, p.lds_inv = R * inv;
    return p;
}

template <typename T>
static bool ext1d_fill_bands(Ext1dBands<T>& b, T* const* c, int nc, int hlen, int levels)
{
    if (!c) return false;
    b.nlev = levels, b.n[0] = nc;
    for (int l = 1; l <= levels; l++) b.n[l] = ext_half(b.n[l - 1], hlen);
    for (int l = 0; l <= levels; l++) {
        if (!c[l]) return false;
        b.p[l] = c[l];
    }
    return true;
}

// ---- drivers -----------------------------------------------------------------------------------------------------------------
template <typename T>
static int ext1d_forward_level(const T* src, T* a, T* d, int nr, int nc, int mode, const typename FiltersOf<T>::type* f)
{
    if (!src || !a || !d || !f || mode < 0 || mode >= EXT_NUM_MODES || !ext1d_ok(nr, nc, f->hlen)) return PDWT_EINVAL;
    const int hlen = f->hlen, N = ext_half(nc, hlen), tiles = idiv_up(N, kExt1dTile);
    const size_t lds = sizeof(T) * (2 * kExt1dTile + PDWT_MAX_FILTER_WIDTH);
    hipLaunchKernelGGL((k_ext1d_fwd<T>), dim3((unsigned)nr * (unsigned)tiles), dim3(kExt1dThreads), lds, stream(), src, a, d, nc, N, tiles, mode, hlen, taps_fwd<T>(f));
    PDWT_HIP_TRY(hipGetLastError());
    return PDWT_OK;
}

template <typename T>
static int ext1d_inverse_level(T* dst, const T* a, const T* d, int nr, int nc, const typename FiltersOf<T>::type* f)
{
    if (!dst || !a || !d || !f || !ext1d_ok(nr, nc, f->hlen)) return PDWT_EINVAL;
    const int hlen = f->hlen, N = ext_half(nc, hlen), tiles = idiv_up((nc + 1) >> 1, kExt1dTile);
    const size_t lds = sizeof(T) * 2 * (kExt1dTile + PDWT_MAX_FILTER_WIDTH / 2);
    hipLaunchKernelGGL((k_ext1d_inv<T>), dim3((unsigned)nr * (unsigned)tiles), dim3(kExt1dThreads), lds, stream(), dst, a, d, nc, N, tiles, hlen, taps_inv<T>(f));
    PDWT_HIP_TRY(hipGetLastError());
    return PDWT_OK;
}

template <typename T, int HL>
static int launch_ext1d_fwd_fused(const T* src, const Ext1dBands<T>& b, int nr, int mode, const Ext1dPlan& p, const Taps2<T>& taps)
{
    if (p.lds_fwd > 64 * 1024)
        if (const int rc = lds_opt_in_ptr((const void*)k_ext1d_fwd_fused<T, HL>); rc != PDWT_OK) return rc;
    hipLaunchKernelGGL((k_ext1d_fwd_fused<T, HL>), dim3(idiv_up(nr, p.R)), dim3(kExt1dThreads), p.lds_fwd, stream(), src, b, nr, p.R, mode, taps);
    PDWT_HIP_TRY(hipGetLastError());
    return PDWT_EXT1D_FUSED;
}
template <typename T, int HL>
static int launch_ext1d_inv_fused(T* dst, const Ext1dBands<T>& b, int nr, const Ext1dPlan& p, const Taps2<T>& taps)
{
    if (p.lds_inv > 64 * 1024)
        if (const int rc = lds_opt_in_ptr((const void*)k_ext1d_inv_fused<T, HL>); rc != PDWT_OK) return rc;
    hipLaunchKernelGGL((k_ext1d_inv_fused<T, HL>), dim3(idiv_up(nr, p.R)), dim3(kExt1dThreads), p.lds_inv, stream(), dst, b, nr, p.R, taps);
    PDWT_HIP_TRY(hipGetLastError());
    return PDWT_EXT1D_FUSED;
}

// The approximation of level l (1 .. L - 1) of the per-level path: the halves of d_tmp in turn (each nr x N_1 elements), as the
// ping buffers of BoundaryWavelets.
template <typename T>
static T* ext1d_tmp_of(T* tmp, int nr, int n1, int l) { return tmp + ((l - 1) & 1) * (size_t)nr * n1; }

template <typename T>
static int ext1d_forward(const T* src, T* const* c, int nr, int nc, int levels, int mode, const typename FiltersOf<T>::type* f, T* tmp)
{
    Ext1dBands<T> b;
    if (!src || !f || mode < 0 || mode >= EXT_NUM_MODES || !ext1d_levels_ok(levels) || !ext1d_ok(nr, nc, f->hlen) || !ext1d_fill_bands(b, c, nc, f->hlen, levels))
        return PDWT_EINVAL;
    const int hlen = f->hlen;
    const Ext1dPlan p = ext1d_plan(nc, hlen, levels, sizeof(T));
    if (p.fused) {
        const Taps2<T> taps = taps_fwd<T>(f);
        return with_filter_length<2>(hlen, [&](auto hl) { return launch_ext1d_fwd_fused<T, decltype(hl)::value>(src, b, nr, mode, p, taps); });
    }
    if (levels > 1 && !tmp) return PDWT_EINVAL;
    for (int l = 1; l <= levels; l++) {
        T* a = l == levels ? b.p[0] : ext1d_tmp_of(tmp, nr, b.n[1], l);
        if (const int rc = ext1d_forward_level<T>(src, a, b.p[l], nr, b.n[l - 1], mode, f); rc != PDWT_OK) return rc;
        src = a;
    }
    return PDWT_EXT1D_LEVELS;
}

template <typename T>
static int ext1d_inverse(T* dst, T* const* c, int nr, int nc, int levels, const typename FiltersOf<T>::type* f, T* tmp)
{
    Ext1dBands<T> b;
    if (!dst || !f || !ext1d_levels_ok(levels) || !ext1d_ok(nr, nc, f->hlen) || !ext1d_fill_bands(b, c, nc, f->hlen, levels)) return PDWT_EINVAL;
    const int hlen = f->hlen;
    const Ext1dPlan p = ext1d_plan(nc, hlen, levels, sizeof(T));
    if (p.fused) {
        const Taps2<T> taps = taps_inv<T>(f);
        return with_filter_length<2>(hlen, [&](auto hl) { return launch_ext1d_inv_fused<T, decltype(hl)::value>(dst, b, nr, p, taps); });
    }
    if (levels > 1 && !tmp) return PDWT_EINVAL;
    for (int l = levels; l >= 1; l--) {
        const T* a = l == levels ? b.p[0] : ext1d_tmp_of(tmp, nr, b.n[1], l);
        T* out = l == 1 ? dst : ext1d_tmp_of(tmp, nr, b.n[1], l - 1);
        if (const int rc = ext1d_inverse_level<T>(out, a, b.p[l], nr, b.n[l - 1], f); rc != PDWT_OK) return rc;
    }
    return PDWT_EXT1D_LEVELS;
}

}  // namespace pdwt

using namespace pdwt;

extern "C" {
int pdwt_num_bands_ext1d(int Nc, int hlen, int levels)
{
    if (!ext1d_levels_ok(levels) || !ext1d_ok(1, Nc, hlen)) return PDWT_EINVAL;
    return levels + 1;
}
long long pdwt_ext1d_band_len(int Nc, int hlen, int levels, int num)
{
    const int nb = pdwt_num_bands_ext1d(Nc, hlen, levels);
    if (nb < 0 || num < 0 || num >= nb) return PDWT_EINVAL;
    const int lev = num == 0 ? levels : num;  // [A_L, D_1, ..., D_L]
    for (int l = 0; l < lev; l++) Nc = ext_half(Nc, hlen);
    return Nc;
}
int pdwt_ext1d_fused(int Nc, int hlen, int levels, int elem_size)
{
    if (pdwt_num_bands_ext1d(Nc, hlen, levels) < 0 || (elem_size != 4 && elem_size != 8)) return PDWT_EINVAL;
    return ext1d_plan(Nc, hlen, levels, (size_t)elem_size).fused ? 1 : 0;
}
long long pdwt_ext1d_tmp_elems(int Nr, int Nc, int hlen, int levels, int elem_size)
{
    const int fu = pdwt_ext1d_fused(Nc, hlen, levels, elem_size);
    if (fu < 0 || !ext1d_ok(Nr, Nc, hlen)) return PDWT_EINVAL;
    return (fu || levels == 1) ? 0 : 2ll * Nr * ext_half(Nc, hlen);
}
int pdwt_ext1d_forward_level_f32(const float* d_src, float* d_a, float* d_d, int nr, int nc, int mode, const pdwt_filters_f32* f)
{
    return ext1d_forward_level<float>(d_src, d_a, d_d, nr, nc, mode, f);
}
int pdwt_ext1d_forward_level_f64(const double* d_src, double* d_a, double* d_d, int nr, int nc, int mode, const pdwt_filters_f64* f)
{
    return ext1d_forward_level<double>(d_src, d_a, d_d, nr, nc, mode, f);
}
int pdwt_ext1d_inverse_level_f32(float* d_dst, const float* d_a, const float* d_d, int nr, int nc, const pdwt_filters_f32* f)
{
    return ext1d_inverse_level<float>(d_dst, d_a, d_d, nr, nc, f);
}
int pdwt_ext1d_inverse_level_f64(double* d_dst, const double* d_a, const double* d_d, int nr, int nc, const pdwt_filters_f64* f)
{
    return ext1d_inverse_level<double>(d_dst, d_a, d_d, nr, nc, f);
}
int pdwt_ext1d_forward_f32(const float* d_src, float* const* d_coeffs, int nr, int nc, int levels, int mode, const pdwt_filters_f32* f, float* d_tmp)
{
    return ext1d_forward<float>(d_src, d_coeffs, nr, nc, levels, mode, f, d_tmp);
}
int pdwt_ext1d_forward_f64(const double* d_src, double* const* d_coeffs, int nr, int nc, int levels, int mode, const pdwt_filters_f64* f, double* d_tmp)
{
    return ext1d_forward<double>(d_src, d_coeffs, nr, nc, levels, mode, f, d_tmp);
}
int pdwt_ext1d_inverse_f32(float* d_dst, float* const* d_coeffs, int nr, int nc, int levels, const pdwt_filters_f32* f, float* d_tmp)
{
    return ext1d_inverse<float>(d_dst, d_coeffs, nr, nc, levels, f, d_tmp);
}
int pdwt_ext1d_inverse_f64(double* d_dst, double* const* d_coeffs, int nr, int nc, int levels, const pdwt_filters_f64* f, double* d_tmp)
{
    return ext1d_inverse<double>(d_dst, d_coeffs, nr, nc, levels, f, d_tmp);
}
}
