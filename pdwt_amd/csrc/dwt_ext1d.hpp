// dwt_ext1d.hpp -- the stages of the batched 1-D transform with signal-extension boundary modes (dwt_ext1d.hip; include/pdwt_hip.h
// "Batched 1-D DWT with boundary modes"): the LDS line layout, the halo fill, one analysis / synthesis level over a pack of rows, and the
// window staging of the per-level kernels.  Every stage takes the thread count as a template argument and the thread index as an
// argument and contains no barrier, so the same code runs on the device (NT = 256, the kernels place the barriers between the stages)
// and on a CPU with NT = 1, tid = 0 (a host program can include this header and run whole pipelines under a sanitizer).
//
// One level of a line of n samples, bank of even length F (the formulas of dwt_ext.hpp): N = (n + F - 1) / 2,
//   a[i] = sum_k L[k] xe[2i + 1 - k]                                   window = xe[2i + 2 - F .. 2i + 1], F samples
//   x[2p], x[2p + 1] = sum_m a[p + m] IL[F-2-2m | F-1-2m] + d[p + m] IH[F-2-2m | F-1-2m],  m = 0 .. F/2 - 1   (no extension)
// Summation order (both kernel forms go through ext1d_fwd_item / ext1d_inv_item, hence agree bit for bit): one FMA per tap in ascending
// order of the window sample / of the coefficient; the inverse keeps the a and d sums apart and adds them once.
//
// LDS line of the forward transform: [hl cells | n samples | F - 1 cells], hl = F - 2 rounded up to 4 elements, the line stride a multiple
// of 4 elements: the samples start 16-byte aligned (16-byte staging stores), and the window of position i starts at the EVEN cell
// hl - (F - 2) + 2i, so a work item reads its window as F / 2 aligned pairs (ds_read_b64 / b128): consecutive lanes read consecutive
// pairs, which is free of the 2-way bank conflict that stride-2 scalar reads have.  The extension is written once per level into the
// F - 2 cells to the left and the F - 1 cells to the right (the last window of an odd line reaches xe[n + F - 2]).
#pragma once
#include "dwt_ext.hpp"

namespace pdwt {

constexpr int kExt1dThreads = 256;
constexpr int kExt1dMaxLev = 32;
constexpr int kExt1dTile = 1024;  // per-level kernels: band positions (forward) / sample pairs (inverse) per workgroup

template <typename T> struct Ext1dVec;
template <> struct Ext1dVec<float> {
    typedef float v2 __attribute__((ext_vector_type(2)));
    typedef float v16 __attribute__((ext_vector_type(4)));
    static constexpr int NV = 4;
};
template <> struct Ext1dVec<double> {
    typedef double v2 __attribute__((ext_vector_type(2)));
    typedef double v16 __attribute__((ext_vector_type(2)));
    static constexpr int NV = 2;
};

template <typename T>
struct Ext1dBands {
    T* p[kExt1dMaxLev + 1];   // p[0] = A_L, p[l] = D_l (l = 1 the finest), each Nr x n[l] row-major (n[L] for p[0])
    int n[kExt1dMaxLev + 1];  // n[0] = Nc, n[l] = coefficients per row of level l
    int nlev;
};

__host__ __device__ inline int ext1d_ru4(int v) { return (v + 3) & ~3; }
__host__ __device__ inline int ext1d_hl(int F) { return ext1d_ru4(F - 2); }                            // left halo cells (aligned)
__host__ __device__ inline int ext1d_stride(int n, int F) { return ext1d_ru4(ext1d_hl(F) + n + F - 1); }  // forward line

__host__ __device__ __forceinline__ float ext1d_fma(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__host__ __device__ __forceinline__ double ext1d_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }

// opaque_zero() of vol3d.hpp where it exists; a plain 0 on the host
__host__ __device__ __forceinline__ int ext1d_zero()
{
#if defined(__HIP_DEVICE_COMPILE__)
    return opaque_zero();
#else
    return 0;
#endif
}
// HL = 0: the length is a run-time argument (the per-level kernels: 4 kernels instead of 80).  A compile-time bank whose 2 * HL taps do
// not fit the scalar registers next to everything else is indexed through the opaque zero, as in dwt_ext.hpp.
template <typename T, int HL>
constexpr bool ext1d_opaque_taps() { return HL == 0 || HL * sizeof(T) > 128; }

// (lo, hi) of one position from its window p[0 .. F-1] (p aligned to a pair)
template <typename T, int HL>
__host__ __device__ __forceinline__ void ext1d_fwd_item(const T* p, int hlen, const Taps2<T>& taps, T& lo, T& hi)
{
    using V2 = typename Ext1dVec<T>::v2;
    const int F = HL ? HL : hlen;
    const int z0 = ext1d_opaque_taps<T, HL>() ? ext1d_zero() : 0;
    T sl = T(0), sh = T(0);
    auto step = [&](int m) {
        const V2 v = *reinterpret_cast<const V2*>(p + 2 * m);
        sl = ext1d_fma(v[0], taps.a[F - 1 - 2 * m + z0], sl);
        sh = ext1d_fma(v[0], taps.b[F - 1 - 2 * m + z0], sh);
        sl = ext1d_fma(v[1], taps.a[F - 2 - 2 * m + z0], sl);
        sh = ext1d_fma(v[1], taps.b[F - 2 - 2 * m + z0], sh);
    };
    if constexpr (ext1d_opaque_taps<T, HL>()) {  // a real loop, four steps at a time: the taps are loaded as they are used
#pragma unroll 4
        for (int m = 0; m < F / 2; m++) step(m);
    } else {
#pragma unroll
        for (int m = 0; m < F / 2; m++) step(m);
    }
    lo = sl, hi = sh;
}

// (x[2p], x[2p + 1]) from the coefficients pa[0 .. F/2 - 1], pd[0 .. F/2 - 1] (= a[p ..], d[p ..])
template <typename T, int HL>
__host__ __device__ __forceinline__ void ext1d_inv_item(const T* pa, const T* pd, int hlen, const Taps2<T>& taps, T& x0, T& x1)
{
    const int F = HL ? HL : hlen;
    const int z0 = ext1d_opaque_taps<T, HL>() ? ext1d_zero() : 0;
    T ae = T(0), ao = T(0), de = T(0), dd = T(0);
    auto step = [&](int m) {
        const T ca = pa[m], cd = pd[m];
        ae = ext1d_fma(ca, taps.a[F - 2 - 2 * m + z0], ae);
        ao = ext1d_fma(ca, taps.a[F - 1 - 2 * m + z0], ao);
        de = ext1d_fma(cd, taps.b[F - 2 - 2 * m + z0], de);
        dd = ext1d_fma(cd, taps.b[F - 1 - 2 * m + z0], dd);
    };
    if constexpr (ext1d_opaque_taps<T, HL>()) {
#pragma unroll 4
        for (int m = 0; m < F / 2; m++) step(m);
    } else {
#pragma unroll
        for (int m = 0; m < F / 2; m++) step(m);
    }
    x0 = ae + de, x1 = ao + dd;
}

// ---- packs of whole rows (the fused kernels) ----------------------------------------------------------------------------------
// Copy `rows` consecutive rows of n elements (contiguous at src) to the lines dst + r * stride + off: 16-byte loads and stores when
// every row starts aligned (n a multiple of the vector, src, off and stride aligned: the caller's lines are), else element-wise.
template <typename T, int NT>
__host__ __device__ __forceinline__ void ext1d_stage_rows(T* dst, int stride, int off, const T* __restrict__ src, int rows, int n, int tid)
{
    using V = typename Ext1dVec<T>::v16;
    constexpr int NV = Ext1dVec<T>::NV;
    if ((n % NV) == 0 && (reinterpret_cast<uintptr_t>(src) & 15) == 0) {
        const int nch = n / NV, total = rows * nch;
        for (int e = tid; e < total; e += NT) {
            const int r = rows == 1 ? 0 : e / nch, c = e - r * nch;
            reinterpret_cast<V*>(dst + (size_t)r * stride + off)[c] = reinterpret_cast<const V*>(src)[e];
        }
    } else {
        const int total = rows * n;
        for (int e = tid; e < total; e += NT) {
            const int r = rows == 1 ? 0 : e / n, c = e - r * n;
            dst[(size_t)r * stride + off + c] = src[e];
        }
    }
}

// Write the extension of every line into its halo cells: xe[2 - F .. -1] and xe[n .. n + F - 2].  ext_index is a full modulo / fold (the
// halo may be as long as the line: F - 2 = n - 1).  Reads samples, writes halo cells only: needs a barrier before and after, none inside.
template <typename T, int NT>
__host__ __device__ __forceinline__ void ext1d_fill_halo(T* lines, int stride, int off, int rows, int n, int F, int mode, int tid)
{
    const int hc = 2 * F - 3, total = rows * hc;
    for (int e = tid; e < total; e += NT) {
        const int r = e / hc, k = e - r * hc;
        const int s = k < F - 2 ? k - (F - 2) : n + (k - (F - 2));
        const int j = ext_index(s, n, mode);
        T* line = lines + (size_t)r * stride + off;
        line[s] = j < 0 ? T(0) : line[j];
    }
}

// One analysis level of a pack: lines of n samples at cur (stride cs) -> the detail rows gd[r * N + i] (global, the pack's first row)
// and the approximation either to ga (global; the last level) or, ga == NULL, to the lines at nxt (stride ns).
template <typename T, int HL, int NT>
__host__ __device__ __forceinline__ void ext1d_fwd_level(const T* cur, int cs, T* nxt, int ns, int off, int rows, int n, int hlen, const Taps2<T>& taps,
                                                         T* __restrict__ gd, T* __restrict__ ga, int tid)
{
    const int F = HL ? HL : hlen, N = ext_half(n, F), total = rows * N;
    const T* base = cur + off - (F - 2);
    for (int e = tid; e < total; e += NT) {
        const int r = rows == 1 ? 0 : e / N, i = e - r * N;
        T lo, hi;
        ext1d_fwd_item<T, HL>(base + (size_t)r * cs + 2 * i, hlen, taps, lo, hi);
        gd[e] = hi;
        if (ga) ga[e] = lo;
        else nxt[(size_t)r * ns + off + i] = lo;
    }
}

// One synthesis level of a pack: coefficient lines a (stride as) and d (stride ds), no halo -> n samples per row at out + r * os (LDS
// lines or, with os = n, the global rows of the pack).  Two samples per work item.
template <typename T, int HL, int NT>
__host__ __device__ __forceinline__ void ext1d_inv_level(const T* a, int as, const T* d, int ds, T* out, int os, int rows, int n, int hlen, const Taps2<T>& taps, int tid)
{
    const int P = (n + 1) >> 1, total = rows * P;
    for (int e = tid; e < total; e += NT) {
        const int r = rows == 1 ? 0 : e / P, p = e - r * P;
        T x0, x1;
        ext1d_inv_item<T, HL>(a + (size_t)r * as + p, d + (size_t)r * ds + p, hlen, taps, x0, x1);
        T* o = out + (size_t)r * os + 2 * p;
        o[0] = x0;
        if (2 * p + 1 < n) o[1] = x1;
    }
}

// ---- tiles of one row (the per-level kernels) -------------------------------------------------------------------------------------
// Stage xe[s0 .. s0 + w) of the row into win: plain addressing when the window lies inside the row (a workgroup-uniform branch), the
// index map of the mode otherwise.
template <typename T, int NT>
__host__ __device__ __forceinline__ void ext1d_stage_window(T* win, const T* __restrict__ row, int n, int s0, int w, int mode, int tid)
{
    if (s0 >= 0 && s0 + w <= n) {
        for (int k = tid; k < w; k += NT) win[k] = row[s0 + k];
    } else {
        for (int k = tid; k < w; k += NT) {
            const int j = ext_index(s0 + k, n, mode);
            win[k] = j < 0 ? T(0) : row[j];
        }
    }
}

// cnt positions from the staged window (win[0] = xe[2 * i0 + 2 - F]) to a[0 .. cnt), d[0 .. cnt)
template <typename T, int NT>
__host__ __device__ __forceinline__ void ext1d_fwd_tile(const T* win, int cnt, int hlen, const Taps2<T>& taps, T* __restrict__ a, T* __restrict__ d, int tid)
{
    for (int i = tid; i < cnt; i += NT) {
        T lo, hi;
        ext1d_fwd_item<T, 0>(win + 2 * i, hlen, taps, lo, hi);
        a[i] = lo;
        d[i] = hi;
    }
}

// cntp pairs from the staged coefficient windows (wa[0] = a[p0]) to x[0 .. nx) (x = the sample 2 * p0 of the row, nx samples left)
template <typename T, int NT>
__host__ __device__ __forceinline__ void ext1d_inv_tile(const T* wa, const T* wd, int cntp, int nx, int hlen, const Taps2<T>& taps, T* __restrict__ x, int tid)
{
    for (int p = tid; p < cntp; p += NT) {
        T x0, x1;
        ext1d_inv_item<T, 0>(wa + p, wd + p, hlen, taps, x0, x1);
        x[2 * p] = x0;
        if (2 * p + 1 < nx) x[2 * p + 1] = x1;
    }
}

}  // namespace pdwt
