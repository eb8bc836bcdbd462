// dwt_ext.hpp -- the device side of the 2-D transform with signal-extension boundary modes (dwt_ext.hip; include/pdwt_hip.h "2-D DWT with
// boundary modes"): the index map of the modes and the stages of the two tile kernels as device functions -- stage a window in LDS,
// analysis along the rows / along the columns, stage the four child windows, synthesis along the columns / along the rows.  The
// kernels only place the buffers and call them in order.  (The packet and volume tile kernels, wpt2d.hip and dwt3d.hip, still carry
// their own copies of the pass loops: folding them onto this header is the follow-up of DESIGN.md 3.11.)
//
// One level along one axis, bank of even length F: N = (n + F - 1) / 2 coefficients per band,
//   a[i] = sum_k L[k] xe[2i + 1 - k]                    (xe = the line extended by the mode)
//   x[k] = sum_i a[i] IL[k + F - 2 - 2i] + d[i] IH[k + F - 2 - 2i]   over the i with a tap index in 0 .. F-1 (all inside 0 .. N-1)
#pragma once
#include "vol3d.hpp"

namespace pdwt {

enum ExtMode { EXT_ZERO = 0, EXT_CONSTANT = 1, EXT_SYMMETRIC = 2, EXT_REFLECT = 3, EXT_PERIODIC = 4, EXT_NUM_MODES = 5 };

// coefficients per band of a line of n samples
__host__ __device__ inline int ext_half(int n, int hlen) { return (n + hlen - 1) >> 1; }

// Index of the sample that xe[s] repeats, for ANY s (a tile may overhang the band by more than the line is long: full modulo, so
// the index is in bounds whatever the overhang); -1: the sample is 0 (mode zero).  n <= 2^30.
__host__ __device__ inline int ext_index(int s, int n, int mode)
{
    if ((unsigned)s < (unsigned)n) return s;
    switch (mode) {
    case EXT_ZERO: return -1;
    case EXT_CONSTANT: return s < 0 ? 0 : n - 1;
    case EXT_SYMMETRIC: {  // half-sample mirror, period 2n
        const int p = 2 * n;
        int m = s % p;
        if (m < 0) m += p;
        return m < n ? m : p - 1 - m;
    }
    case EXT_REFLECT: {  // whole-sample mirror, period 2n - 2; one sample: the constant
        if (n == 1) return 0;
        const int p = 2 * n - 2;
        int m = s % p;
        if (m < 0) m += p;
        return m < n ? m : p - m;
    }
    default: {  // EXT_PERIODIC
        int m = s % n;
        if (m < 0) m += n;
        return m;
    }
    }
}

// ---- forward ------------------------------------------------------------------------------------------------------------------
// Stage the RI x CI window with the origin (gy0, gx0) of the nr x nc image src into in[RI][CI].  A window that lies inside the image
// is copied with plain addressing (a workgroup-uniform branch); any other goes through the index map of the mode, computed once per
// window row and column into map[RI + CI].  Ends with a barrier.
template <typename T, int RI, int CI, int NT>
__device__ __forceinline__ void ext_stage_window(T* in, int* map, const T* __restrict__ src, int nr, int nc, int gy0, int gx0, int mode, int tid)
{
    if (gy0 >= 0 && gx0 >= 0 && gy0 + RI <= nr && gx0 + CI <= nc) {
        const T* __restrict__ p = src + (size_t)gy0 * nc + gx0;
        for (int e = tid; e < RI * CI; e += NT) {
            const int r = e / CI, cc = e - r * CI;  // (compile-time divisor)
            in[e] = p[(size_t)r * nc + cc];
        }
    } else {
        for (int e = tid; e < RI + CI; e += NT) map[e] = e < RI ? ext_index(gy0 + e, nr, mode) : ext_index(gx0 + (e - RI), nc, mode);
        __syncthreads();
        for (int e = tid; e < RI * CI; e += NT) {
            const int r = e / CI, cc = e - r * CI;
            const int sr = map[r], sc = map[RI + cc];
            in[e] = (sr < 0 || sc < 0) ? T(0) : src[(size_t)sr * nc + sc];
        }
    }
    __syncthreads();
}

// Analysis along the rows of in[RI][CI]: OX positions per row, low pass into rb[0][RI][OX], high pass into rb[1][RI][OX]; one FMA per
// tap in ascending order of the window (tap HL-1-j on sample j).  Ends with a barrier.
template <typename T, int HL, int RI, int CI, int OX, int NT>
__device__ __forceinline__ void ext_rows_analysis(const T* in, T* rb, const Taps2<T>& taps, int tid)
{
    for (int e = tid; e < RI * OX; e += NT) {
        const int r = e / OX, ox = e % OX;
        const T* p = in + r * CI + 2 * ox;
        const int z0 = opaque_zero();
        T sl = T(0), sh = T(0);
#pragma unroll
        for (int j = 0; j < HL; j++) {
            const T v = p[j];
            sl = fma_t<T>(v, taps.a[HL - 1 - j + z0], sl);
            sh = fma_t<T>(v, taps.b[HL - 1 - j + z0], sh);
        }
        rb[e] = sl;
        rb[RI * OX + e] = sh;
    }
    __syncthreads();
}

// Analysis along the columns of rb[2][RI][OX] for the OY x OX positions from (oy0, ox0), stored to the four hr x hc bands:
// row low -> A (column low), H (column high); row high -> V, D.  Positions past the bands are not stored.
template <typename T, int HL, int RI, int OX, int OY, int NT>
__device__ __forceinline__ void ext_cols_analysis_write(const T* rb, const Taps2<T>& taps, T* __restrict__ ba, T* __restrict__ bh, T* __restrict__ bv,
                                                        T* __restrict__ bd, int hr, int hc, int oy0, int ox0, int tid)
{
    for (int e = tid; e < OY * OX; e += NT) {
        const int oy = e / OX, ox = e % OX;
        if (oy0 + oy >= hr || ox0 + ox >= hc) continue;
        const size_t o = (size_t)(oy0 + oy) * hc + (ox0 + ox);
#pragma unroll
        for (int xb = 0; xb < 2; xb++) {
            const T* p = rb + xb * RI * OX + (2 * oy) * OX + ox;
            const int z0 = opaque_zero();
            T sl = T(0), sh = T(0);
#pragma unroll
            for (int j = 0; j < HL; j++) {
                const T v = p[j * OX];
                sl = fma_t<T>(v, taps.a[HL - 1 - j + z0], sl);
                sh = fma_t<T>(v, taps.b[HL - 1 - j + z0], sh);
            }
            (xb ? bv : ba)[o] = sl;
            (xb ? bd : bh)[o] = sh;
        }
    }
}

// ---- inverse ------------------------------------------------------------------------------------------------------------------
// Sample k of a line needs the coefficients (k >> 1) + m, m = 0 .. HL/2 - 1, with the taps HL-2-2m (k even) / HL-1-2m (k odd): no
// wrap, no extension, no mode.  A tile of G samples from an even g0 therefore needs the G/2 + HL/2 - 1 coefficients from g0 / 2.

// Stage the WR x WC windows with the origin (wy0, wx0) of the four hr x hc bands into in[4][WR][WC]; positions past a band (the
// overhang of the last tiles) are staged as 0.  Ends with a barrier.
template <typename T, int WR, int WC, int NT>
__device__ __forceinline__ void ext_stage_children(T* in, const T* const* q, int hr, int hc, int wy0, int wx0, int tid)
{
#pragma unroll
    for (int qd = 0; qd < 4; qd++) {
        const T* __restrict__ band = q[qd];
        for (int e = tid; e < WR * WC; e += NT) {
            const int r = e / WC, cc = e - r * WC;
            const int y = wy0 + r, x = wx0 + cc;
            in[qd * WR * WC + e] = (y < hr && x < hc) ? band[(size_t)y * hc + x] : T(0);
        }
    }
    __syncthreads();
}

// Synthesis along the columns: GY samples per column of the windows, (A, H) into cb[0][GY][WC], (V, D) into cb[1][GY][WC]; the two
// branch sums are added once.  Ends with a barrier.
template <typename T, int HL, int WR, int WC, int GY, int NT>
__device__ __forceinline__ void ext_cols_synthesis(const T* in, T* cb, const Taps2<T>& taps, int tid)
{
    constexpr int h2 = HL / 2;
    for (int e = tid; e < 2 * GY * WC; e += NT) {
        const int xb = e / (GY * WC), rem = e - xb * (GY * WC), gy = rem / WC, cc = rem - gy * WC;
        const bool odd = gy & 1;
        const T* pa = in + (2 * xb) * WR * WC + (gy >> 1) * WC + cc;
        const T* pd = pa + WR * WC;
        T sa = T(0), sd = T(0);
#pragma unroll
        for (int m = 0; m < h2; m++) {
            const T fl = odd ? taps.a[HL - 1 - 2 * m] : taps.a[HL - 2 - 2 * m];
            const T fh = odd ? taps.b[HL - 1 - 2 * m] : taps.b[HL - 2 - 2 * m];
            sa = fma_t<T>(pa[m * WC], fl, sa);
            sd = fma_t<T>(pd[m * WC], fh, sd);
        }
        cb[e] = sa + sd;
    }
    __syncthreads();
}

// Synthesis along the rows of cb[2][GY][WC] for the GY x GX samples from (g0y, g0x), stored to the nr x nc image; samples past it
// are not stored.
template <typename T, int HL, int WC, int GY, int GX, int NT>
__device__ __forceinline__ void ext_rows_synthesis_write(const T* cb, const Taps2<T>& taps, T* __restrict__ dst, int nr, int nc, int g0y, int g0x, int tid)
{
    constexpr int h2 = HL / 2;
    for (int e = tid; e < GY * GX; e += NT) {
        const int gy = e / GX, gx = e % GX;
        if (g0y + gy >= nr || g0x + gx >= nc) continue;
        const bool odd = gx & 1;
        const T* pa = cb + gy * WC + (gx >> 1);
        const T* pd = pa + GY * WC;
        T sa = T(0), sd = T(0);
#pragma unroll
        for (int m = 0; m < h2; m++) {
            const T fl = odd ? taps.a[HL - 1 - 2 * m] : taps.a[HL - 2 - 2 * m];
            const T fh = odd ? taps.b[HL - 1 - 2 * m] : taps.b[HL - 2 - 2 * m];
            sa = fma_t<T>(pa[m], fl, sa);
            sd = fma_t<T>(pd[m], fh, sd);
        }
        dst[(size_t)(g0y + gy) * nc + (g0x + gx)] = sa + sd;
    }
}

}  // namespace pdwt
