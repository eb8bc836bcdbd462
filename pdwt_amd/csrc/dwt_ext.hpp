// dwt_ext.hpp -- the device side of the 2-D transform with signal-extension boundary modes (dwt_ext.hip; include/pdwt_hip.h "2-D DWT with
// boundary modes"): what belongs to the modes -- their index map and the two staging functions that read through it or zero-fill, the
// window of a forward tile and the four child windows of an inverse tile.  The passes that follow the staging (analysis along the rows /
// columns, synthesis along the columns / rows) are the stages of tile_stages.hpp, shared with the periodised tile kernels; the
// synthesis runs with SHIFT = 0.  The kernels only place the buffers and call the stages in order.
//
// One level along one axis, bank of even length F: N = (n + F - 1) / 2 coefficients per band,
//   a[i] = sum_k L[k] xe[2i + 1 - k]                    (xe = the line extended by the mode)
//   x[k] = sum_i a[i] IL[k + F - 2 - 2i] + d[i] IH[k + F - 2 - 2i]   over the i with a tap index in 0 .. F-1 (all inside 0 .. N-1)
#pragma once
#include "tile_stages.hpp"

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

// ---- inverse ------------------------------------------------------------------------------------------------------------------
// Sample k of a line needs the coefficients (k >> 1) + m, m = 0 .. HL/2 - 1, with the taps HL-2-2m (k even) / HL-1-2m (k odd): no
// wrap, no extension, no mode.  A tile of G samples from an even g0 therefore needs the G/2 + HL/2 - 1 coefficients from g0 / 2.

// Stage the WR x WC windows with the origin (wy0, wx0) of the four hr x hc bands into in[4][WR][WC]; positions outside a band are
// staged as 0: past it in the overhang of the last tiles, and before it where the origin is negative (the level adjoint stages the
// bands padded with HL/2 - 1 zeros on every side).  Ends with a barrier.
template <typename T, int WR, int WC, int NT>
__device__ __forceinline__ void ext_stage_children(T* in, const T* const* q, int hr, int hc, int wy0, int wx0, int tid)
{
#pragma unroll
    for (int qd = 0; qd < 4; qd++) {
        const T* __restrict__ band = q[qd];
        for (int e = tid; e < WR * WC; e += NT) {
            const int r = e / WC, cc = e - r * WC;
            const int y = wy0 + r, x = wx0 + cc;
            in[qd * WR * WC + e] = ((unsigned)y < (unsigned)hr && (unsigned)x < (unsigned)hc) ? band[(size_t)y * hc + x] : T(0);
        }
    }
    __syncthreads();
}

}  // namespace pdwt
