// tile_stages.hpp -- "one separable level of a tile through LDS", written once for the kernel families that compute it: the x-y kernels
// of the volume transform (dwt3d.hip), the packet tile kernels (wpt2d.hip), the boundary-mode tile kernels in 2-D and 3-D (dwt_ext.hip,
// dwt_ext3d.hip) and the synthesis of their level adjoint (dwt_ext_adj.hip, through it the x-y half of dwt_ext3d_adj.hip).
// Here: the tile shape and its LDS sizes, the two inner products (this file is the one place that states the summation order), the four
// LDS stages and the periodic staging of a window.  A kernel places its buffers, stages its window (periodic: below; by a boundary mode:
// dwt_ext.hpp) and calls the stages in order.
//
// The periodised and the boundary-mode synthesis are one rule: sample g of a line reads the coefficients (gp >> 1) + m, m = 0 .. HL/2 - 1,
// of its window with the taps HL-2-2m (gp even) / HL-1-2m (gp odd), where gp = g + SHIFT.  Boundary modes: SHIFT = 0, the window starts at
// coefficient g0 / 2.  Periodised: SHIFT = syn_shift(HL), the window starts HL/4 coefficients earlier (and is one coefficient longer).
//
// Not folded onto this header, on purpose: the z register-window kernels of the volume transforms and the z adjoint (their loops unroll
// completely and read the taps straight from the kernel argument; behind a function that takes the taps by reference the compiler loads
// all 2 * HL taps at the kernel's entry, and the float64 banks of 22 taps and more spill SGPRs -- they are written once as kernel
// templates on the job in z_stages.hpp, which keeps the taps in the kernel's own body); swt3d.hip (sublattice addressing, chunked
// tap reloads in fma_taps2, an inverse that stages one x band at a time); the whole-image-in-LDS kernels with run-time geometry
// (their 2-D stages are shared in image_stages.hpp, the 1-D ones in dwt_ext1d.hpp / wpt1d.hpp); the Haar and cost kernels of wpt2d.hip.
#pragma once
#include "vol3d.hpp"

namespace pdwt {

// ---- the tile -----------------------------------------------------------------------------------------------------------------
constexpr int kTileThreads = 256;
constexpr int TFX = 32, TFY = 16;  // forward tile (band positions)
constexpr int TIX = 64, TIY = 32;  // inverse tile (samples, even starts)

// the sample index shift of the periodised synthesis
constexpr int syn_shift(int hl) { return ((hl / 2) & 1) ? 0 : 1; }
// rows / columns of the forward window of a tile of o positions, and of the child windows of a tile of g samples
constexpr int tile_fwd_win(int o, int hl) { return 2 * o + hl - 2; }
constexpr int tile_inv_win(int g, int hl, bool periodised) { return g / 2 + hl / 2 - 1 + (periodised ? 1 : 0); }

// LDS of a forward tile: the window [RI][CI], the row pass [2][RI][TFX] and, for the boundary modes, the index map [RI + CI]
template <typename T, int HL>
constexpr size_t tile_fwd_lds(bool with_map)
{
    constexpr size_t RI = tile_fwd_win(TFY, HL), CI = tile_fwd_win(TFX, HL);
    return sizeof(T) * (RI * CI + 2 * RI * TFX) + (with_map ? sizeof(int) * (RI + CI) : 0);
}
// LDS of an inverse tile: the four child windows [4][WR][WC] and the column pass [2][TIY][WC]
template <typename T, int HL>
constexpr size_t tile_inv_lds(bool periodised)
{
    const size_t WR = tile_inv_win(TIY, HL, periodised), WC = tile_inv_win(TIX, HL, periodised);
    return sizeof(T) * (4 * WR * WC + 2 * (size_t)TIY * WC);
}

// ---- the two inner products ---------------------------------------------------------------------------------------------------
// Analysis of one position: (lo, hi) from p[j * STRIDE], j = 0 .. HL-1, tap HL-1-j on sample j, one FMA per tap in ascending j.  The tap
// index goes through opaque_zero(), so the tap loads stay inside the loop.
template <typename T, int HL, int STRIDE>
__device__ __forceinline__ void ana_dot(const T* p, const Taps2<T>& taps, T& lo, T& hi)
{
    const int z0 = opaque_zero();
    T sl = T(0), sh = T(0);
#pragma unroll
    for (int j = 0; j < HL; j++) {
        const T v = p[j * STRIDE];
        sl = fma_t<T>(v, taps.a[HL - 1 - j + z0], sl);
        sh = fma_t<T>(v, taps.b[HL - 1 - j + z0], sh);
    }
    lo = sl;
    hi = sh;
}

// Synthesis of the sample with the shifted index gp from pa[m * STRIDE] and pd[m * STRIDE], m = 0 .. HL/2 - 1: taps HL-1-2m if gp is odd,
// HL-2-2m if it is even; one FMA per tap in ascending m for each branch, the two branch sums added once.  The level adjoint calls it
// (adj_rows_synthesis_write).  The two synthesis stages below spell the same loop out instead: called as a function it compiles to
// other code (the operands arrive as parameters), and the periodised float64 kernels of 40 taps then measured 8 to 13 % slower per
// transform pair (volumes and packets); spelled out they compile to the code they had before they were shared.
template <typename T, int HL, int STRIDE>
__device__ __forceinline__ T syn_dot(const T* pa, const T* pd, int gp, const Taps2<T>& taps)
{
    const bool odd = gp & 1;
    T sa = T(0), sd = T(0);
#pragma unroll
    for (int m = 0; m < HL / 2; m++) {
        const T fl = odd ? taps.a[HL - 1 - 2 * m] : taps.a[HL - 2 - 2 * m];
        const T fh = odd ? taps.b[HL - 1 - 2 * m] : taps.b[HL - 2 - 2 * m];
        sa = fma_t<T>(pa[m * STRIDE], fl, sa);
        sd = fma_t<T>(pd[m * STRIDE], fh, sd);
    }
    return sa + sd;
}

// ---- periodic staging ---------------------------------------------------------------------------------------------------------
// The RI x CI window with the origin (gy0, gx0) of the nr x nc image src into in[RI][CI], every row and column index through wrap_ext
// (the periodisation of an odd line repeats its last sample).  Ends with a barrier.
template <typename T, int RI, int CI, int NT>
__device__ __forceinline__ void tile_stage_window_per(T* in, const T* __restrict__ src, int nr, int nc, int gy0, int gx0, int tid)
{
    for (int e = tid; e < RI * CI; e += NT) {
        const int r = e / CI, cc = e - r * CI;  // (compile-time divisor)
        in[e] = src[(size_t)wrap_ext(gy0 + r, nr) * nc + wrap_ext(gx0 + cc, nc)];
    }
    __syncthreads();
}

// The WR x WC windows with the origin (wy0, wx0) of the four hr x hc bands into in[4][WR][WC], every index through wrap_per; band(qd)
// is the base of band qd (how the four are found is the kernel's: a table of pointers, or a stride).  Ends with a barrier.
template <typename T, int WR, int WC, int NT, typename Band>
__device__ __forceinline__ void tile_stage_children_per(T* in, Band band, int hr, int hc, int wy0, int wx0, int tid)
{
    for (int e = tid; e < 4 * WR * WC; e += NT) {
        const int qd = e / (WR * WC), rem = e - qd * (WR * WC), r = rem / WC, cc = rem - r * WC;
        in[e] = band(qd)[(size_t)wrap_per(wy0 + r, hr) * hc + wrap_per(wx0 + cc, hc)];
    }
    __syncthreads();
}

// ---- forward stages -----------------------------------------------------------------------------------------------------------
// Analysis along the rows of in[RI][CI]: OX positions per row, low pass into rb[0][RI][OX], high pass into rb[1][RI][OX].  Ends with a
// barrier.
template <typename T, int HL, int RI, int CI, int OX, int NT>
__device__ __forceinline__ void tile_rows_analysis(const T* in, T* rb, const Taps2<T>& taps, int tid)
{
    for (int e = tid; e < RI * OX; e += NT) {
        const int r = e / OX, ox = e % OX;
        T sl, sh;
        ana_dot<T, HL, 1>(in + r * CI + 2 * ox, taps, sl, sh);
        rb[e] = sl;
        rb[RI * OX + e] = sh;
    }
    __syncthreads();
}

// Analysis along the columns of rb[2][RI][OX] for the OY x OX positions from (oy0, ox0), stored to the four hr x hc bands:
// row low -> A (column low), H (column high); row high -> V, D.  Positions past the bands are not stored.
template <typename T, int HL, int RI, int OX, int OY, int NT>
__device__ __forceinline__ void tile_cols_analysis_write(const T* rb, const Taps2<T>& taps, T* __restrict__ ba, T* __restrict__ bh, T* __restrict__ bv,
                                                         T* __restrict__ bd, int hr, int hc, int oy0, int ox0, int tid)
{
    for (int e = tid; e < OY * OX; e += NT) {
        const int oy = e / OX, ox = e % OX;
        if (oy0 + oy >= hr || ox0 + ox >= hc) continue;
        const size_t o = (size_t)(oy0 + oy) * hc + (ox0 + ox);
#pragma unroll
        for (int xb = 0; xb < 2; xb++) {
            T sl, sh;
            ana_dot<T, HL, OX>(rb + xb * RI * OX + (2 * oy) * OX + ox, taps, sl, sh);
            (xb ? bv : ba)[o] = sl;
            (xb ? bd : bh)[o] = sh;
        }
    }
}

// ---- inverse stages -----------------------------------------------------------------------------------------------------------
// Synthesis along the columns of the windows in[4][WR][WC]: GY samples per column, (A, H) into cb[0][GY][WC], (V, D) into cb[1][GY][WC].
// Ends with a barrier.
template <typename T, int HL, int SHIFT, int WR, int WC, int GY, int NT>
__device__ __forceinline__ void tile_cols_synthesis(const T* in, T* cb, const Taps2<T>& taps, int tid)
{
    for (int e = tid; e < 2 * GY * WC; e += NT) {
        const int xb = e / (GY * WC), rem = e - xb * (GY * WC), gy = rem / WC, cc = rem - gy * WC;
        const int gp = gy + SHIFT;
        const T* pa = in + (2 * xb) * WR * WC + (gp >> 1) * WC + cc;
        const T* pd = pa + WR * WC;
        const bool odd = gp & 1;
        T sa = T(0), sd = T(0);
#pragma unroll
        for (int m = 0; m < HL / 2; m++) {  // (syn_dot, spelled out: see there)
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
template <typename T, int HL, int SHIFT, int WC, int GY, int GX, int NT>
__device__ __forceinline__ void tile_rows_synthesis_write(const T* cb, const Taps2<T>& taps, T* __restrict__ dst, int nr, int nc, int g0y, int g0x, int tid)
{
    for (int e = tid; e < GY * GX; e += NT) {
        const int gy = e / GX, gx = e % GX;
        if (g0y + gy >= nr || g0x + gx >= nc) continue;
        const int gp = gx + SHIFT;
        const T* pa = cb + gy * WC + (gp >> 1);
        const T* pd = pa + GY * WC;
        const bool odd = gp & 1;
        T sa = T(0), sd = T(0);
#pragma unroll
        for (int m = 0; m < HL / 2; m++) {  // (syn_dot, spelled out: see there)
            const T fl = odd ? taps.a[HL - 1 - 2 * m] : taps.a[HL - 2 - 2 * m];
            const T fh = odd ? taps.b[HL - 1 - 2 * m] : taps.b[HL - 2 - 2 * m];
            sa = fma_t<T>(pa[m], fl, sa);
            sd = fma_t<T>(pd[m], fh, sd);
        }
        dst[(size_t)(g0y + gy) * nc + (g0x + gx)] = sa + sd;
    }
}

}  // namespace pdwt
