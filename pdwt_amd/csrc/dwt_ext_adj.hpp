// dwt_ext_adj.hpp -- the stages of the ADJOINT of the forward transform with signal-extension boundary modes (dwt_ext_adj.hip;
// include/pdwt_hip.h "Adjoints of the boundary-mode DWT").  With an extension the adjoint of the analysis is not the synthesis: the
// extension matrix folds back and the taps are the analysis taps.
//
// One level along one line of n samples, bank of even length F, N = (n + F - 1) / 2, cotangents abar, dbar of N entries:
//   u[s]    = sum_i abar[i] L[2i + 1 - s] + dbar[i] H[2i + 1 - s]     s = 2 - F .. 2N - 1, over the i with a tap index in 0 .. F-1
//   xbar[k] = sum of u[s] over the s with ext_index(s, n, mode) == k, in ascending s (s = k included)
// u is a synthesis onto the EXTENDED line.  With the reversed taps L'[j] = L[F-1-j] and the cell e = s + F - 2 of the extended line
//   u[e] = sum_i' a'[i'] L'[e + F - 2 - 2i'],   a'[i'] = abar[i' - (F/2 - 1)]  (0 outside 0 .. N-1)
// which is the inverse formula of dwt_ext.hpp on a coefficient line padded with F/2 - 1 zeros on either side: the pair functions of the
// inverse (ext1d_inv_item; tile_cols_synthesis of tile_stages.hpp with SHIFT 0) are reused as they are, on E = 2N + F - 2 =
// 2 (N + F/2 - 1) cells.
// The fold is a gather in a fixed order (no floating-point atomics): the pre-images come from ext_index itself, never from a count.
//
// The 1-D stages take the thread count as a template argument and the thread index as an argument and contain no barrier, like those
// of dwt_ext1d.hpp, so a host program runs them with NT = 1 under a sanitizer.  The 2-D stages follow dwt_ext.hpp.
#pragma once
#include "dwt_ext1d.hpp"

namespace pdwt {

// cells of the extended line
__host__ __device__ inline int adj_ext_len(int n, int F) { return 2 * ext_half(n, F) + F - 2; }
// halo cells of a line: F - 2 to the left, 2N - n to the right
__host__ __device__ inline int adj_halo_len(int n, int F) { return adj_ext_len(n, F) - n; }
// the extended index s of halo cell h (0 .. halo_len - 1)
__host__ __device__ inline int adj_halo_s(int h, int n, int F) { return h < F - 2 ? h - (F - 2) : n + (h - (F - 2)); }

// the reversed analysis taps (the rest of the table is 0)
template <typename T>
inline Taps2<T> taps_adj(const typename FiltersOf<T>::type* f)
{
    Taps2<T> t;
    for (int i = 0; i < PDWT_MAX_FILTER_WIDTH; i++) {
        const bool in = i < f->hlen;
        t.a[i] = in ? f->L[f->hlen - 1 - i] : T(0);
        t.b[i] = in ? f->H[f->hlen - 1 - i] : T(0);
    }
    return t;
}

// ---- 1-D: packs of whole rows (the fused kernel) -------------------------------------------------------------------------------
// Zero the cells c0 .. c0 + cnt - 1 of every line (the padding of a coefficient line).
template <typename T, int NT>
__host__ __device__ __forceinline__ void ext1d_zero_cells(T* lines, int stride, int c0, int cnt, int rows, int tid)
{
    for (int e = tid; e < rows * cnt; e += NT) {
        const int r = e / cnt, k = e - r * cnt;
        lines[(size_t)r * stride + c0 + k] = T(0);
    }
}

// Synthesis of a pack onto the extended lines: a and d point at the PADDED coefficient lines (a[0] = abar[-(F/2 - 1)] = 0), ext at cell
// 0 of the extended lines (s = 2 - F); N + F/2 - 1 pairs per row.
template <typename T, int HL, int NT>
__host__ __device__ __forceinline__ void ext1d_adj_level(const T* a, int as, const T* d, int ds, T* ext, int es, int rows, int N, int hlen, const Taps2<T>& taps, int tid)
{
    const int F = HL ? HL : hlen, P = N + F / 2 - 1, total = rows * P;
    for (int e = tid; e < total; e += NT) {
        const int r = rows == 1 ? 0 : e / P, p = e - r * P;
        T x0, x1;
        ext1d_inv_item<T, HL>(a + (size_t)r * as + p, d + (size_t)r * ds + p, hlen, taps, x0, x1);
        T* o = ext + (size_t)r * es + 2 * p;
        o[0] = x0;
        o[1] = x1;
    }
}

// ext_index of the halo cells of a line of n samples (H entries; -1: dropped, mode zero), once per level: the fold looks the targets up
// instead of taking a modulo per pair of cells.
template <int NT>
__host__ __device__ __forceinline__ void ext1d_halo_map(int* hmap, int n, int F, int mode, int tid)
{
    const int H = adj_halo_len(n, F);
    for (int h = tid; h < H; h += NT) hmap[h] = ext_index(adj_halo_s(h, n, F), n, mode);
}

// The gather counterpart of ext1d_fill_halo: every sample of a line adds the halo cells that repeat it, x[k] = sum of u[s] over the s
// with ext_index(s) == k in ascending s -- the left halo cells, the sample itself, the right halo cells.  x: the samples (row stride
// xs); hl: the F - 2 left halo cells, hr: the 2N - n right ones (row stride hs; in an LDS line hl = x - (F - 2), hr = x + n); hmap: the
// table of ext1d_halo_map.  One work item per halo cell: the FIRST halo cell of a target sample gathers for it, the others leave, so a
// sample is written by one item and read by that item alone.  Samples that no halo cell repeats are not touched.  Needs a barrier
// before (the line and hmap are complete) and after.
template <typename T, int NT>
__host__ __device__ __forceinline__ void ext1d_fold_halo(T* x, int xs, const T* hl, const T* hr, int hs, const int* hmap, int rows, int n, int F, int tid)
{
    const int H = adj_halo_len(n, F), total = rows * H;
    for (int e = tid; e < total; e += NT) {
        const int r = e / H, h = e - r * H;
        const int k = hmap[h];
        if (k < 0) continue;  // mode zero: the halo is dropped
        bool first = true;
        for (int g = 0; g < h; g++) first = first && hmap[g] != k;
        if (!first) continue;
        const T* pl = hl + (size_t)r * hs;
        const T* pr = hr + (size_t)r * hs;
        T* px = x + (size_t)r * xs + k;
        T acc = T(0);
        for (int g = h; g < F - 2; g++)
            if (hmap[g] == k) acc += pl[g];
        acc += *px;
        for (int g = h > F - 2 ? h : F - 2; g < H; g++)
            if (hmap[g] == k) acc += pr[g - (F - 2)];
        *px = acc;
    }
}

// Copy `rows` lines of n samples (stride, from cell off) to consecutive rows at dst.
template <typename T, int NT>
__host__ __device__ __forceinline__ void ext1d_store_rows(T* __restrict__ dst, const T* lines, int stride, int off, int rows, int n, int tid)
{
    const int total = rows * n;
    for (int e = tid; e < total; e += NT) {
        const int r = rows == 1 ? 0 : e / n, c = e - r * n;
        dst[e] = lines[(size_t)r * stride + off + c];
    }
}

// ---- 1-D: tiles of one row (the per-level kernels) ---------------------------------------------------------------------------------
// Stage the padded coefficients a'[p0 .. p0 + w) of a row (N coefficients at row) into win; 0 outside the row.
template <typename T, int NT>
__host__ __device__ __forceinline__ void ext1d_adj_stage(T* win, const T* __restrict__ row, int N, int F, int p0, int w, int tid)
{
    for (int k = tid; k < w; k += NT) {
        const int i = p0 + k - (F / 2 - 1);
        win[k] = (unsigned)i < (unsigned)N ? row[i] : T(0);
    }
}

// cntp pairs from the staged windows (wa[0] = a'[p0]): the cells 2 p0 .. of the extended line go to the row x (the real samples) or to
// the row's halo cells (left | right, as ext1d_fold_halo reads them; NULL: dropped).
template <typename T, int NT>
__host__ __device__ __forceinline__ void ext1d_adj_tile(const T* wa, const T* wd, int p0, int cntp, int n, int hlen, const Taps2<T>& taps, T* __restrict__ x,
                                                        T* __restrict__ halo, int tid)
{
    for (int p = tid; p < cntp; p += NT) {
        T v[2];
        ext1d_inv_item<T, 0>(wa + p, wd + p, hlen, taps, v[0], v[1]);
        for (int j = 0; j < 2; j++) {
            const int e = 2 * (p0 + p) + j, s = e - (hlen - 2);
            if ((unsigned)s < (unsigned)n) x[s] = v[j];
            else if (halo) halo[s < 0 ? e : e - n] = v[j];
        }
    }
}

// ---- 2-D (tiles of the extended grid) -------------------------------------------------------------------------------------------------
// The frame of an image: the cells of the extended Er x Ec grid outside the nr x nc samples, packed as the F - 2 top rows and the
// bottom rows (Ec cells each), then per sample row its left and right cells.  (ey, ex): a cell of the extended grid that is in the frame.
__host__ __device__ inline size_t adj_frame_elems(int nr, int nc, int F) { return (size_t)adj_ext_len(nr, F) * adj_ext_len(nc, F) - (size_t)nr * nc; }
__host__ __device__ inline size_t adj_frame_index(int ey, int ex, int nr, int nc, int Er, int Ec, int F)
{
    if (ey < F - 2) return (size_t)ey * Ec + ex;
    if (ey >= F - 2 + nr) return (size_t)(ey - nr) * Ec + ex;
    return (size_t)(Er - nr) * Ec + (size_t)(ey - (F - 2)) * (Ec - nc) + (ex < F - 2 ? ex : ex - nc);
}

// tile_rows_synthesis_write (SHIFT 0) onto the extended grid: the GY x GX cells from (g0y, g0x) of the Er x Ec grid; a cell of the
// sample range is stored to the image, any other to the frame (NULL: dropped, mode zero).
template <typename T, int HL, int WC, int GY, int GX, int NT>
__device__ __forceinline__ void adj_rows_synthesis_write(const T* cb, const Taps2<T>& taps, T* __restrict__ dst, T* __restrict__ frame, int nr, int nc, int Er,
                                                         int Ec, int g0y, int g0x, int tid)
{
    for (int e = tid; e < GY * GX; e += NT) {
        const int gy = e / GX, gx = e % GX;
        const int ey = g0y + gy, ex = g0x + gx;
        if (ey >= Er || ex >= Ec) continue;
        const int sy = ey - (HL - 2), sx = ex - (HL - 2);
        const bool real = (unsigned)sy < (unsigned)nr && (unsigned)sx < (unsigned)nc;
        if (!real && !frame) continue;
        const T* pa = cb + gy * WC + (gx >> 1);
        const T u = syn_dot<T, HL, 1>(pa, pa + GY * WC, gx, taps);
        if (real) dst[(size_t)sy * nc + sx] = u;
        else frame[adj_frame_index(ey, ex, nr, nc, Er, Ec, HL)] = u;
    }
}

// The 2-D fold of one sample (y, x): xbar = sum over sy in Pre(y), ascending, of (sum over sx in Pre(x), ascending, of U[sy][sx]).
// rmap / cmap: ext_index of the halo cells of the two axes (Hr and Hc entries).  U of the sample itself is read from the image, every
// other pre-image lies in the frame.  Returns false (and leaves the image alone) when the sample has no pre-image besides itself.
template <typename T>
__host__ __device__ __forceinline__ bool adj_fold_sample(T* __restrict__ img, const T* __restrict__ frame, const int* rmap, const int* cmap, int y, int x, int nr,
                                                         int nc, int F)
{
    const int Er = adj_ext_len(nr, F), Ec = adj_ext_len(nc, F), Hr = Er - nr, Hc = Ec - nc, F2 = F - 2;
    bool any = false;
    for (int h = 0; h < Hr && !any; h++) any = rmap[h] == y;
    for (int h = 0; h < Hc && !any; h++) any = cmap[h] == x;
    if (!any) return false;
    T* own = img + (size_t)y * nc + x;
    auto row_sum = [&](int ey, bool self) {  // the row ey of the extended grid
        T s = T(0);
        for (int h = 0; h < F2; h++)
            if (cmap[h] == x) s += frame[adj_frame_index(ey, h, nr, nc, Er, Ec, F)];
        s += self ? *own : frame[adj_frame_index(ey, F2 + x, nr, nc, Er, Ec, F)];
        for (int h = F2; h < Hc; h++)
            if (cmap[h] == x) s += frame[adj_frame_index(ey, nc + h, nr, nc, Er, Ec, F)];
        return s;
    };
    T acc = T(0);
    for (int h = 0; h < F2; h++)
        if (rmap[h] == y) acc += row_sum(h, false);
    acc += row_sum(F2 + y, true);
    for (int h = F2; h < Hr; h++)
        if (rmap[h] == y) acc += row_sum(nr + h, false);
    *own = acc;
    return true;
}

// ---- what dwt_ext_adj.hip shares with the 3-D adjoint (dwt_ext3d_adj.hip) --------------------------------------------------------------
// what a 2-D level adjoint on B images refuses
bool adj2_level_ok(long long B, int nr, int nc, int hlen);
// one level of the 2-D adjoint of the forward transform on B images: (a, h, v, d) cotangent stacks (B, hr, hc) -> dst (B, nr, nc); tmp: B
// frames of adj_frame_elems (may be NULL in mode zero).  Defined and instantiated for float and double in dwt_ext_adj.hip.
template <typename T>
int adj2_forward_level(T* dst, const T* a, const T* h, const T* v, const T* d, int B, int nr, int nc, int mode, const typename FiltersOf<T>::type* f, T* tmp);

// the bank whose forward transform in mode zero is the adjoint of the inverse: L' = reversed IL, H' = reversed IH
template <typename T>
inline bool adj_inverse_bank(typename FiltersOf<T>::type& g, const typename FiltersOf<T>::type* f)
{
    if (!f || f->hlen < 2 || f->hlen > PDWT_MAX_FILTER_WIDTH || (f->hlen & 1)) return false;
    g = *f;
    for (int i = 0; i < f->hlen; i++) g.L[i] = f->IL[f->hlen - 1 - i], g.H[i] = f->IH[f->hlen - 1 - i];
    return true;
}

}  // namespace pdwt
