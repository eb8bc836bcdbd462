// wpt1d.hpp -- the stages of the batched 1-D wavelet packet transform (wpt1d.hip; include/pdwt_hip.h "Batched 1-D wavelet packets"): the
// LDS line layouts, the halo fills, one analysis / synthesis depth step over a pack of rows, and the window staging of the per-level
// kernels.  As in dwt_ext1d.hpp every stage takes the thread count as a template argument and the thread index as an argument and
// contains no barrier, so the same code runs on the device (NT = 256, the kernels place the barriers between the stages) and on a CPU
// with NT = 1, tid = 0 (a host program can include this header and run whole pipelines under a sanitizer).
//
// One step of a node of n samples, bank of even length F (the periodised level of Wavelets; oracle ana_lines / syn_lines):
//   N = div2(n),  c = F/2 - 1:   a[i] = sum_j xe[2i - c + j] L[F-1-j],  xe = the node made even by repeating its last sample, periodic
//   h2 = F/2, c' = h2/2, shift = 1 - (h2 & 1):  the pair x[2q - shift], x[2q - shift + 1] = sum_m a[(q - c' + m) mod N] IL[F-2-2m | F-1-2m]
//                                               + the same sum over d with IH, q = 0 .. (n - 1 + shift) / 2; the two sums added once
// One FMA per tap in ascending order of the window sample / of the coefficient: wp1_fwd_item / wp1_inv_item have the arithmetic of
// ext1d_fwd_item / ext1d_inv_item (the window of the periodised level only starts elsewhere), so they ARE those functions.  Haar
// (F = 2) is the reference's 1-D Haar level instead: s * (x0 +- x1) with s = 0.70710678118654746 as a double, the product evaluated
// in double and rounded once, x1 clamped to the last sample of an odd node (what the periodic halo of one cell holds).
//
// LDS lines.  A row at depth l is 2^l node segments, each with its own periodic halo, since the neighbours of a node's ends are its own
// other end and not the next node:
//   forward  [c cells | n_l samples | F/2 cells], segment stride wp1_fseg = n_l + F - 1 rounded up to even: the window of position i
//            starts at the EVEN cell 2i of the segment, so a work item reads it as F/2 aligned pairs (ds_read_b64 / b128)
//   inverse  [c' cells | n_l coefficients | h2 - 1 - c' + shift cells], segment stride wp1_iseg = n_l + h2; the window of pair q starts at cell q
// The halos are written by a full modulo (F - 2 can exceed n_l), so the item loops have no index map and no branch.
#pragma once
#include <vector>

#include "dwt_ext1d.hpp"

namespace pdwt {

constexpr int kWp1Threads = 256;
constexpr int kWp1MaxLev = 12;   // WPT1D_MAX_LEVELS: 4096 nodes per row enter grid and table sizes
constexpr int kWp1Tile = 1024;   // per-level kernels: child positions (forward) / sample pairs (inverse) per workgroup

// node states of the inverse (one byte per node, node i of depth l at (2^l - 1) + i)
enum Wp1State : unsigned char { WP1_SKIP = 0, WP1_LOAD = 1, WP1_SYNTH = 2 };

template <typename T>
struct Wp1Levels {
    T* p[kWp1MaxLev + 1];   // p[l], l = 1 .. L: the allocation of depth l, (Nr, 2^l, n[l]) row-major; p[0] unused
    int n[kWp1MaxLev + 1];  // n[0] = Nc, n[l] = div2(n[l - 1])
    int L;
};

__host__ __device__ inline int wp1_div2(int n) { return (n + 1) >> 1; }
__host__ __device__ inline int wp1_fseg(int n, int F) { return (n + F - 1 + 1) & ~1; }
__host__ __device__ inline int wp1_iseg(int n, int F) { return n + F / 2; }
__host__ __device__ inline int wp1_shift(int F) { return ((F / 2) & 1) ? 0 : 1; }
__host__ __device__ inline int wp1_pairs(int n, int F) { return (n - 1 + wp1_shift(F)) / 2 + 1; }  // work items of one parent of n samples

// wrap_ext / wrap_per of common.hpp for host and device
__host__ __device__ inline int wp1_wrap_ext(int s, int n)
{
    const int np = n + (n & 1);
    if ((unsigned)s >= (unsigned)np) {
        s %= np;
        if (s < 0) s += np;
    }
    return (s == n) ? n - 1 : s;
}
__host__ __device__ inline int wp1_wrap_per(int s, int n)
{
    if ((unsigned)s >= (unsigned)n) {
        s %= n;
        if (s < 0) s += n;
    }
    return s;
}

// ---- host: what the packet families (wpt1d.hip, wpt2db.hip) ask of a bank, a size and a basis -------------------------------------------
inline bool packet_bank_ok(int hlen) { return hlen >= 2 && hlen <= PDWT_MAX_FILTER_WIDTH && !(hlen & 1); }
inline int packet_ilog2(int v)
{
    int l = 0;
    while (v > 1) v >>= 1, l++;
    return l;
}

// The node-state table of a basis given as n (depth, index) pairs of a tree of `levels` depths with ARITY (2 or 4) children per node:
// one byte per node, node i of depth l at (ARITY^l - 1) / (ARITY - 1) + i; LOAD for a basis node, SYNTH for every node above one, SKIP
// below.  PDWT_EINVAL unless every root-to-leaf path meets exactly one node of the basis.
template <int ARITY>
inline int packet_state_table(int levels, int max_levels, const int* depth, const int* idx, int n, unsigned char* out)
{
    static_assert(ARITY == 2 || ARITY == 4, "binary trees of rows, quad-trees of images");
    constexpr int B = ARITY == 4 ? 2 : 1;  // nodes of depth l: 1 << (B * l)
    auto nodes = [](int l) { return 1 << (B * l); };
    auto off = [&](int l) { return (nodes(l) - 1) / (ARITY - 1); };
    if (levels < 1 || levels > max_levels || !depth || !idx || !out || n < 1) return PDWT_EINVAL;
    const int total = off(levels + 1);
    std::vector<unsigned char> leaf((size_t)nodes(levels), 0);
    for (int k = 0; k < total; k++) out[k] = WP1_SKIP;
    for (int k = 0; k < n; k++) {
        const int d = depth[k], i = idx[k];
        if (d < 0 || d > levels || i < 0 || i >= nodes(d)) return PDWT_EINVAL;
        const int span = nodes(levels - d);
        for (int j = i * span; j < (i + 1) * span; j++) {
            if (leaf[j]) return PDWT_EINVAL;  // two nodes on one root-to-leaf path
            leaf[j] = 1;
        }
        out[off(d) + i] = WP1_LOAD;
    }
    for (size_t j = 0; j < leaf.size(); j++)
        if (!leaf[j]) return PDWT_EINVAL;  // a path that meets no node
    for (int l = levels - 1; l >= 0; l--)
        for (int i = 0; i < nodes(l); i++) {
            const unsigned char* kid = out + off(l + 1) + ARITY * i;
            for (int q = 0; q < ARITY; q++)
                if (kid[q] != WP1_SKIP) out[off(l) + i] = WP1_SYNTH;
        }
    return PDWT_OK;
}

// ---- the only places where taps meet samples ------------------------------------------------------------------------------------
#define WP1_ONE_SQRT2 0.70710678118654746

// (a, d) of one position from its window p[0 .. F-1] (p aligned to a pair); HL = 0: the length is the run-time hlen
template <typename T, int HL>
__host__ __device__ __forceinline__ void wp1_fwd_item(const T* p, int hlen, const Taps2<T>& taps, T& lo, T& hi)
{
    ext1d_fwd_item<T, HL>(p, hlen, taps, lo, hi);
}
template <typename T>
__host__ __device__ __forceinline__ void wp1_haar_fwd_item(const T* p, T& lo, T& hi)
{
    using V2 = typename Ext1dVec<T>::v2;
    const V2 v = *reinterpret_cast<const V2*>(p);
    lo = (T)(WP1_ONE_SQRT2 * (double)(v[0] + v[1]));
    hi = (T)(WP1_ONE_SQRT2 * (double)(v[0] - v[1]));
}
// the pair (x[2q - shift], x[2q - shift + 1]) from the coefficients pa[0 .. F/2 - 1], pd[0 .. F/2 - 1]
template <typename T, int HL>
__host__ __device__ __forceinline__ void wp1_inv_item(const T* pa, const T* pd, int hlen, const Taps2<T>& taps, T& x0, T& x1)
{
    ext1d_inv_item<T, HL>(pa, pd, hlen, taps, x0, x1);
}
template <typename T>
__host__ __device__ __forceinline__ void wp1_haar_inv_item(const T* pa, const T* pd, T& x0, T& x1)
{
    const T a = pa[0], d = pd[0];
    x0 = (T)(WP1_ONE_SQRT2 * (double)(a + d));
    x1 = (T)(WP1_ONE_SQRT2 * (double)(a - d));
}
// the bank decides (compile time in the fused kernels, a uniform branch in the per-level ones)
template <typename T, int HL>
__host__ __device__ __forceinline__ void wp1_fwd_pos(const T* p, int hlen, const Taps2<T>& taps, T& lo, T& hi)
{
    if ((HL ? HL : hlen) == 2) wp1_haar_fwd_item<T>(p, lo, hi);
    else wp1_fwd_item<T, HL>(p, hlen, taps, lo, hi);
}
template <typename T, int HL>
__host__ __device__ __forceinline__ void wp1_inv_pos(const T* pa, const T* pd, int hlen, const Taps2<T>& taps, T& x0, T& x1)
{
    if ((HL ? HL : hlen) == 2) wp1_haar_inv_item<T>(pa, pd, x0, x1);
    else wp1_inv_item<T, HL>(pa, pd, hlen, taps, x0, x1);
}

// ---- packs of whole rows: forward -------------------------------------------------------------------------------------------------
// Copy `rows` consecutive rows of n samples (contiguous at src) to the depth-0 lines dst + r * ls + c: 16-byte loads when every row starts
// aligned, else element-wise; the LDS stores are scalar (the samples of a line start c cells in, which need not be a 16-byte offset).
template <typename T, int NT>
__host__ __device__ __forceinline__ void wp1_stage_rows(T* dst, int ls, int c, const T* __restrict__ src, int rows, int n, int tid)
{
    using V = typename Ext1dVec<T>::v16;
    constexpr int NV = Ext1dVec<T>::NV;
    if ((n % NV) == 0 && (reinterpret_cast<uintptr_t>(src) & 15) == 0) {
        const int nch = n / NV, total = rows * nch;
        for (int e = tid; e < total; e += NT) {
            const int r = rows == 1 ? 0 : e / nch, ch = e - r * nch;
            const V v = reinterpret_cast<const V*>(src)[e];
            T* o = dst + (size_t)r * ls + c + ch * NV;
#pragma unroll
            for (int k = 0; k < NV; k++) o[k] = v[k];
        }
    } else {
        const int total = rows * n;
        for (int e = tid; e < total; e += NT) {
            const int r = rows == 1 ? 0 : e / n, col = e - r * n;
            dst[(size_t)r * ls + c + col] = src[e];
        }
    }
}

// Write the periodic halo of every node segment of the lines of one depth: xe[-c .. -1] and xe[n .. n + F/2 - 1] (F - 1 cells per node).
// Reads samples, writes halo cells only: needs a barrier before and after, none inside.
template <typename T, int NT>
__host__ __device__ __forceinline__ void wp1_fwd_halo(T* lines, int ls, int ns, int rows, int nodes, int n, int F, int tid)
{
    const int c = F / 2 - 1, hc = F - 1, per_row = nodes * hc, total = rows * per_row;
    for (int e = tid; e < total; e += NT) {
        const int r = e / per_row, rem = e - r * per_row, k = rem / hc, h = rem - k * hc;
        const int s = h < c ? h - c : n + (h - c);
        T* seg = lines + (size_t)r * ls + (size_t)k * ns + c;
        seg[s] = seg[wp1_wrap_ext(s, n)];
    }
}

// One analysis step of a pack: the lines of depth l at cur (`nodes` segments of stride cns per line of stride cls, n samples each) -> both
// children of every node, straight from registers to the rows of the depth-(l+1) allocation at g (the pack's first row; a row is
// 2 * nodes * N elements) and, nxt != NULL, into the lines at nxt (segment stride nns, line stride nls).  Work items are numbered across
// (row, parent, position): lanes are consecutive within a node, so the two store streams are coalesced.
template <typename T, int HL, int NT>
__host__ __device__ __forceinline__ void wp1_fwd_level(const T* cur, int cls, int cns, T* nxt, int nls, int nns, int rows, int nodes, int n, int hlen,
                                                       const Taps2<T>& taps, T* __restrict__ g, int tid)
{
    const int F = HL ? HL : hlen, c = F / 2 - 1, N = wp1_div2(n), per_row = nodes * N, total = rows * per_row;
    for (int e = tid; e < total; e += NT) {
        const int r = e / per_row, rem = e - r * per_row, k = rem / N, i = rem - k * N;
        T lo, hi;
        wp1_fwd_pos<T, HL>(cur + (size_t)r * cls + (size_t)k * cns + 2 * i, hlen, taps, lo, hi);
        T* go = g + (size_t)r * (2 * (size_t)per_row) + (size_t)(2 * k) * N + i;
        go[0] = lo;
        go[N] = hi;
        if (nxt) {
            T* no = nxt + (size_t)r * nls + (size_t)(2 * k) * nns + c + i;
            no[0] = lo;
            no[nns] = hi;
        }
    }
}

// ---- packs of whole rows: inverse -------------------------------------------------------------------------------------------------
// Stage the LOAD nodes of one depth from the rows of its allocation at g (the pack's first row) into the inverse lines.
template <typename T, int NT>
__host__ __device__ __forceinline__ void wp1_inv_stage(T* lines, int ls, int is, const T* __restrict__ g, const unsigned char* __restrict__ st, int rows, int nodes,
                                                       int n, int F, int tid)
{
    const int cl = F / 4, per_row = nodes * n, total = rows * per_row;
    for (int e = tid; e < total; e += NT) {
        const int r = e / per_row, rem = e - r * per_row, k = rem / n, i = rem - k * n;
        if (st[k] != WP1_LOAD) continue;
        lines[(size_t)r * ls + (size_t)k * is + cl + i] = g[(size_t)r * per_row + rem];
    }
}

// The periodic halo of every node segment that holds coefficients (LOAD or SYNTH): F/2 - 1 + shift cells per node.
template <typename T, int NT>
__host__ __device__ __forceinline__ void wp1_inv_halo(T* lines, int ls, int is, const unsigned char* __restrict__ st, int rows, int nodes, int n, int F, int tid)
{
    const int cl = F / 4, hc = F / 2 - 1 + wp1_shift(F);  // (Haar: none; the kernels do not call this stage then)
    if (hc <= 0) return;
    const int per_row = nodes * hc, total = rows * per_row;
    for (int e = tid; e < total; e += NT) {
        const int r = e / per_row, rem = e - r * per_row, k = rem / hc, h = rem - k * hc;
        if (st[k] == WP1_SKIP) continue;
        const int s = h < cl ? h - cl : n + (h - cl);
        T* seg = lines + (size_t)r * ls + (size_t)k * is + cl;
        seg[s] = seg[wp1_wrap_per(s, n)];
    }
}

// One synthesis step of a pack: every SYNTH parent of depth l (`nodes` of them per row, n samples) from its two children in the lines at
// ch (segment stride cis, line stride cls) -> its segment in the lines at par (segment stride pis, line stride pls), or, par == NULL
// (depth 0, one node), the rows at g (the pack's first row, n elements per row).  Two samples per work item.
template <typename T, int HL, int NT>
__host__ __device__ __forceinline__ void wp1_inv_level(const T* ch, int cls, int cis, T* par, int pls, int pis, const unsigned char* __restrict__ st, int rows,
                                                       int nodes, int n, int hlen, const Taps2<T>& taps, T* __restrict__ g, int tid)
{
    const int F = HL ? HL : hlen, sh = wp1_shift(F), Q = wp1_pairs(n, F), per_row = nodes * Q, total = rows * per_row;
    for (int e = tid; e < total; e += NT) {
        const int r = e / per_row, rem = e - r * per_row, k = rem / Q, q = rem - k * Q;
        if (st[k] != WP1_SYNTH) continue;
        const T* pa = ch + (size_t)r * cls + (size_t)(2 * k) * cis + q;
        T x0, x1;
        wp1_inv_pos<T, HL>(pa, pa + cis, hlen, taps, x0, x1);
        const int g0 = 2 * q - sh;
        T* o = par ? par + (size_t)r * pls + (size_t)k * pis + F / 4 : g + (size_t)r * n;
        if (g0 >= 0) o[g0] = x0;
        if (g0 + 1 < n) o[g0 + 1] = x1;
    }
}

// ---- tiles of one node (the per-level kernels) ----------------------------------------------------------------------------------------
// Stage xe[s0 .. s0 + w) of a node into win: plain addressing when the window lies inside the node (a workgroup-uniform branch)
template <typename T, int NT>
__host__ __device__ __forceinline__ void wp1_stage_window(T* win, const T* __restrict__ node, int n, int s0, int w, int tid)
{
    if (s0 >= 0 && s0 + w <= n) {
        for (int k = tid; k < w; k += NT) win[k] = node[s0 + k];
    } else {
        for (int k = tid; k < w; k += NT) win[k] = node[wp1_wrap_ext(s0 + k, n)];
    }
}
// cnt positions from the staged window (win[0] = xe[2 * i0 - c]) to a[0 .. cnt), d[0 .. cnt)
template <typename T, int NT>
__host__ __device__ __forceinline__ void wp1_fwd_tile(const T* win, int cnt, int hlen, const Taps2<T>& taps, T* __restrict__ a, T* __restrict__ d, int tid)
{
    for (int i = tid; i < cnt; i += NT) {
        T lo, hi;
        wp1_fwd_pos<T, 0>(win + 2 * i, hlen, taps, lo, hi);
        a[i] = lo;
        d[i] = hi;
    }
}
// Stage the children's coefficients (q0 - c' + k) mod N, k = 0 .. w - 1, into wa / wd
template <typename T, int NT>
__host__ __device__ __forceinline__ void wp1_stage_children(T* wa, T* wd, const T* __restrict__ a, const T* __restrict__ d, int N, int j0, int w, int tid)
{
    if (j0 >= 0 && j0 + w <= N) {
        for (int k = tid; k < w; k += NT) {
            wa[k] = a[j0 + k];
            wd[k] = d[j0 + k];
        }
    } else {
        for (int k = tid; k < w; k += NT) {
            const int j = wp1_wrap_per(j0 + k, N);
            wa[k] = a[j];
            wd[k] = d[j];
        }
    }
}
// cntq pairs from the staged windows to the parent x (n samples), the first pair being q0
template <typename T, int NT>
__host__ __device__ __forceinline__ void wp1_inv_tile(const T* wa, const T* wd, int q0, int cntq, int n, int hlen, const Taps2<T>& taps, T* __restrict__ x, int tid)
{
    const int sh = wp1_shift(hlen);
    for (int q = tid; q < cntq; q += NT) {
        T x0, x1;
        wp1_inv_pos<T, 0>(wa + q, wd + q, hlen, taps, x0, x1);
        const int g0 = 2 * (q0 + q) - sh;
        if (g0 >= 0) x[g0] = x0;
        if (g0 + 1 < n) x[g0 + 1] = x1;
    }
}

// ---- what one workgroup does ------------------------------------------------------------------------------------------------------------
// The kernels of wpt1d.hip are these functions with NT = 256 and an LDS-only barrier as `sync`; a host program runs them with NT = 1,
// tid = 0 and a `sync` that does nothing, on a heap buffer of the size the launch would request.
//
// LDS placement of the fused forms: `region` elements; the lines of even depths start at base, those of odd depths END at base + region,
// so two adjacent depths never overlap when region >= R * (the largest sum of two adjacent lines).

// All depths of the pack of R rows number `block`: stage once, then per depth compute, store, and (unless it is the last) fill the halos
// of the other buffer.  The last depth never touches LDS.
template <typename T, int HL, int NT, typename Sync>
__host__ __device__ __forceinline__ void wp1_fwd_fused_block(T* base, int region, const T* __restrict__ src, const Wp1Levels<T>& lv, int Nr, int R, unsigned block,
                                                             const Taps2<T>& taps, int tid, Sync sync)
{
    constexpr int c = HL / 2 - 1;
    const size_t row0 = (size_t)block * R;
    const int rows = (size_t)Nr - row0 < (size_t)R ? (int)((size_t)Nr - row0) : R;
    int n = lv.n[0], nodes = 1, cns = wp1_fseg(n, HL), cls = cns;
    T* cur = base;
    wp1_stage_rows<T, NT>(cur, cls, c, src + row0 * (size_t)n, rows, n, tid);
    sync();
    wp1_fwd_halo<T, NT>(cur, cls, cns, rows, nodes, n, HL, tid);
    sync();
    for (int l = 0; l < lv.L; l++) {
        const int N = lv.n[l + 1], nns = wp1_fseg(N, HL), nls = 2 * nodes * nns;
        const bool last = l + 1 == lv.L;
        T* nxt = last ? nullptr : (((l + 1) & 1) ? base + region - (size_t)R * nls : base);
        wp1_fwd_level<T, HL, NT>(cur, cls, cns, nxt, nls, nns, rows, nodes, n, HL, taps, lv.p[l + 1] + row0 * (2 * (size_t)nodes * N), tid);
        if (last) break;
        sync();
        wp1_fwd_halo<T, NT>(nxt, nls, nns, rows, 2 * nodes, N, HL, tid);
        sync();
        cur = nxt, cls = nls, cns = nns, n = N, nodes *= 2;
    }
}

// From depth L to 0 under the state table: stage the LOAD nodes of depth L, then per depth synthesise the SYNTH parents from the line
// below, stage the LOAD nodes of the parents' depth next to them, fill the halos.  Depth 0 goes to the rows of dst.
template <typename T, int HL, int NT, typename Sync>
__host__ __device__ __forceinline__ void wp1_inv_fused_block(T* base, int region, T* __restrict__ dst, const Wp1Levels<T>& lv, const unsigned char* __restrict__ state,
                                                             int Nr, int R, unsigned block, const Taps2<T>& taps, int tid, Sync sync)
{
    constexpr bool has_halo = HL / 2 - 1 + (((HL / 2) & 1) ? 0 : 1) > 0;  // (Haar reads no neighbour)
    const size_t row0 = (size_t)block * R;
    const int rows = (size_t)Nr - row0 < (size_t)R ? (int)((size_t)Nr - row0) : R;
    const int L = lv.L;
    int nodes = 1 << L, N = lv.n[L], cis = wp1_iseg(N, HL), cls = nodes * cis;
    T* ch = (L & 1) ? base + region - (size_t)R * cls : base;
    wp1_inv_stage<T, NT>(ch, cls, cis, lv.p[L] + row0 * ((size_t)nodes * N), state + (nodes - 1), rows, nodes, N, HL, tid);
    sync();
    if constexpr (has_halo) {
        wp1_inv_halo<T, NT>(ch, cls, cis, state + (nodes - 1), rows, nodes, N, HL, tid);
        sync();
    }
    for (int l = L - 1; l >= 0; l--) {
        nodes >>= 1;
        const int n = lv.n[l], pis = wp1_iseg(n, HL), pls = nodes * pis;
        const unsigned char* st = state + (nodes - 1);
        if (l == 0) {
            wp1_inv_level<T, HL, NT>(ch, cls, cis, (T*)nullptr, 0, 0, st, rows, 1, n, HL, taps, dst + row0 * (size_t)n, tid);
            break;
        }
        T* par = (l & 1) ? base + region - (size_t)R * pls : base;
        wp1_inv_level<T, HL, NT>(ch, cls, cis, par, pls, pis, st, rows, nodes, n, HL, taps, dst, tid);  // (dst is not used while par is given)
        wp1_inv_stage<T, NT>(par, pls, pis, lv.p[l] + row0 * ((size_t)nodes * n), st, rows, nodes, n, HL, tid);
        sync();
        if constexpr (has_halo) {
            wp1_inv_halo<T, NT>(par, pls, pis, st, rows, nodes, n, HL, tid);
            sync();
        }
        ch = par, cls = pls, cis = pis;
    }
}

// One tile of one parent of one row, forward: win holds 2 * kWp1Tile + hlen - 2 elements
template <typename T, int NT, typename Sync>
__host__ __device__ __forceinline__ void wp1_fwd_level_block(T* win, const T* __restrict__ src, T* __restrict__ dst, int n, int N, int tiles, int hlen, unsigned block,
                                                             const Taps2<T>& taps, int tid, Sync sync)
{
    const unsigned seg = block / (unsigned)tiles, tile = block - seg * (unsigned)tiles;  // seg = row * nodes + parent
    const int i0 = (int)tile * kWp1Tile, cnt = N - i0 < kWp1Tile ? N - i0 : kWp1Tile;
    wp1_stage_window<T, NT>(win, src + (size_t)seg * n, n, 2 * i0 - (hlen / 2 - 1), 2 * cnt + hlen - 2, tid);
    sync();
    T* a = dst + (size_t)seg * 2 * N + i0;
    wp1_fwd_tile<T, NT>(win, cnt, hlen, taps, a, a + N, tid);
}

// One tile of one parent of one row, inverse: smem holds two windows of kWp1Tile + PDWT_MAX_FILTER_WIDTH / 2 elements
template <typename T, int NT, typename Sync>
__host__ __device__ __forceinline__ void wp1_inv_level_block(T* smem, T* __restrict__ par, const T* __restrict__ child, int n, int N, int nodes,
                                                             const int* __restrict__ list, int count, const unsigned char* __restrict__ st, int tiles, int hlen,
                                                             unsigned block, const Taps2<T>& taps, int tid, Sync sync)
{
    T* wa = smem;
    T* wd = wa + kWp1Tile + PDWT_MAX_FILTER_WIDTH / 2;
    const unsigned job = block / (unsigned)tiles, tile = block - job * (unsigned)tiles;
    const unsigned row = job / (unsigned)count, li = job - row * (unsigned)count;
    const int k = list ? list[li] : (int)li;
    if (st && st[k] != WP1_SYNTH) return;  // (uniform over the workgroup)
    const int Q = wp1_pairs(n, hlen), q0 = (int)tile * kWp1Tile, cntq = Q - q0 < kWp1Tile ? Q - q0 : kWp1Tile;
    const T* a = child + ((size_t)row * nodes + k) * 2 * N;
    wp1_stage_children<T, NT>(wa, wd, a, a + N, N, q0 - hlen / 4, cntq + hlen / 2 - 1, tid);
    sync();
    wp1_inv_tile<T, NT>(wa, wd, q0, cntq, n, hlen, taps, par + ((size_t)row * nodes + k) * n, tid);
}

}  // namespace pdwt
