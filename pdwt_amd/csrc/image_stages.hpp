// image_stages.hpp -- "every level of a whole image inside the LDS of one workgroup", written once for the two kernel families that
// compute it: the batched 2-D transform with boundary modes (dwt_ext2db.hpp) and the batched 2-D wavelet packets (wpt2db.hpp).  What
// tile_stages.hpp is for the tile kernels, with run-time geometry: the copy-in, the rule that says where the taps live, the two inner
// products (this file is the one place that states their summation order), the index-table fill and the four LDS stages.  A family
// keeps its pipelines (which buffer holds what, and where the barriers stand), its structs and its plan.
//
// One departure, measured: the FORWARD boundary kernels keep their two analysis loops and their table fill written out in
// dwt_ext2db.hpp and share only the item and the copy-in.  Through the analysis stages below (a compile-time "-1 means zero" flag, the
// line pair found by a compare, the band stores in a functor) k_ext2db_fwd_fused<float, 8> ran 2 to 4 % slower (64 x 128^2 db4 L3:
// 30.4 us against 29.3 / 29.3 of the build before, 29.6 against 28.7 / 28.6 in mode zero), with 13 instructions FEWER; written out, all
// 40 forward kernels are instruction-identical to that build.  The analysis stages therefore serve the periodised line only.
//
// Every stage is __host__ __device__, takes the thread count as a template argument and the thread index as an argument and contains no
// barrier: the kernels run them with NT = 512 between LDS-only barriers, a host program with NT = 1, tid = 0 under a sanitizer.
//
// The two kinds of line.  A level maps a line of n samples to `half` positions per band; position i reads the window of F samples from
// 2 i + S0 of the line continued past its ends, and the inverse makes the samples 2 q - shift, 2 q - shift + 1 from F / 2 coefficients.
//   extended (boundary modes)  S0 = 2 - F; a sample past the ends is the one the mode names, or 0 (mode zero: its table entry is
//                              -1); half = (n + F - 1) / 2 covers every window that meets the line, so the inverse needs
//                              nothing past the ends of a band: shift 0, pair p reads the coefficients p .. p + F/2 - 1 (PER = false)
//   periodised (packets)       S0 = -(F/2 - 1); the line made even is periodic; half = div2(n); the inverse wraps: shift = wp1_shift(F),
//                              pair q reads (q - F/4 + m) mod half through an index table near the ends (PER = true)
// A window that lies inside the line -- all but about F / 2 at each end -- is read with plain addressing, any other through a table of
// source indices that img_fill_map wrote (one table serves every line of a pass: they have one length).
//
// Line pairs.  The column passes work on pairs of planes: pair kb = 2 k + xb is column band xb of image / node k.  In the synthesis
// stages NP is the number of pairs where the kernel knows it at compile time (the boundary kernels hold ONE image: the pair of a work
// item is then found without an integer division), 0 where it is the argument (the packets: 2 * 4^l).
//
// Values: rows first with the intermediate rounded to T, then columns, one FMA per tap in ascending order of the window; inverse columns
// first, the (A, H) and (V, D) sums added once each, then rows, the low and high sums added once.
#pragma once
#include "wpt1d.hpp"

namespace pdwt {

// a state table of the synthesis stages holds one byte per parent; only the parents whose byte is this are computed (WPB_SYNTH)
constexpr unsigned char kImgSynth = 2;

// n contiguous elements src -> dst (LDS): 16-byte loads and stores where src is aligned (dst is: every LDS region starts on 16 bytes),
// the tail element-wise
template <typename T, int NT>
__host__ __device__ __forceinline__ void img_copy_in(T* dst, const T* __restrict__ src, int n, int tid)
{
    using V = typename Ext1dVec<T>::v16;
    constexpr int NV = Ext1dVec<T>::NV;
    int done = 0;
    if ((reinterpret_cast<uintptr_t>(src) & 15) == 0 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
        const int nch = n / NV;
        for (int e = tid; e < nch; e += NT) reinterpret_cast<V*>(dst)[e] = reinterpret_cast<const V*>(src)[e];
        done = nch * NV;
    }
    for (int e = done + tid; e < n; e += NT) dst[e] = src[e];
}

// map[k] = index(k), k = 0 .. cnt - 1
template <int NT, typename Index>
__host__ __device__ __forceinline__ void img_fill_map(int* map, int cnt, Index index, int tid)
{
    for (int k = tid; k < cnt; k += NT) map[k] = index(k);
}

// The 2 * HL taps stay in scalar registers for the short banks only (up to 10 taps float32, 4 float64): next to the shapes, the band
// pointers and the loop state of a whole pyramid a longer bank spills scalar registers.  Longer banks index the taps through the opaque
// zero of dwt_ext.hpp, so that they are loaded where they are used.
template <typename T, int HL>
constexpr bool img_opaque_taps() { return HL * sizeof(T) > 40; }

// (lo, hi) of one position: `get(j)` is sample j of its window, j = 0 .. HL-1 (tap HL-1-j on sample j)
template <typename T, int HL, typename Get>
__host__ __device__ __forceinline__ void img_fwd_item(Get get, const Taps2<T>& taps, T& lo, T& hi)
{
    const int z0 = img_opaque_taps<T, HL>() ? ext1d_zero() : 0;
    T sl = T(0), sh = T(0);
    auto step = [&](int j) {
        const T v = get(j);
        sl = ext1d_fma(v, taps.a[HL - 1 - j + z0], sl);
        sh = ext1d_fma(v, taps.b[HL - 1 - j + z0], sh);
    };
    if constexpr (img_opaque_taps<T, HL>()) {
#pragma unroll 8
        for (int j = 0; j < HL; j++) step(j);
    } else {
#pragma unroll
        for (int j = 0; j < HL; j++) step(j);
    }
    lo = sl, hi = sh;
}

// (x0, x1) = one pair of samples of a line from the coefficients ga(m), gd(m), m = 0 .. HL/2 - 1: the sums of ext1d_inv_item
template <typename T, int HL, typename GetA, typename GetD>
__host__ __device__ __forceinline__ void img_inv_item(GetA ga, GetD gd, const Taps2<T>& taps, T& x0, T& x1)
{
    const int z0 = img_opaque_taps<T, HL>() ? ext1d_zero() : 0;
    T ae = T(0), ao = T(0), de = T(0), dd = T(0);
    auto step = [&](int m) {
        const T ca = ga(m), cd = gd(m);
        ae = ext1d_fma(ca, taps.a[HL - 2 - 2 * m + z0], ae);
        ao = ext1d_fma(ca, taps.a[HL - 1 - 2 * m + z0], ao);
        de = ext1d_fma(cd, taps.b[HL - 2 - 2 * m + z0], de);
        dd = ext1d_fma(cd, taps.b[HL - 1 - 2 * m + z0], dd);
    };
    if constexpr (img_opaque_taps<T, HL>()) {
#pragma unroll 4
        for (int m = 0; m < HL / 2; m++) step(m);
    } else {
#pragma unroll
        for (int m = 0; m < HL / 2; m++) step(m);
    }
    x0 = ae + de, x1 = ao + dd;
}

// ---- forward (the periodised line; the boundary kernels: dwt_ext2db.hpp) --------------------------------------------------------------
// Analysis along the `rows` rows of in[rows][nc] (of all nodes of a depth: they are one run of rows): hc positions per row, low pass into
// rb[0][rows][hc], high pass into rb[1][rows][hc].  cmap[k] = the source of sample k + S0, k = 0 .. 2 hc + HL - 3.
template <typename T, int HL, int S0, int NT>
__host__ __device__ __forceinline__ void img_rows_analysis(const T* in, T* rb, const int* cmap, int rows, int nc, int hc, const Taps2<T>& taps, int tid)
{
    const int total = rows * hc;
    for (int e = tid; e < total; e += NT) {
        const int r = e / hc, ox = e - r * hc;
        const T* row = in + r * nc;
        const int s0 = 2 * ox + S0;
        T lo, hi;
        if (s0 >= 0 && s0 + HL <= nc) {
            const T* p = row + s0;
            img_fwd_item<T, HL>([&](int j) { return p[j]; }, taps, lo, hi);
        } else {
            const int* m = cmap + 2 * ox;
            img_fwd_item<T, HL>([&](int j) { return row[m[j]]; }, taps, lo, hi);
        }
        rb[e] = lo;
        rb[total + e] = hi;
    }
}

// Analysis along the columns of rb[2][np / 2][nr][hc] for the hr x hc positions of every line pair: row low -> A (column low), H (column
// high); row high -> V, D.  Work items are numbered across (pair, row, position), position fastest: store(kb, o, lo, hi) receives the
// column low and high pass of position o of pair kb and puts them where the family keeps them.
template <typename T, int HL, int S0, int NT, typename Store>
__host__ __device__ __forceinline__ void img_cols_analysis(const T* rb, const int* rmap, int np, int nr, int hr, int hc, const Taps2<T>& taps, int tid, Store store)
{
    const int per = hr * hc, plane = (np >> 1) * nr * hc, total = np * per;
    for (int e = tid; e < total; e += NT) {
        const int kb = e / per, o = e - kb * per, k = kb >> 1, xb = kb & 1;
        const int oy = o / hc, ox = o - oy * hc;
        const T* col = rb + xb * plane + k * nr * hc + ox;
        const int s0 = 2 * oy + S0;
        T lo, hi;
        if (s0 >= 0 && s0 + HL <= nr) {
            const T* p = col + s0 * hc;
            img_fwd_item<T, HL>([&](int j) { return p[j * hc]; }, taps, lo, hi);
        } else {
            const int* m = rmap + 2 * oy;
            img_fwd_item<T, HL>([&](int j) { return col[m[j] * hc]; }, taps, lo, hi);
        }
        store(kb, o, lo, hi);
    }
}

// ---- inverse ----------------------------------------------------------------------------------------------------------------------------
// the sample pairs of a line of n samples (the work items of a synthesis stage along it) and the index shift of the first
template <bool PER>
__host__ __device__ __forceinline__ int img_pairs(int n, int F) { return PER ? wp1_pairs(n, F) : (n + 1) >> 1; }

// Synthesis along the columns: line pair kb is a + kb * ps (column low) and d + kb * ps (column high), both [hr][hc], and fills
// cb[kb][nr][hc]; two rows per work item.  st (PER only; NULL: every parent): the parent kb >> 1 is computed where its byte is
// kImgSynth.  rmap (PER only): (k - HL/4) mod hr, k = 0 .. pairs + HL/2 - 2.  Extended: the last coefficient read is row
// ((nr - 1) >> 1) + HL / 2 - 1 = hr - 1.
template <typename T, int HL, bool PER, int NP, int NT>
__host__ __device__ __forceinline__ void img_cols_synthesis(const T* a, const T* d, int ps, T* cb, const int* rmap, const unsigned char* st, int np, int nr, int hr, int hc,
                                                            const Taps2<T>& taps, int tid)
{
    constexpr int h2 = HL / 2, cq = PER ? HL / 4 : 0;
    const int sh = PER ? wp1_shift(HL) : 0;
    if constexpr (NP != 0) np = NP;
    const int per = img_pairs<PER>(nr, HL) * hc, total = np * per;
    for (int e = tid; e < total; e += NT) {
        const int kb = NP == 1 ? 0 : e / per, rem = e - kb * per;
        if (PER && st && st[kb >> 1] != kImgSynth) continue;
        const int q = rem / hc, cc = rem - q * hc;
        const T *la = a + kb * ps + cc, *ld = d + kb * ps + cc;
        T x0, x1;
        if (!PER || (q - cq >= 0 && q - cq + h2 <= hr)) {
            const T *pa = la + (q - cq) * hc, *pd = ld + (q - cq) * hc;
            img_inv_item<T, HL>([&](int m) { return pa[m * hc]; }, [&](int m) { return pd[m * hc]; }, taps, x0, x1);
        } else {
            const int* mp = rmap + q;
            img_inv_item<T, HL>([&](int m) { return la[mp[m] * hc]; }, [&](int m) { return ld[mp[m] * hc]; }, taps, x0, x1);
        }
        const int g0 = 2 * q - sh;
        T* o = cb + kb * nr * hc + cc;
        if (!PER || g0 >= 0) o[g0 * hc] = x0;
        if (g0 + 1 < nr) o[(g0 + 1) * hc] = x1;
    }
}

// Synthesis along the rows of cb[nodes][2][nr][hc] ((A, H) | (V, D) of every node) into out + k * nr * nc, node k (LDS or HBM); two
// samples per work item.  NP: the nodes, as above (1: one image).  st, cmap: as above, along the rows.
template <typename T, int HL, bool PER, int NP, int NT>
__host__ __device__ __forceinline__ void img_rows_synthesis(const T* cb, T* out, const int* cmap, const unsigned char* st, int nodes, int nr, int nc, int hc,
                                                            const Taps2<T>& taps, int tid)
{
    constexpr int h2 = HL / 2, cq = PER ? HL / 4 : 0;
    const int sh = PER ? wp1_shift(HL) : 0;
    if constexpr (NP != 0) nodes = NP;
    const int Q = img_pairs<PER>(nc, HL), per = nr * Q, total = nodes * per;
    for (int e = tid; e < total; e += NT) {
        const int k = NP == 1 ? 0 : e / per, rem = e - k * per;
        if (PER && st && st[k] != kImgSynth) continue;
        const int r = rem / Q, q = rem - r * Q;
        const T* a = cb + ((2 * k) * nr + r) * hc;
        const T* d = a + nr * hc;
        T x0, x1;
        if (!PER || (q - cq >= 0 && q - cq + h2 <= hc)) {
            const T *pa = a + (q - cq), *pd = d + (q - cq);
            img_inv_item<T, HL>([&](int m) { return pa[m]; }, [&](int m) { return pd[m]; }, taps, x0, x1);
        } else {
            const int* mp = cmap + q;
            img_inv_item<T, HL>([&](int m) { return a[mp[m]]; }, [&](int m) { return d[mp[m]]; }, taps, x0, x1);
        }
        const int g0 = 2 * q - sh;
        T* o = out + (size_t)k * nr * nc + (size_t)r * nc;
        if (!PER || g0 >= 0) o[g0] = x0;
        if (g0 + 1 < nc) o[g0 + 1] = x1;
    }
}

}  // namespace pdwt
