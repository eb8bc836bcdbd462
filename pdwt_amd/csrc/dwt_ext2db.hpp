// dwt_ext2db.hpp -- the pipelines of the fused kernels of the batched 2-D transform with signal-extension boundary modes (dwt_ext2db.hip;
// include/pdwt_hip.h "Batched 2-D DWT with boundary modes"): the whole pyramid of ONE image in the LDS of one workgroup.  The copy-in,
// the two items and the synthesis stages are those of image_stages.hpp, shared with the packets (wpt2db.hpp); the synthesis runs on the
// extended line: no shift, centre or table, one line pair per call.  The two analysis loops and the table fill are written out here:
// through the shared analysis stages the float32 kernels of up to 10 taps measured 2 to 4 % slower (image_stages.hpp).  Every stage takes the thread count as a
// template argument and the thread index as an argument and contains no barrier; the two pipelines (ext2db_fwd_image /
// ext2db_inv_image) take the barrier as a functor.  The kernels pass the LDS-only barrier and
// NT = 512; a host program passes a no-op and NT = 1, tid = 0 and runs whole pipelines on the CPU under a sanitizer.
//
// Values.  The operation sequence is that of the tile kernels of dwt_ext.hpp, so the results are the same bits: forward rows first with
// the intermediate rounded to T, then columns, one FMA per tap in ascending order of the window, the extension materialised as values
// (a sample of mode `zero` is a 0 that goes through its FMA); inverse columns first, the (A, H) and (V, D) sums added once each, then
// rows, the low and high sums added once.
//
// Forward LDS: [img: nr x nc | rb: 2 x nr x hc | cmap | rmap].  The extension is read through two source-index tables written once per
// level: cmap[k] = ext_index(k + 2 - F, nc) for the 2 hc + F - 2 window cells of a row, rmap likewise for a column (-1: the sample is 0).
// Windows that lie inside the line (all but about F / 2 at each end) skip the table.  The approximation of a level is written over the
// image (dead after the row pass) and is the next level's input.
// Inverse LDS: [ra: one band | rd: one band | cb: 2 x nr x hc].  ra holds the approximation, rd receives H; column synthesis of the pair
// fills cb[0]; then V and D are staged over the two (at most two child bands are resident at a time) and fill cb[1]; row synthesis
// writes the nr x nc result into ra, the next level's approximation, or, at level 1, to the image in HBM.
#pragma once
#include "image_stages.hpp"

namespace pdwt {

constexpr int kExt2dbThreads = 512;
constexpr int kExt2dbMaxLev = 32;

template <typename T>
struct Ext2dbBands {
    T* p[3 * kExt2dbMaxLev + 1];                       // the band stacks [A_L, H1, V1, D1, ..., H_L, V_L, D_L], each B x nr[l] x nc[l]
    int nr[kExt2dbMaxLev + 1], nc[kExt2dbMaxLev + 1];  // [0] the image, [l] the bands of level l
    int nlev;
};

// map[k] = the sample that xe[k + 2 - F] repeats, k = 0 .. 2 * half + F - 3: the windows of the `half` positions of a line of n samples
template <int NT>
__host__ __device__ __forceinline__ void ext2db_fill_map(int* map, int n, int half, int F, int mode, int tid)
{
    const int cnt = 2 * half + F - 2;
    for (int k = tid; k < cnt; k += NT) map[k] = ext_index(k + 2 - F, n, mode);
}

// Analysis along the rows of in[nr][nc]: hc positions per row, low pass into rb[0][nr][hc], high pass into rb[1][nr][hc].
template <typename T, int HL, int NT>
__host__ __device__ __forceinline__ void ext2db_rows_analysis(const T* in, T* rb, const int* cmap, int nr, int nc, int hc, const Taps2<T>& taps, int tid)
{
    const int total = nr * hc;
    for (int e = tid; e < total; e += NT) {
        const int r = e / hc, ox = e - r * hc;
        const T* row = in + r * nc;
        const int s0 = 2 * ox + 2 - HL;
        T lo, hi;
        if (s0 >= 0 && 2 * ox + 1 < nc) {
            const T* p = row + s0;
            img_fwd_item<T, HL>([&](int j) { return p[j]; }, taps, lo, hi);
        } else {
            const int* m = cmap + 2 * ox;
            img_fwd_item<T, HL>([&](int j) { const int s = m[j]; return s < 0 ? T(0) : row[s]; }, taps, lo, hi);
        }
        rb[e] = lo;
        rb[total + e] = hi;
    }
}

// Analysis along the columns of rb[2][nr][hc] for the hr x hc positions of the four bands: row low -> A (column low), H (column high);
// row high -> V, D.  H, V, D go to the image's slices of the band stacks; A to ga when given (the last level), else to the LDS
// buffer a_lds[hr][hc].  One work item per (row band, position).
template <typename T, int HL, int NT>
__host__ __device__ __forceinline__ void ext2db_cols_analysis(const T* rb, const int* rmap, T* a_lds, T* __restrict__ ga, T* __restrict__ gh, T* __restrict__ gv,
                                                              T* __restrict__ gd, int nr, int hr, int hc, const Taps2<T>& taps, int tid)
{
    const int per = hr * hc, total = 2 * per, plane = nr * hc;
    for (int e = tid; e < total; e += NT) {
        const int xb = e >= per ? 1 : 0, o = e - xb * per;
        const int oy = o / hc, ox = o - oy * hc;
        const T* col = rb + xb * plane + ox;
        const int s0 = 2 * oy + 2 - HL;
        T lo, hi;
        if (s0 >= 0 && 2 * oy + 1 < nr) {
            const T* p = col + s0 * hc;
            img_fwd_item<T, HL>([&](int j) { return p[j * hc]; }, taps, lo, hi);
        } else {
            const int* m = rmap + 2 * oy;
            img_fwd_item<T, HL>([&](int j) { const int s = m[j]; return s < 0 ? T(0) : col[s * hc]; }, taps, lo, hi);
        }
        if (xb) {
            gv[o] = lo;
            gd[o] = hi;
        } else {
            gh[o] = hi;
            if (ga) ga[o] = lo;
            else a_lds[o] = lo;
        }
    }
}

// All levels of image `ib` of the batch.  img: Nr * Nc elements, rb: 2 * Nr * nc[1], cmap: 2 * nc[1] + HL - 2 ints, rmap: 2 * nr[1] + HL - 2.
template <typename T, int HL, int NT, typename Bar>
__host__ __device__ __forceinline__ void ext2db_fwd_image(T* img, T* rb, int* cmap, int* rmap, const T* __restrict__ src, const Ext2dbBands<T>& b, size_t ib, int mode,
                                                          const Taps2<T>& taps, int tid, Bar bar)
{
    const int L = b.nlev;
    img_copy_in<T, NT>(img, src + ib * ((size_t)b.nr[0] * b.nc[0]), b.nr[0] * b.nc[0], tid);
    ext2db_fill_map<NT>(cmap, b.nc[0], b.nc[1], HL, mode, tid);
    bar();
    for (int lev = 1; lev <= L; lev++) {
        const int nr = b.nr[lev - 1], nc = b.nc[lev - 1], hr = b.nr[lev], hc = b.nc[lev];
        ext2db_fill_map<NT>(rmap, nr, hr, HL, mode, tid);  // (read by the column pass, after the barrier; the last one was read before the previous)
        ext2db_rows_analysis<T, HL, NT>(img, rb, cmap, nr, nc, hc, taps, tid);
        bar();
        const size_t o = ib * ((size_t)hr * hc);
        T* const* d = b.p + 3 * (lev - 1) + 1;
        const bool last = lev == L;
        ext2db_cols_analysis<T, HL, NT>(rb, rmap, img, last ? b.p[0] + o : nullptr, d[0] + o, d[1] + o, d[2] + o, nr, hr, hc, taps, tid);
        if (last) break;
        ext2db_fill_map<NT>(cmap, hc, b.nc[lev + 1], HL, mode, tid);  // (the row pass that read cmap is behind the barrier)
        bar();
    }
}

// ---- inverse --------------------------------------------------------------------------------------------------------------------------
// All levels of image `ib`, coarse to fine.  ra, rd: one band of the largest level each (nr[1] * nc[1] elements, rounded up to 16 bytes);
// cb: 2 * Nr * nc[1].
template <typename T, int HL, int NT, typename Bar>
__host__ __device__ __forceinline__ void ext2db_inv_image(T* ra, T* rd, T* cb, T* __restrict__ dst, const Ext2dbBands<T>& b, size_t ib, const Taps2<T>& taps, int tid, Bar bar)
{
    const int L = b.nlev;
    img_copy_in<T, NT>(ra, b.p[0] + ib * ((size_t)b.nr[L] * b.nc[L]), b.nr[L] * b.nc[L], tid);
    for (int lev = L; lev >= 1; lev--) {
        const int nr = b.nr[lev - 1], nc = b.nc[lev - 1], hr = b.nr[lev], hc = b.nc[lev], per = hr * hc;
        const size_t o = ib * (size_t)per;
        T* const* d = b.p + 3 * (lev - 1) + 1;
        T* cb1 = cb + nr * hc;
        img_copy_in<T, NT>(rd, d[0] + o, per, tid);  // H  (rd was last read two barriers ago)
        bar();
        img_cols_synthesis<T, HL, false, 1, NT>(ra, rd, 0, cb, nullptr, nullptr, 1, nr, hr, hc, taps, tid);
        bar();
        img_copy_in<T, NT>(ra, d[1] + o, per, tid);  // V
        img_copy_in<T, NT>(rd, d[2] + o, per, tid);  // D
        bar();
        img_cols_synthesis<T, HL, false, 1, NT>(ra, rd, 0, cb1, nullptr, nullptr, 1, nr, hr, hc, taps, tid);
        bar();
        if (lev == 1) {
            img_rows_synthesis<T, HL, false, 1, NT>(cb, dst + ib * ((size_t)nr * nc), nullptr, nullptr, 1, nr, nc, hc, taps, tid);
            break;
        }
        img_rows_synthesis<T, HL, false, 1, NT>(cb, ra, nullptr, nullptr, 1, nr, nc, hc, taps, tid);  // A_{lev-1}, complete at the barrier after the next H is staged
    }
}

}  // namespace pdwt
