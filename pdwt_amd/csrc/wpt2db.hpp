// wpt2db.hpp -- the pipelines of the fused kernels of the batched 2-D wavelet packet transform (wpt2db.hip; include/pdwt_hip.h "Batched
// 2-D wavelet packets"): the whole quad-tree of ONE image in the LDS of one workgroup.  The stages are those of image_stages.hpp, shared
// with the inverse of the boundary modes (dwt_ext2db.hpp), run on the periodised line: window offset -(F/2 - 1), 2 * 4^l line pairs per
// pass, a synthesis with shift, centre and table under an optional state table.  Every stage takes the thread count as a template
// argument and the thread index as an argument and contains no barrier; the pipelines (wpb_*_image) take the barrier as a functor.  The kernels pass the LDS-only barrier and NT = 512; a host program passes a no-op and NT = 1, tid = 0 and
// runs whole pipelines on the CPU under a sanitizer.
//
// Values.  The operation sequence is that of k_wp_fwd / k_wp_inv (wpt2d.hip), so the results are the same bits: forward rows first with
// the intermediate rounded to T, then columns, one FMA per tap in ascending order of the window; inverse columns first, the (A, H) and
// (V, D) sums added once each, then rows, the low and high sums added once.  Haar is the clamped 2x2 butterfly of k_wp_haar_*.
//
// LDS: [cur | tmp | cmap | rmap | state].  A depth l lies in `cur` exactly as in HBM: 4^l nodes of nr_l x nc_l, contiguous, so the rows
// of all nodes are ONE run of 4^l nr_l rows and an offset inside the image's depth-l line is the offset inside cur.
//   forward  row pass of every node cur -> tmp (low | high, 4^l nr_l rows of nc_{l+1}), column pass tmp -> the four children, to HBM and
//            (unless this is the last depth) over cur in the layout of depth l + 1
//   inverse  column synthesis of every SYNTH parent cur (children, depth l + 1) -> tmp ((A, H) | (V, D) per parent, nr_l rows of nc_{l+1}),
//            row synthesis tmp -> cur in the layout of depth l (depth 0: the image in HBM); the LOAD nodes of depth l are staged next to them
//   Haar     no row pass: the butterfly goes from one buffer to the other, the two taking turns
// The periodic wrap is read through two source-index tables per depth (all nodes of a depth have one shape, so one table serves them
// all): windows that lie inside the line -- all but about F / 2 at each end -- skip the table.
#pragma once
#include <algorithm>

#include "image_stages.hpp"

namespace pdwt {

constexpr int kWpbThreads = 512;
constexpr int kWpbMaxLev = 7;  // WPT_MAX_LEVELS

// node states of the inverse (one byte per node, node i of depth l at (4^l - 1) / 3 + i) and what a depth holds of one of them
enum WpbState : unsigned char { WPB_SKIP = 0, WPB_LOAD = 1, WPB_SYNTH = 2 };
static_assert((int)WPB_SKIP == (int)WP1_SKIP && (int)WPB_LOAD == (int)WP1_LOAD && (int)WPB_SYNTH == (int)WP1_SYNTH && WPB_SYNTH == kImgSynth,
              "one table format: packet_state_table (wpt1d.hpp) writes it, the stages of image_stages.hpp read it");
enum WpbSummary : unsigned char { WPB_NONE = 0, WPB_ALL = 1, WPB_MIXED = 2 };

template <typename T>
struct WpbTree {
    T* p[kWpbMaxLev + 1];                          // p[l], l = 1 .. L: the allocation of depth l, (B, 4^l, nr[l], nc[l]); p[0] unused
    int nr[kWpbMaxLev + 1], nc[kWpbMaxLev + 1];    // [0] the image
    int L;
    unsigned char synth[kWpbMaxLev + 1], load[kWpbMaxLev + 1];  // inverse: WpbSummary of the SYNTH / LOAD nodes of each depth
};

__host__ __device__ inline int wpb_nodes(int l) { return 1 << (2 * l); }
__host__ __device__ inline int wpb_state_off(int l) { return (wpb_nodes(l) - 1) / 3; }

// ---- the plan (host, no device): the single source of the decision and of the LDS bytes of both launches ----------------------------------
struct WpbLds {
    int cur, tmp, tab;  // elements, elements, ints
};

struct WpbPlan {
    bool fused;
    WpbLds lds;
    size_t lds_fwd, lds_inv;  // bytes of a workgroup (one image)
};
inline WpbPlan wpb_plan(int Nr, int Nc, int hlen, int L, size_t elem)
{
    int nr[kWpbMaxLev + 1], nc[kWpbMaxLev + 1];
    nr[0] = Nr, nc[0] = Nc;
    for (int l = 1; l <= L; l++) nr[l] = div2(nr[l - 1]), nc[l] = div2(nc[l - 1]);
    size_t cur = 0, tmp = 0;
    for (int l = 0; l <= L; l++) cur = std::max(cur, (size_t)wpb_nodes(l) * nr[l] * nc[l]);
    for (int l = 0; l < L; l++) tmp = std::max(tmp, 2 * (size_t)wpb_nodes(l) * nr[l] * nc[l + 1]);
    cur = (cur + 3) & ~(size_t)3;
    tmp = (std::max(cur, tmp) + 3) & ~(size_t)3;
    const size_t tab = (size_t)ext1d_ru4(2 * std::max(nr[1], nc[1]) + hlen - 2);
    const size_t st = ((size_t)wpb_state_off(L + 1) + 15) & ~(size_t)15;
    WpbPlan p;
    p.lds_fwd = (cur + tmp) * elem + 2 * tab * sizeof(int);
    p.lds_inv = p.lds_fwd + st;
    p.fused = std::max(p.lds_fwd, p.lds_inv) <= kLdsMax;
    p.lds.cur = p.fused ? (int)cur : 0, p.lds.tmp = p.fused ? (int)tmp : 0, p.lds.tab = (int)tab;
    return p;
}

// ---- forward ----------------------------------------------------------------------------------------------------------------------------
// map[k] = the sample that xe[k - (F/2 - 1)] repeats, k = 0 .. 2 * half + F - 3: the windows of the `half` positions of a line of n samples
template <int NT>
__host__ __device__ __forceinline__ void wpb_fill_fmap(int* map, int n, int half, int F, int tid)
{
    img_fill_map<NT>(map, 2 * half + F - 2, [&](int k) { return wp1_wrap_ext(k - (F / 2 - 1), n); }, tid);
}

// The column pass of a depth: lanes write contiguous runs of a child node (4k + 2xb, and its neighbour), to the image's depth-(l+1) line
// at g and, nxt != NULL, to the same offsets of nxt.  (g is a parameter so that it can be __restrict__ for the whole pass.)
template <typename T, int HL, int NT>
__host__ __device__ __forceinline__ void wpb_cols_analysis(const T* tmp, const int* rmap, T* nxt, T* __restrict__ g, int nodes, int nr, int hr, int hc, const Taps2<T>& taps,
                                                           int tid)
{
    const int per = hr * hc;
    img_cols_analysis<T, HL, -(HL / 2 - 1), NT>(tmp, rmap, 2 * nodes, nr, hr, hc, taps, tid, [&](int kb, int o, T lo, T hi) {
        const int off = (2 * kb) * per + o;
        g[off] = lo;
        g[off + per] = hi;
        if (nxt) {
            nxt[off] = lo;
            nxt[off + per] = hi;
        }
    });
}

// All depths of image `ib`.  cur: cur_elems of the plan, tmp likewise, cmap / rmap: `tab` ints each.
template <typename T, int HL, int NT, typename Bar>
__host__ __device__ __forceinline__ void wpb_fwd_image(T* cur, T* tmp, int* cmap, int* rmap, const T* __restrict__ src, const WpbTree<T>& t, size_t ib, const Taps2<T>& taps,
                                                       int tid, Bar bar)
{
    const int L = t.L;
    img_copy_in<T, NT>(cur, src + ib * ((size_t)t.nr[0] * t.nc[0]), t.nr[0] * t.nc[0], tid);
    wpb_fill_fmap<NT>(cmap, t.nc[0], t.nc[1], HL, tid);
    bar();
    for (int l = 0; l < L; l++) {
        const int nodes = wpb_nodes(l), nr = t.nr[l], nc = t.nc[l], hr = t.nr[l + 1], hc = t.nc[l + 1];
        wpb_fill_fmap<NT>(rmap, nr, hr, HL, tid);  // (read by the column pass, after the barrier; the last one was read before the previous)
        img_rows_analysis<T, HL, -(HL / 2 - 1), NT>(cur, tmp, cmap, nodes * nr, nc, hc, taps, tid);
        bar();
        const bool last = l + 1 == L;
        T* g = t.p[l + 1] + ib * ((size_t)(4 * nodes) * hr * hc);
        wpb_cols_analysis<T, HL, NT>(tmp, rmap, last ? (T*)nullptr : cur, g, nodes, nr, hr, hc, taps, tid);
        if (last) break;
        wpb_fill_fmap<NT>(cmap, hc, t.nc[l + 2], HL, tid);  // (the row pass that read cmap is behind the barrier)
        bar();
    }
}

// Haar: the butterfly of k_wp_haar_fwd, one work item per child position; b0 and b1 hold cur_elems each
template <typename T, int NT, typename Bar>
__host__ __device__ __forceinline__ void wpb_haar_fwd_image(T* b0, T* b1, const T* __restrict__ src, const WpbTree<T>& t, size_t ib, int tid, Bar bar)
{
    const int L = t.L;
    img_copy_in<T, NT>(b0, src + ib * ((size_t)t.nr[0] * t.nc[0]), t.nr[0] * t.nc[0], tid);
    bar();
    T *cur = b0, *nxt = b1;
    for (int l = 0; l < L; l++) {
        const int nodes = wpb_nodes(l), nr = t.nr[l], nc = t.nc[l], hr = t.nr[l + 1], hc = t.nc[l + 1];
        const int per = hr * hc, total = nodes * per;
        const bool last = l + 1 == L;
        T* __restrict__ g = t.p[l + 1] + ib * ((size_t)(4 * nodes) * per);
        for (int e = tid; e < total; e += NT) {
            const int k = e / per, o = e - k * per, y = o / hc, xx = o - y * hc;
            const T* x = cur + k * nr * nc;
            const int y0 = 2 * y, y1 = (2 * y + 1 == nr) ? nr - 1 : 2 * y + 1;
            const int x0 = 2 * xx, x1 = (2 * xx + 1 == nc) ? nc - 1 : 2 * xx + 1;
            const T a = x[y0 * nc + x0], b = x[y0 * nc + x1], cc = x[y1 * nc + x0], d = x[y1 * nc + x1];
            const T qa = T(0.5) * ((a + cc) + (b + d)), qh = T(0.5) * ((a - cc) + (b - d));
            const T qv = T(0.5) * ((a + cc) - (b + d)), qd = T(0.5) * ((a - cc) - (b - d));
            const int off = 4 * k * per + o;
            g[off] = qa, g[off + per] = qh, g[off + 2 * per] = qv, g[off + 3 * per] = qd;
            if (!last) nxt[off] = qa, nxt[off + per] = qh, nxt[off + 2 * per] = qv, nxt[off + 3 * per] = qd;
        }
        if (last) break;
        bar();
        T* s = cur;
        cur = nxt, nxt = s;
    }
}

// ---- inverse ----------------------------------------------------------------------------------------------------------------------------
// map[k] = (k - F/4) mod N, k = 0 .. pairs + F/2 - 2: the windows of the sample pairs of a parent line of n samples (N = div2(n) coefficients)
template <int NT>
__host__ __device__ __forceinline__ void wpb_fill_imap(int* map, int n, int N, int F, int tid)
{
    img_fill_map<NT>(map, wp1_pairs(n, F) + F / 2 - 1, [&](int k) { return wp1_wrap_per(k - F / 4, N); }, tid);
}

// Stage the LOAD nodes of a depth (`nodes` of `per` elements, the image's line at g) into buf at their own offsets
template <typename T, int NT>
__host__ __device__ __forceinline__ void wpb_stage_nodes(T* buf, const T* __restrict__ g, const unsigned char* st, int summary, int nodes, int per, int tid)
{
    if (summary == WPB_ALL) {
        img_copy_in<T, NT>(buf, g, nodes * per, tid);
    } else if (summary == WPB_MIXED) {
        const int total = nodes * per;
        for (int e = tid; e < total; e += NT)
            if (st[e / per] == WPB_LOAD) buf[e] = g[e];
    }
}

// Stage the state table into LDS when some depth needs it; returns the LDS copy or NULL.  Needs a barrier before the first use.
template <typename T, int NT>
__host__ __device__ __forceinline__ const unsigned char* wpb_stage_state(unsigned char* stl, const unsigned char* __restrict__ state, const WpbTree<T>& t, int tid)
{
    bool mixed = false;
    for (int l = 0; l <= t.L; l++) mixed = mixed || t.synth[l] == WPB_MIXED || t.load[l] == WPB_MIXED;
    if (!mixed) return nullptr;
    const int total = wpb_state_off(t.L + 1);
    for (int i = tid; i < total; i += NT) stl[i] = state[i];
    return stl;
}

// Image `ib` from depth L to 0 under the state table (root: SYNTH).  Writes the image only.
template <typename T, int HL, int NT, typename Bar>
__host__ __device__ __forceinline__ void wpb_inv_image(T* cur, T* tmp, int* cmap, int* rmap, unsigned char* stl, const unsigned char* __restrict__ state, T* __restrict__ dst,
                                                       const WpbTree<T>& t, size_t ib, const Taps2<T>& taps, int tid, Bar bar)
{
    const int L = t.L;
    const unsigned char* st = wpb_stage_state<T, NT>(stl, state, t, tid);
    if (st) bar();
    {
        const int per = t.nr[L] * t.nc[L];
        wpb_stage_nodes<T, NT>(cur, t.p[L] + ib * ((size_t)wpb_nodes(L) * per), st + (st ? wpb_state_off(L) : 0), t.load[L], wpb_nodes(L), per, tid);
    }
    wpb_fill_imap<NT>(rmap, t.nr[L - 1], t.nr[L], HL, tid);
    bar();
    for (int l = L - 1; l >= 0; l--) {
        const int nodes = wpb_nodes(l), nr = t.nr[l], nc = t.nc[l], hr = t.nr[l + 1], hc = t.nc[l + 1];
        const unsigned char* sl = t.synth[l] == WPB_MIXED ? st + wpb_state_off(l) : nullptr;
        const bool any = t.synth[l] != WPB_NONE;
        wpb_fill_imap<NT>(cmap, nc, hc, HL, tid);  // (its last reader, the row synthesis of the depth below, is behind a barrier)
        // the children of every SYNTH parent: cur holds depth l + 1 (4 * nodes nodes of hr x hc); tmp receives [nodes][2][nr][hc]
        if (any) img_cols_synthesis<T, HL, true, 0, NT>(cur, cur + hr * hc, 2 * hr * hc, tmp, rmap, sl, 2 * nodes, nr, hr, hc, taps, tid);
        bar();
        if (l == 0) {
            if (any) img_rows_synthesis<T, HL, true, 0, NT>(tmp, dst + ib * ((size_t)nr * nc), cmap, sl, 1, nr, nc, hc, taps, tid);
            break;
        }
        if (any) img_rows_synthesis<T, HL, true, 0, NT>(tmp, cur, cmap, sl, nodes, nr, nc, hc, taps, tid);
        wpb_stage_nodes<T, NT>(cur, t.p[l] + ib * ((size_t)nodes * nr * nc), st + (st ? wpb_state_off(l) : 0), t.load[l], nodes, nr * nc, tid);
        wpb_fill_imap<NT>(rmap, t.nr[l - 1], nr, HL, tid);
        bar();
    }
}

// Haar: the butterfly of k_wp_haar_inv, one work item per parent sample; the two buffers take turns
template <typename T, int NT, typename Bar>
__host__ __device__ __forceinline__ void wpb_haar_inv_image(T* b0, T* b1, unsigned char* stl, const unsigned char* __restrict__ state, T* __restrict__ dst, const WpbTree<T>& t,
                                                            size_t ib, int tid, Bar bar)
{
    const int L = t.L;
    const unsigned char* st = wpb_stage_state<T, NT>(stl, state, t, tid);
    if (st) bar();
    T *ch = b0, *par = b1;
    {
        const int per = t.nr[L] * t.nc[L];
        wpb_stage_nodes<T, NT>(ch, t.p[L] + ib * ((size_t)wpb_nodes(L) * per), st + (st ? wpb_state_off(L) : 0), t.load[L], wpb_nodes(L), per, tid);
    }
    bar();
    for (int l = L - 1; l >= 0; l--) {
        const int nodes = wpb_nodes(l), nr = t.nr[l], nc = t.nc[l], hr = t.nr[l + 1], hc = t.nc[l + 1];
        const unsigned char* sl = t.synth[l] == WPB_MIXED ? st + wpb_state_off(l) : nullptr;
        const int per = nr * nc, cs = hr * hc, total = nodes * per;
        T* out = l == 0 ? dst + ib * (size_t)per : par;
        if (t.synth[l] != WPB_NONE)
            for (int e = tid; e < total; e += NT) {
                const int k = e / per, rem = e - k * per;
                if (sl && sl[k] != WPB_SYNTH) continue;
                const int y = rem / nc, xx = rem - y * nc;
                const T* c4 = ch + 4 * k * cs + (y >> 1) * hc + (xx >> 1);
                const T a = c4[0], cc = c4[cs], b = c4[2 * cs], d = c4[3 * cs];
                T r;
                if (!(y & 1)) r = (xx & 1) ? T(0.5) * ((a + cc) - (b + d)) : T(0.5) * ((a + cc) + (b + d));
                else r = (xx & 1) ? T(0.5) * ((a - cc) - (b - d)) : T(0.5) * ((a - cc) + (b - d));
                out[e] = r;
            }
        if (l == 0) break;
        wpb_stage_nodes<T, NT>(par, t.p[l] + ib * ((size_t)nodes * per), st + (st ? wpb_state_off(l) : 0), t.load[l], nodes, per, tid);
        bar();
        T* s = ch;
        ch = par, par = s;
    }
}

}  // namespace pdwt
