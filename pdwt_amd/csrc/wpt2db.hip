// wpt2db.hip -- the batched 2-D wavelet packet transform (include/pdwt_hip.h "Batched 2-D wavelet packets"; the class:
// WaveletPacketsImages, include/wpt_batch.h): the full quad-tree of wpt2d.hip on every image of a B x Nr x Nc stack.  Depth l of the batch
// is ONE allocation (B, 4^l, nr_l, nc_l), image-major: image b's depth-l line is one contiguous run, and the batch is a FOREST -- image
// b's node i is forest node g = b 4^l + i with the children 4g .. 4g + 3, the addressing of the level entries of wpt2d.hip.
//   k_wpb_fwd_fused       the WHOLE tree of one image per workgroup (grid.x = B): the image is staged into LDS once (16-byte loads), every
//                         depth is a row pass LDS -> LDS over all 4^l nodes and a column pass whose four children go to HBM from registers
//                         and (unless it is the last depth) over the LDS copy in the layout of the next depth.  Traffic: one read of the
//                         batch, one write of each depth.
//   k_wpb_inv_fused       climbs from depth L to 0 in LDS under a table of one byte per node (LOAD: a basis node, staged from HBM; SYNTH:
//                         made from its four children; SKIP: below the basis), staged into LDS once; a per-depth summary (all / none /
//                         mixed) in the kernel arguments spares the default basis every table read.  Writes the images only.
//   k_wpb_haar_*_fused    the same with the clamped 2x2 butterfly.
//   per depth             images that do not fit LDS, and allow_fused = 0: the level entries of wpt2d.hip on the forest, in chunks of at
//                         most 16384 parents (no kernel of its own).  4^l divides 16384, so a chunk is a whole number of images and the
//                         chunk-relative parent list of a partial basis is the SAME for every chunk (the last one takes a prefix).
// The pipelines of the fused kernels are the functions of wpt2db.hpp, their stages those of image_stages.hpp; all forms (and a loop over WaveletPackets instances) compute the same
// bits.  Barriers between LDS stages are LDS-only (lgkmcnt), so the child stores of a depth are not waited for.
//
// Workgroup size 512, for the reason given in dwt_ext2db.hip: an image above 80 KiB has the compute unit to itself and needs two waves per
// SIMD to hide the LDS latency of the tap loops.  A packet depth does not shrink: every depth has about Nr Nc / 4 positions.
// LDS rule (wpb_plan, the single source of truth), in elements, ru4 = rounded up to a multiple of 4:
//   cur = ru4(max_{l = 0..L} 4^l nr_l nc_l)          tmp = ru4(max(cur, max_{l < L} 2 4^l nr_l nc_{l+1}))
//   tab = ru4(2 max(nr_1, nc_1) + hlen - 2) ints     st  = ru16(sum_{l <= L} 4^l) bytes
//   forward (cur + tmp) elem + 8 tab;  inverse the same + st.  Fused when the larger fits 160 KiB.
#include <algorithm>

#include "wpt2db.hpp"

namespace pdwt {

constexpr int kWpbMaxBatch = 65535;
constexpr long long kWpbMaxForest = 1ll << 22;  // B 4^L: bounds the pointer and state tables of the class
constexpr int kWpbChunk = 16384;                // parents per launch of a level entry of wpt2d.hip

template <typename T, int HL>
__global__ __launch_bounds__(kWpbThreads) void k_wpb_fwd_fused(const T* __restrict__ src, WpbTree<T> t, WpbLds lds, Taps2<T> taps)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    T* cur = reinterpret_cast<T*>(smem);
    T* tmp = cur + lds.cur;
    int* cmap = reinterpret_cast<int*>(tmp + lds.tmp);
    wpb_fwd_image<T, HL, kWpbThreads>(cur, tmp, cmap, cmap + lds.tab, src, t, (size_t)blockIdx.x, taps, (int)threadIdx.x, LdsBarrier());
}

template <typename T, int HL>
__global__ __launch_bounds__(kWpbThreads) void k_wpb_inv_fused(T* __restrict__ dst, WpbTree<T> t, const unsigned char* __restrict__ state, WpbLds lds, Taps2<T> taps)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    T* cur = reinterpret_cast<T*>(smem);
    T* tmp = cur + lds.cur;
    int* cmap = reinterpret_cast<int*>(tmp + lds.tmp);
    unsigned char* stl = reinterpret_cast<unsigned char*>(cmap + 2 * lds.tab);
    wpb_inv_image<T, HL, kWpbThreads>(cur, tmp, cmap, cmap + lds.tab, stl, state, dst, t, (size_t)blockIdx.x, taps, (int)threadIdx.x, LdsBarrier());
}

template <typename T>
__global__ __launch_bounds__(kWpbThreads) void k_wpb_haar_fwd_fused(const T* __restrict__ src, WpbTree<T> t, WpbLds lds)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    T* b0 = reinterpret_cast<T*>(smem);
    wpb_haar_fwd_image<T, kWpbThreads>(b0, b0 + lds.cur, src, t, (size_t)blockIdx.x, (int)threadIdx.x, LdsBarrier());
}

template <typename T>
__global__ __launch_bounds__(kWpbThreads) void k_wpb_haar_inv_fused(T* __restrict__ dst, WpbTree<T> t, const unsigned char* __restrict__ state, WpbLds lds)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    T* b0 = reinterpret_cast<T*>(smem);
    unsigned char* stl = reinterpret_cast<unsigned char*>(reinterpret_cast<int*>(b0 + lds.cur + lds.tmp) + 2 * lds.tab);
    wpb_haar_inv_image<T, kWpbThreads>(b0, b0 + lds.cur, stl, state, dst, t, (size_t)blockIdx.x, (int)threadIdx.x, LdsBarrier());
}

// ---- geometry (host, no device; the plan is wpb_plan of wpt2db.hpp) -------------------------------------------------------------------
// WaveletPackets::geometry: the clamped depth (0: too small, a bad size or a bad bank) and the node shapes of depth 0 .. that depth
static int wpb_geometry(int Nr, int Nc, int hlen, int levels, int* nr, int* nc)
{
    if (Nr < 1 || Nc < 1 || !packet_bank_ok(hlen) || (unsigned long long)Nr * (unsigned long long)Nc >= (1ull << 31)) return 0;
    if (levels < 1) levels = 1;
    int lmax = packet_ilog2((Nr < Nc ? Nr : Nc) / (hlen - 1));
    if (lmax > kWpbMaxLev) lmax = kWpbMaxLev;
    if (levels > lmax) levels = lmax;
    for (int l = 0; l <= levels; l++) {
        if (nr) nr[l] = Nr;
        if (nc) nc[l] = Nc;
        Nr = div2(Nr), Nc = div2(Nc);
    }
    return levels;
}
// a tree of exactly `levels` depths over a batch of B such images exists
static bool wpb_ok(long long B, int Nr, int Nc, int hlen, int levels)
{
    if (B < 1 || B > kWpbMaxBatch || levels < 1 || levels > kWpbMaxLev) return false;
    if (wpb_geometry(Nr, Nc, hlen, levels, nullptr, nullptr) != levels) return false;
    return B * (long long)wpb_nodes(levels) <= kWpbMaxForest;
}

template <typename T>
static bool wpb_fill_tree(WpbTree<T>& t, T* const* nodes, int Nr, int Nc, int L)
{
    if (!nodes) return false;
    t.L = L, t.nr[0] = Nr, t.nc[0] = Nc;
    for (int l = 0; l <= kWpbMaxLev; l++) t.p[l] = nullptr, t.synth[l] = t.load[l] = WPB_NONE;
    for (int l = 1; l <= kWpbMaxLev; l++) t.nr[l] = t.nc[l] = 0;
    for (int l = 1; l <= L; l++) {
        if (!nodes[l - 1]) return false;
        t.p[l] = nodes[l - 1], t.nr[l] = div2(t.nr[l - 1]), t.nc[l] = div2(t.nc[l - 1]);
    }
    return true;
}

// Is the table one a state_table call can have written?  (The kernels index LDS by it: checked before every inverse.)
static bool wpb_state_valid(int L, const unsigned char* st)
{
    if (st[0] != WPB_SYNTH) return false;
    for (int l = 0; l <= L; l++)
        for (int i = 0; i < wpb_nodes(l); i++) {
            const unsigned char s = st[wpb_state_off(l) + i];
            if (s > WPB_SYNTH || (l == L && s == WPB_SYNTH)) return false;
            if (l == L) continue;
            const unsigned char* kid = st + wpb_state_off(l + 1) + 4 * i;
            for (int q = 0; q < 4; q++)
                if ((s == WPB_SYNTH) != (kid[q] != WPB_SKIP)) return false;  // a SYNTH parent has four live children, any other none
        }
    return true;
}

static unsigned char wpb_summary(const unsigned char* st, int n, unsigned char what)
{
    int cnt = 0;
    for (int i = 0; i < n; i++) cnt += st[i] == what;
    return cnt == 0 ? WPB_NONE : cnt == n ? WPB_ALL : WPB_MIXED;
}

// chunk-relative parent lists of the per-depth inverse: depth l (0 .. L-1) at wpb_list_off(B, l), for each of the min(B, 16384 / 4^l) images
// of a chunk, in image order, its SYNTH parents j 4^l + i.  Returns the ints of all depths; writes when lists != NULL.
static long long wpb_list_off(long long B, int l)
{
    long long off = 0;
    for (int k = 0; k < l; k++) off += std::min<long long>(B * wpb_nodes(k), kWpbChunk);
    return off;
}
static long long wpb_chunk_lists(long long B, int L, const unsigned char* st, int* lists)
{
    if (lists)
        for (int l = 0; l < L; l++) {
            const int n = wpb_nodes(l), imgs = (int)std::min<long long>(B, kWpbChunk / n);
            int* o = lists + wpb_list_off(B, l);
            for (int j = 0; j < imgs; j++)
                for (int i = 0; i < n; i++)
                    if (st[wpb_state_off(l) + i] == WPB_SYNTH) *o++ = j * n + i;
        }
    return wpb_list_off(B, L);
}

// ---- drivers ------------------------------------------------------------------------------------------------------------------------
template <typename T> struct WpbLevelFn;
template <> struct WpbLevelFn<float> {
    static int fwd(const float* p, float* c, int nr, int nc, const int* l, int n, const pdwt_filters_f32* f) { return pdwt_wpt2d_forward_level_f32(p, c, nr, nc, l, n, f); }
    static int inv(float* p, const float* c, int nr, int nc, const int* l, int n, const pdwt_filters_f32* f) { return pdwt_wpt2d_inverse_level_f32(p, c, nr, nc, l, n, f); }
};
template <> struct WpbLevelFn<double> {
    static int fwd(const double* p, double* c, int nr, int nc, const int* l, int n, const pdwt_filters_f64* f) { return pdwt_wpt2d_forward_level_f64(p, c, nr, nc, l, n, f); }
    static int inv(double* p, const double* c, int nr, int nc, const int* l, int n, const pdwt_filters_f64* f) { return pdwt_wpt2d_inverse_level_f64(p, c, nr, nc, l, n, f); }
};

template <typename T, int HL>
static int launch_wpb_fwd(const T* src, const WpbTree<T>& t, int B, const WpbPlan& p, const Taps2<T>& taps)
{
    int rc;
    if constexpr (HL == 2) rc = launch_lds(k_wpb_haar_fwd_fused<T>, dim3(B), dim3(kWpbThreads), p.lds_fwd, src, t, p.lds);
    else rc = launch_lds(k_wpb_fwd_fused<T, HL>, dim3(B), dim3(kWpbThreads), p.lds_fwd, src, t, p.lds, taps);
    return rc == PDWT_OK ? PDWT_WPTB_FUSED : rc;
}
template <typename T, int HL>
static int launch_wpb_inv(T* dst, const WpbTree<T>& t, const unsigned char* d_state, int B, const WpbPlan& p, const Taps2<T>& taps)
{
    int rc;
    if constexpr (HL == 2) rc = launch_lds(k_wpb_haar_inv_fused<T>, dim3(B), dim3(kWpbThreads), p.lds_inv, dst, t, d_state, p.lds);
    else rc = launch_lds(k_wpb_inv_fused<T, HL>, dim3(B), dim3(kWpbThreads), p.lds_inv, dst, t, d_state, p.lds, taps);
    return rc == PDWT_OK ? PDWT_WPTB_FUSED : rc;
}

template <typename T>
static int wpb_forward(const T* src, T* const* nodes, int B, int Nr, int Nc, int levels, const typename FiltersOf<T>::type* f, int allow_fused)
{
    WpbTree<T> t;
    if (!src || !f || !wpb_ok(B, Nr, Nc, f->hlen, levels) || !wpb_fill_tree(t, nodes, Nr, Nc, levels)) return PDWT_EINVAL;
    const WpbPlan p = wpb_plan(Nr, Nc, f->hlen, levels, sizeof(T));
    if (p.fused && allow_fused) {
        const Taps2<T> taps = taps_fwd<T>(f);
        return with_filter_length<2>(f->hlen, [&](auto hl) { return launch_wpb_fwd<T, decltype(hl)::value>(src, t, B, p, taps); });
    }
    for (int l = 0; l < levels; l++) {
        const long long parents = (long long)B * wpb_nodes(l);
        const size_t ps = (size_t)t.nr[l] * t.nc[l], cs = (size_t)t.nr[l + 1] * t.nc[l + 1];
        const T* par = l == 0 ? src : t.p[l];
        for (long long c0 = 0; c0 < parents; c0 += kWpbChunk) {
            const int n = (int)std::min<long long>(kWpbChunk, parents - c0);
            if (const int rc = WpbLevelFn<T>::fwd(par + (size_t)c0 * ps, t.p[l + 1] + 4 * (size_t)c0 * cs, t.nr[l], t.nc[l], nullptr, n, f); rc != PDWT_OK) return rc;
        }
    }
    return PDWT_WPTB_LEVELS;
}

// state: the HOST table of pdwt_wptb_state_table; d_state: its device copy (read by the fused form); d_lists: the device copy of
// pdwt_wptb_chunk_lists (read by the per-depth form at the depths that hold SYNTH parents and others)
template <typename T>
static int wpb_inverse(T* dst, T* const* nodes, int B, int Nr, int Nc, int levels, const unsigned char* state, const unsigned char* d_state, const int* d_lists,
                       const typename FiltersOf<T>::type* f, int allow_fused)
{
    WpbTree<T> t;
    if (!dst || !f || !state || !wpb_ok(B, Nr, Nc, f->hlen, levels) || !wpb_fill_tree(t, nodes, Nr, Nc, levels) || !wpb_state_valid(levels, state)) return PDWT_EINVAL;
    for (int l = 0; l <= levels; l++) {
        t.synth[l] = wpb_summary(state + wpb_state_off(l), wpb_nodes(l), WPB_SYNTH);
        t.load[l] = wpb_summary(state + wpb_state_off(l), wpb_nodes(l), WPB_LOAD);
    }
    const WpbPlan p = wpb_plan(Nr, Nc, f->hlen, levels, sizeof(T));
    if (p.fused && allow_fused) {
        if (!d_state) return PDWT_EINVAL;
        const Taps2<T> taps = taps_inv<T>(f);
        return with_filter_length<2>(f->hlen, [&](auto hl) { return launch_wpb_inv<T, decltype(hl)::value>(dst, t, d_state, B, p, taps); });
    }
    for (int l = 0; l < levels; l++)
        if (t.synth[l] == WPB_MIXED && !d_lists) return PDWT_EINVAL;  // (before anything is launched)
    for (int l = levels - 1; l >= 0; l--) {
        if (t.synth[l] == WPB_NONE) continue;
        const int n4 = wpb_nodes(l);
        int nsynth = 0;
        for (int i = 0; i < n4; i++) nsynth += state[wpb_state_off(l) + i] == WPB_SYNTH;
        const long long parents = (long long)B * n4;
        const size_t ps = (size_t)t.nr[l] * t.nc[l], cs = (size_t)t.nr[l + 1] * t.nc[l + 1];
        T* par = l == 0 ? dst : t.p[l];
        const int* list = t.synth[l] == WPB_MIXED ? d_lists + wpb_list_off(B, l) : nullptr;
        for (long long c0 = 0; c0 < parents; c0 += kWpbChunk) {
            const int n = (int)std::min<long long>(kWpbChunk, parents - c0);  // a whole number of images: 4^l divides the chunk
            const int count = list ? (n / n4) * nsynth : n;
            if (const int rc = WpbLevelFn<T>::inv(par + (size_t)c0 * ps, t.p[l + 1] + 4 * (size_t)c0 * cs, t.nr[l], t.nc[l], list, count, f); rc != PDWT_OK) return rc;
        }
    }
    return PDWT_WPTB_LEVELS;
}

}  // namespace pdwt

using namespace pdwt;

extern "C" {
int pdwt_wptb_geometry(int Nr, int Nc, int hlen, int levels, int* nr, int* nc) { return wpb_geometry(Nr, Nc, hlen, levels, nr, nc); }
int pdwt_wptb_fused(int Nr, int Nc, int hlen, int levels, int elem_size)
{
    const int L = wpb_geometry(Nr, Nc, hlen, levels, nullptr, nullptr);
    if (L < 1 || (elem_size != 4 && elem_size != 8)) return PDWT_EINVAL;
    return wpb_plan(Nr, Nc, hlen, L, (size_t)elem_size).fused ? 1 : 0;
}
long long pdwt_wptb_lds_bytes(int Nr, int Nc, int hlen, int levels, int elem_size, int dir)
{
    const int L = wpb_geometry(Nr, Nc, hlen, levels, nullptr, nullptr);
    if (L < 1 || (elem_size != 4 && elem_size != 8) || (dir != 0 && dir != 1)) return PDWT_EINVAL;
    const WpbPlan p = wpb_plan(Nr, Nc, hlen, L, (size_t)elem_size);
    return (long long)(dir == 0 ? p.lds_fwd : p.lds_inv);
}
long long pdwt_wptb_tmp_elems(int B, int Nr, int Nc, int hlen, int levels, int elem_size, int allow_fused)
{
    const int fu = pdwt_wptb_fused(Nr, Nc, hlen, levels, elem_size);
    const int L = wpb_geometry(Nr, Nc, hlen, levels, nullptr, nullptr);
    if (fu < 0 || !wpb_ok(B, Nr, Nc, hlen, L)) return PDWT_EINVAL;
    return fu && allow_fused ? 0 : wpb_list_off(B, L);
}
int pdwt_wptb_state_table(int levels, const int* depth, const int* idx, int n, unsigned char* out) { return packet_state_table<4>(levels, kWpbMaxLev, depth, idx, n, out); }
long long pdwt_wptb_chunk_lists(int B, int levels, const unsigned char* state, int* lists)
{
    if (B < 1 || B > kWpbMaxBatch || levels < 1 || levels > kWpbMaxLev || !state || (long long)B * wpb_nodes(levels) > kWpbMaxForest || !wpb_state_valid(levels, state))
        return PDWT_EINVAL;
    return wpb_chunk_lists(B, levels, state, lists);
}
int pdwt_wptb_forward_f32(const float* d_src, float* const* d_nodes, int B, int Nr, int Nc, int levels, const pdwt_filters_f32* f, int allow_fused)
{
    return wpb_forward<float>(d_src, d_nodes, B, Nr, Nc, levels, f, allow_fused);
}
int pdwt_wptb_forward_f64(const double* d_src, double* const* d_nodes, int B, int Nr, int Nc, int levels, const pdwt_filters_f64* f, int allow_fused)
{
    return wpb_forward<double>(d_src, d_nodes, B, Nr, Nc, levels, f, allow_fused);
}
int pdwt_wptb_inverse_f32(float* d_dst, float* const* d_nodes, int B, int Nr, int Nc, int levels, const unsigned char* state, const unsigned char* d_state, const int* d_lists,
                          const pdwt_filters_f32* f, int allow_fused)
{
    return wpb_inverse<float>(d_dst, d_nodes, B, Nr, Nc, levels, state, d_state, d_lists, f, allow_fused);
}
int pdwt_wptb_inverse_f64(double* d_dst, double* const* d_nodes, int B, int Nr, int Nc, int levels, const unsigned char* state, const unsigned char* d_state, const int* d_lists,
                          const pdwt_filters_f64* f, int allow_fused)
{
    return wpb_inverse<double>(d_dst, d_nodes, B, Nr, Nc, levels, state, d_state, d_lists, f, allow_fused);
}
}
