// wpt1d.hip -- the batched 1-D wavelet packet transform (include/pdwt_hip.h "Batched 1-D wavelet packets"; the class: WaveletPackets1D,
// include/wpt1d.h): the full binary tree of every row of an Nr x Nc batch, pywt.WaveletPacket(mode='periodization') in natural order.
// Depth l is ONE allocation (Nr, 2^l, n_l) row-major: a row's depth-l line is one contiguous run, so a workgroup that owns rows stores
// every depth fully coalesced however small n_l gets.  The stages are the functions of wpt1d.hpp; the kernels place buffers and barriers.
//   k_wp1_fwd_fused  ALL depths of a pack of R rows in one launch: the rows are staged into LDS once, every depth step is computed
//                    LDS -> registers, both children go straight to the depth-(l+1) allocation and (unless it is the last depth) into the
//                    other LDS buffer, whose per-node halos are then filled.  Traffic: one read of the batch, one write of each depth.
//   k_wp1_inv_fused  climbs from depth L to 0 in LDS under a table of one byte per node (LOAD: a basis node, staged from HBM; SYNTH:
//                    made from its two children; SKIP: below the basis).  Reads one batch worth of coefficients, writes the rows only.
//   k_wp1_fwd / k_wp1_inv  ONE depth step per launch over (tile, parent, row) flattened on grid.x, the bank length a run-time
//                    argument: rows that do not fit LDS, and the level entries of the C ABI.
//   k_wp1_moments    sum |c|, sum c^2, max |c| and -sum c^2 ln c^2 of every (row, node) segment of a depth, in double, fixed order.
//   k_wp1_thresh     soft / hard threshold in place on the segments whose node is flagged.
// Both transform forms run wp1_fwd_pos / wp1_inv_pos: bit-identical results.  Barriers between LDS stages are LDS-only (lgkmcnt), so
// the child stores of a depth are not waited for (dwt1d_fused.hip).
//
// LDS placement.  Two lines per row, of adjacent depths; a packet depth does not shrink (line(l) = 2^l segments).  Even depths grow
// from the bottom of the dynamic region, odd depths end at its top, so the region is R times the largest SUM of two adjacent lines.
// Row packing: R = the power of two >= 256 / div2(Nc) (every thread has a position at depth 1), at most 64 and as many as fit 32 KiB.
// Budget rule (needs no device): fused when that region, for ONE row, fits 160 KiB in both directions (pdwt_wp1_fused).
#include <algorithm>

#include "wpt1d.hpp"

namespace pdwt {

constexpr size_t kWp1PackLds = 32 * 1024;  // packs of several rows stay below this

template <typename T, int HL>
__global__ __launch_bounds__(kWp1Threads) void k_wp1_fwd_fused(const T* __restrict__ src, Wp1Levels<T> lv, int Nr, int R, int region, Taps2<T> taps)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    wp1_fwd_fused_block<T, HL, kWp1Threads>(reinterpret_cast<T*>(smem), region, src, lv, Nr, R, blockIdx.x, taps, threadIdx.x, LdsBarrier());
}

template <typename T, int HL>
__global__ __launch_bounds__(kWp1Threads) void k_wp1_inv_fused(T* __restrict__ dst, Wp1Levels<T> lv, const unsigned char* __restrict__ state, int Nr, int R, int region,
                                                               Taps2<T> taps)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    wp1_inv_fused_block<T, HL, kWp1Threads>(reinterpret_cast<T*>(smem), region, dst, lv, state, Nr, R, blockIdx.x, taps, threadIdx.x, LdsBarrier());
}

// src: (nr, nodes, n); dst: (nr, 2 * nodes, N).  blockIdx.x = (row * nodes + parent) * tiles + tile
template <typename T>
__global__ __launch_bounds__(kWp1Threads) void k_wp1_fwd(const T* __restrict__ src, T* __restrict__ dst, int n, int N, int tiles, int hlen, Taps2<T> taps)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    wp1_fwd_level_block<T, kWp1Threads>(reinterpret_cast<T*>(smem), src, dst, n, N, tiles, hlen, blockIdx.x, taps, threadIdx.x, LdsBarrier());
}

// par: (nr, nodes, n); child: (nr, 2 * nodes, N).  blockIdx.x = (row * count + position in the list) * tiles + tile; a parent whose
// state byte is given and is not SYNTH is left alone (the whole-inverse driver runs every depth under the state table)
template <typename T>
__global__ __launch_bounds__(kWp1Threads) void k_wp1_inv(T* __restrict__ par, const T* __restrict__ child, int n, int N, int nodes, const int* __restrict__ list, int count,
                                                         const unsigned char* __restrict__ st, int tiles, int hlen, Taps2<T> taps)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    wp1_inv_level_block<T, kWp1Threads>(reinterpret_cast<T*>(smem), par, child, n, N, nodes, list, count, st, tiles, hlen, blockIdx.x, taps, threadIdx.x, LdsBarrier());
}

// ---- moments ------------------------------------------------------------------------------------------------------------------------
// G lanes (a power of two <= 64) per segment of n contiguous elements: every lane adds its elements (stride G) in double, the G partial
// results are combined by a butterfly (the same order on every run and on every lane), lane 0 stores the four results.  No atomics.
template <typename T>
__global__ __launch_bounds__(kWp1Threads) void k_wp1_moments(const T* __restrict__ x, long long nseg, int n, int G, double* __restrict__ out)
{
    const int per_block = kWp1Threads / G, lane = threadIdx.x & (G - 1);
    const long long seg = (long long)blockIdx.x * per_block + threadIdx.x / G;
    double s1 = 0.0, s2 = 0.0, mx = 0.0, en = 0.0;
    if (seg < nseg) {
        const T* __restrict__ p = x + (size_t)seg * n;
        for (int i = lane; i < n; i += G) {
            const double v = (double)p[i], av = fabs(v), v2 = v * v;
            s1 += av;
            s2 += v2;
            mx = av > mx ? av : mx;
            if (v2 > 0.0) en -= v2 * log(v2);
        }
    }
    for (int d = G >> 1; d >= 1; d >>= 1) {
        s1 += __shfl_xor(s1, d, 64);
        s2 += __shfl_xor(s2, d, 64);
        en += __shfl_xor(en, d, 64);
        const double o = __shfl_xor(mx, d, 64);
        mx = o > mx ? o : mx;
    }
    if (seg < nseg && lane == 0) {
        double* o = out + 4 * (size_t)seg;
        o[0] = s1, o[1] = s2, o[2] = mx, o[3] = en;
    }
}

// ---- threshold ----------------------------------------------------------------------------------------------------------------------
// The formulas of utils.hip (ew_op): soft copysign(max(|x| - b, 0), x); hard x where |x| - b > 0, else 0 * x (keeps the sign of zero)
__device__ __forceinline__ float wp1_abs(float x) { return fabsf(x); }
__device__ __forceinline__ double wp1_abs(double x) { return fabs(x); }
__device__ __forceinline__ float wp1_copysign(float a, float s) { return copysignf(a, s); }
__device__ __forceinline__ double wp1_copysign(double a, double s) { return copysign(a, s); }

template <typename T>
__global__ __launch_bounds__(kWp1Threads) void k_wp1_thresh(T* __restrict__ x, unsigned long long total, unsigned n, unsigned nodes, const unsigned char* __restrict__ flags, int op,
                                                            T beta)
{
    const unsigned long long stride = (unsigned long long)gridDim.x * kWp1Threads;
    for (unsigned long long e = (unsigned long long)blockIdx.x * kWp1Threads + threadIdx.x; e < total; e += stride) {
        const unsigned node = ((unsigned)e / n) % nodes;  // (total < 2^32)
        if (flags[node] != 1) continue;
        const T v = x[e], m = wp1_abs(v) - beta;
        x[e] = op == 0 ? wp1_copysign(m > T(0) ? m : T(0), v) : (m > T(0) ? T(1) : T(0)) * v;
    }
}

// ---- geometry and the plan of the fused path (host, no device) ----------------------------------------------------------------------
// the clamped depth (0: too small or a bad size / bank) and n_0 .. n_L
static int wp1_geometry(int nc, int hlen, int levels, int* n)
{
    if (nc < 1 || nc > (1 << 30) || !packet_bank_ok(hlen)) return 0;
    if (levels < 1) levels = 1;
    const int q = nc / (hlen - 1);
    int lmax = q >= 1 ? packet_ilog2(q) : 0;
    if (lmax > kWp1MaxLev) lmax = kWp1MaxLev;
    if (levels > lmax) levels = lmax;
    if (n)
        for (int l = 0; l <= levels; l++) n[l] = nc, nc = wp1_div2(nc);
    return levels;
}
// a transform of exactly `levels` depths of rows of nc samples exists
static bool wp1_depth_ok(int nc, int hlen, int levels) { return levels >= 1 && levels <= kWp1MaxLev && wp1_geometry(nc, hlen, levels, nullptr) == levels; }
static bool wp1_batch_ok(long long nr, long long nc) { return nr >= 1 && nc >= 1 && (unsigned long long)nr * (unsigned long long)nc < (1ull << 31); }
// one depth of a batch: 2^l * n_l may exceed Nc by up to 2^l - 1 samples per row (ceil-half)
static bool wp1_level_ok(long long nr, long long nnodes, long long n) { return nr >= 1 && (unsigned long long)nr * (unsigned long long)(nnodes * n) < (1ull << 32); }

struct Wp1Plan {
    bool fused;
    int R_fwd, R_inv;
    size_t region_fwd, region_inv;  // elements of the dynamic LDS of ONE row
};
static Wp1Plan wp1_plan(int nc, int hlen, int L, size_t elem)
{
    int n[kWp1MaxLev + 1];
    n[0] = nc;
    for (int l = 1; l <= L; l++) n[l] = wp1_div2(n[l - 1]);
    auto fline = [&](int l) { return ((size_t)1 << l) * wp1_fseg(n[l], hlen); };  // depths 0 .. L - 1 pass through LDS
    auto iline = [&](int l) { return ((size_t)1 << l) * wp1_iseg(n[l], hlen); };  // depths 1 .. L
    size_t fwd = fline(0), inv = iline(L);
    for (int l = 0; l + 1 <= L - 1; l++) fwd = std::max(fwd, fline(l) + fline(l + 1));
    for (int l = 1; l + 1 <= L; l++) inv = std::max(inv, iline(l) + iline(l + 1));
    fwd = (fwd + 3) & ~(size_t)3, inv = (inv + 3) & ~(size_t)3;  // (a multiple of 16 bytes in either precision)
    Wp1Plan p{std::max(fwd, inv) * elem <= kLdsMax, 1, 1, fwd, inv};
    if (!p.fused) return p;
    const int n1 = wp1_div2(nc);
    auto pack = [&](size_t row) {
        int R = 1;
        while (R < 64 && R * n1 < kWp1Threads && 2 * R * row * elem <= kWp1PackLds) R *= 2;
        return R;
    };
    p.R_fwd = pack(fwd), p.R_inv = pack(inv);
    return p;
}

template <typename T>
static bool wp1_fill_levels(Wp1Levels<T>& lv, T* const* nodes, int nc, int L)
{
    if (!nodes) return false;
    lv.L = L, lv.n[0] = nc, lv.p[0] = nullptr;
    for (int l = 1; l <= kWp1MaxLev; l++) lv.p[l] = nullptr, lv.n[l] = 0;
    for (int l = 1; l <= L; l++) {
        if (!nodes[l - 1]) return false;
        lv.p[l] = nodes[l - 1], lv.n[l] = wp1_div2(lv.n[l - 1]);
    }
    return true;
}

// ---- drivers ------------------------------------------------------------------------------------------------------------------------
template <typename T>
static int wp1_forward_level(const T* par, T* child, int nr, int nnodes, int n, const typename FiltersOf<T>::type* f)
{
    if (!par || !child || !f || !packet_bank_ok(f->hlen) || nnodes < 1 || nnodes > (1 << kWp1MaxLev) || n < 1) return PDWT_EINVAL;
    const int N = wp1_div2(n), tiles = idiv_up(N, kWp1Tile);
    if (!wp1_level_ok(nr, nnodes, n) || (unsigned long long)nr * nnodes * tiles >= (1ull << 31)) return PDWT_EINVAL;
    const size_t lds = sizeof(T) * (2 * kWp1Tile + PDWT_MAX_FILTER_WIDTH);
    hipLaunchKernelGGL((k_wp1_fwd<T>), dim3((unsigned)nr * (unsigned)nnodes * (unsigned)tiles), dim3(kWp1Threads), lds, stream(), par, child, n, N, tiles, f->hlen, taps_fwd<T>(f));
    PDWT_HIP_TRY(hipGetLastError());
    return PDWT_OK;
}

template <typename T>
static int wp1_inverse_level(T* par, const T* child, int nr, int nnodes, int n, const int* d_list, int count, const unsigned char* d_state,
                             const typename FiltersOf<T>::type* f)
{
    if (!par || !child || !f || !packet_bank_ok(f->hlen) || nnodes < 1 || nnodes > (1 << kWp1MaxLev) || n < 1) return PDWT_EINVAL;
    if (!d_list) count = nnodes;
    if (count < 1 || count > nnodes) return PDWT_EINVAL;
    const int N = wp1_div2(n), tiles = idiv_up(wp1_pairs(n, f->hlen), kWp1Tile);
    if (!wp1_level_ok(nr, nnodes, n) || (unsigned long long)nr * count * tiles >= (1ull << 31)) return PDWT_EINVAL;
    const size_t lds = sizeof(T) * 2 * (kWp1Tile + PDWT_MAX_FILTER_WIDTH / 2);
    hipLaunchKernelGGL((k_wp1_inv<T>), dim3((unsigned)nr * (unsigned)count * (unsigned)tiles), dim3(kWp1Threads), lds, stream(), par, child, n, N, nnodes, d_list, count, d_state,
                       tiles, f->hlen, taps_inv<T>(f));
    PDWT_HIP_TRY(hipGetLastError());
    return PDWT_OK;
}

template <typename T, int HL>
static int launch_wp1_fwd_fused(const T* src, const Wp1Levels<T>& lv, int nr, const Wp1Plan& p, const Taps2<T>& taps)
{
    const size_t lds = (size_t)p.R_fwd * p.region_fwd * sizeof(T);
    const int rc = launch_lds(k_wp1_fwd_fused<T, HL>, dim3(idiv_up(nr, p.R_fwd)), dim3(kWp1Threads), lds, src, lv, nr, p.R_fwd, (int)(p.R_fwd * p.region_fwd), taps);
    return rc == PDWT_OK ? PDWT_WP1_FUSED : rc;
}
template <typename T, int HL>
static int launch_wp1_inv_fused(T* dst, const Wp1Levels<T>& lv, const unsigned char* d_state, int nr, const Wp1Plan& p, const Taps2<T>& taps)
{
    const size_t lds = (size_t)p.R_inv * p.region_inv * sizeof(T);
    const int rc = launch_lds(k_wp1_inv_fused<T, HL>, dim3(idiv_up(nr, p.R_inv)), dim3(kWp1Threads), lds, dst, lv, d_state, nr, p.R_inv, (int)(p.R_inv * p.region_inv), taps);
    return rc == PDWT_OK ? PDWT_WP1_FUSED : rc;
}

template <typename T>
static int wp1_forward(const T* src, T* const* nodes, int nr, int nc, int levels, const typename FiltersOf<T>::type* f)
{
    Wp1Levels<T> lv;
    if (!src || !f || !wp1_batch_ok(nr, nc) || !wp1_depth_ok(nc, f->hlen, levels) || !wp1_fill_levels(lv, nodes, nc, levels)) return PDWT_EINVAL;
    const Wp1Plan p = wp1_plan(nc, f->hlen, levels, sizeof(T));
    if (p.fused) {
        const Taps2<T> taps = taps_fwd<T>(f);
        return with_filter_length<2>(f->hlen, [&](auto hl) { return launch_wp1_fwd_fused<T, decltype(hl)::value>(src, lv, nr, p, taps); });
    }
    for (int l = 0; l < levels; l++)
        if (const int rc = wp1_forward_level<T>(l == 0 ? src : lv.p[l], lv.p[l + 1], nr, 1 << l, lv.n[l], f); rc != PDWT_OK) return rc;
    return PDWT_WP1_LEVELS;
}

// d_state: the DEVICE copy of a pdwt_wp1_state_table; the per-level path runs every depth under it (parents that are not SYNTH are skipped)
template <typename T>
static int wp1_inverse(T* dst, T* const* nodes, int nr, int nc, int levels, const unsigned char* d_state, const typename FiltersOf<T>::type* f)
{
    Wp1Levels<T> lv;
    if (!dst || !d_state || !f || !wp1_batch_ok(nr, nc) || !wp1_depth_ok(nc, f->hlen, levels) || !wp1_fill_levels(lv, nodes, nc, levels)) return PDWT_EINVAL;
    const Wp1Plan p = wp1_plan(nc, f->hlen, levels, sizeof(T));
    if (p.fused) {
        const Taps2<T> taps = taps_inv<T>(f);
        return with_filter_length<2>(f->hlen, [&](auto hl) { return launch_wp1_inv_fused<T, decltype(hl)::value>(dst, lv, d_state, nr, p, taps); });
    }
    for (int l = levels - 1; l >= 0; l--)
        if (const int rc = wp1_inverse_level<T>(l == 0 ? dst : lv.p[l], lv.p[l + 1], nr, 1 << l, lv.n[l], nullptr, 0, d_state + ((1 << l) - 1), f); rc != PDWT_OK) return rc;
    return PDWT_WP1_LEVELS;
}

template <typename T>
static int wp1_moments(const T* x, long long nseg, int n, double* out)
{
    if (!x || !out || nseg < 1 || n < 1 || (unsigned long long)nseg * (unsigned long long)n >= (1ull << 32)) return PDWT_EINVAL;
    int G = 1;
    while (G < 64 && G * 4 < n) G *= 2;
    const long long blocks = (nseg + kWp1Threads / G - 1) / (kWp1Threads / G);
    if (blocks >= (1ll << 31)) return PDWT_EINVAL;
    const size_t nb = 4 * (size_t)nseg * sizeof(double);
    double* d_out = (double*)pdwt_malloc(nb);
    if (!d_out) return PDWT_ENOMEM;
    hipLaunchKernelGGL((k_wp1_moments<T>), dim3((unsigned)blocks), dim3(kWp1Threads), 0, stream(), x, nseg, n, G, d_out);
    int rc = hipGetLastError() == hipSuccess ? PDWT_OK : PDWT_EHIP;
    if (rc == PDWT_OK) rc = pdwt_memcpy_d2h(out, d_out, nb);  // (synchronises)
    const int rf = pdwt_free(d_out);
    return rc != PDWT_OK ? rc : rf;
}

template <typename T>
static int wp1_thresh(int op, T* x, int nr, int nnodes, int n, const unsigned char* d_flags, T beta)
{
    if (!x || !d_flags || (op != 0 && op != 1) || nnodes < 1 || nnodes > (1 << kWp1MaxLev) || n < 1 || nr < 1) return PDWT_EINVAL;
    const unsigned long long total = (unsigned long long)nr * nnodes * n;
    if (total >= (1ull << 32)) return PDWT_EINVAL;
    const unsigned long long want = (total + kWp1Threads - 1) / kWp1Threads;
    const unsigned blocks = (unsigned)std::min<unsigned long long>(want, 256 * 32);
    hipLaunchKernelGGL((k_wp1_thresh<T>), dim3(blocks), dim3(kWp1Threads), 0, stream(), x, total, (unsigned)n, (unsigned)nnodes, d_flags, op, beta);
    PDWT_HIP_TRY(hipGetLastError());
    return PDWT_OK;
}

}  // namespace pdwt

using namespace pdwt;

extern "C" {
int pdwt_wp1_geometry(int Nc, int hlen, int levels, int* n) { return wp1_geometry(Nc, hlen, levels, n); }
int pdwt_wp1_fused(int Nc, int hlen, int levels, int elem_size)
{
    const int L = wp1_geometry(Nc, hlen, levels, nullptr);
    if (L < 1 || (elem_size != 4 && elem_size != 8)) return PDWT_EINVAL;
    return wp1_plan(Nc, hlen, L, (size_t)elem_size).fused ? 1 : 0;
}
long long pdwt_wp1_tmp_elems(int Nr, int Nc, int hlen, int levels, int elem_size)
{
    if (pdwt_wp1_fused(Nc, hlen, levels, elem_size) < 0 || !wp1_batch_ok(Nr, Nc)) return PDWT_EINVAL;
    return 0;  // every intermediate lives in LDS (fused) or in the allocation of its own depth (per level)
}
int pdwt_wp1_frequency_order(int depth, int* out)
{
    if (depth < 0 || depth > kWp1MaxLev || !out) return PDWT_EINVAL;
    for (int r = 0; r < (1 << depth); r++) out[r] = r ^ (r >> 1);
    return PDWT_OK;
}
int pdwt_wp1_state_table(int levels, const int* depth, const int* idx, int n, unsigned char* out)
{
    const int rc = packet_state_table<2>(levels, kWp1MaxLev, depth, idx, n, out);
    if (rc == PDWT_OK) out[(2 << levels) - 1] = 0;  // (the table is 2^(levels + 1) bytes)
    return rc;
}
int pdwt_memcpy2d(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t height, int kind)
{
    if (!dst || !src || width > dpitch || width > spitch || kind < 0 || kind > 3) return PDWT_EINVAL;
    if (!width || !height) return PDWT_OK;
    if (kind == 3) PDWT_HIP_TRY(hipStreamSynchronize(nullptr));  // a foreign producer, as pdwt_memcpy_d2d_foreign
    const hipMemcpyKind k = kind == 0 ? hipMemcpyHostToDevice : kind == 1 ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    PDWT_HIP_TRY(hipMemcpy2DAsync(dst, dpitch, src, spitch, width, height, k, stream()));
    if (kind != 2) PDWT_HIP_TRY(hipStreamSynchronize(stream()));
    return PDWT_OK;
}

#define PDWT_WP1_ENTRIES(SFX, T, FT)                                                                                                                      \
    int pdwt_wp1_forward_level_##SFX(const T* d_parent, T* d_child, int nr, int nnodes, int n, const FT* f)                                               \
    {                                                                                                                                                     \
        return wp1_forward_level<T>(d_parent, d_child, nr, nnodes, n, f);                                                                                 \
    }                                                                                                                                                     \
    int pdwt_wp1_inverse_level_##SFX(T* d_parent, const T* d_child, int nr, int nnodes, int n, const int* d_list, int count, const FT* f)                 \
    {                                                                                                                                                     \
        return wp1_inverse_level<T>(d_parent, d_child, nr, nnodes, n, d_list, count, nullptr, f);                                                         \
    }                                                                                                                                                     \
    int pdwt_wp1_forward_##SFX(const T* d_src, T* const* d_nodes, int nr, int nc, int levels, const FT* f)                                                \
    {                                                                                                                                                     \
        return wp1_forward<T>(d_src, d_nodes, nr, nc, levels, f);                                                                                         \
    }                                                                                                                                                     \
    int pdwt_wp1_inverse_##SFX(T* d_dst, T* const* d_nodes, int nr, int nc, int levels, const unsigned char* d_state, const FT* f)                        \
    {                                                                                                                                                     \
        return wp1_inverse<T>(d_dst, d_nodes, nr, nc, levels, d_state, f);                                                                                \
    }                                                                                                                                                     \
    int pdwt_wp1_moments_##SFX(const T* d_level, long long nseg, int n, double* out) { return wp1_moments<T>(d_level, nseg, n, out); }                    \
    int pdwt_wp1_thresh_##SFX(int op, T* d_level, int nr, int nnodes, int n, const unsigned char* d_flags, T beta)                                        \
    {                                                                                                                                                     \
        return wp1_thresh<T>(op, d_level, nr, nnodes, n, d_flags, beta);                                                                                  \
    }
PDWT_WP1_ENTRIES(f32, float, pdwt_filters_f32)
PDWT_WP1_ENTRIES(f64, double, pdwt_filters_f64)
#undef PDWT_WP1_ENTRIES
}
