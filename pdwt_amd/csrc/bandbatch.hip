// bandbatch.hip -- the band statistics and per-band thresholds of bandstats.hip over a REGULAR BATCH: B images with the same nb
// bands, band k of n[k] elements in every image, the pointer of band k of image b at tab[b * nb + k] of a table in DEVICE memory
// (WaveletsImages builds it once).  What it replaces is `for b: img[b]->denoise()`: B times (moments launch, 3..6 histogram + pick
// launches, threshold launch, blocking copy).  Here the number of launches and of copies to the host is fixed per group of images
// (the one exception: medians of large bands run in rounds of kRoundSlots pairs).
//
// MI355X design
//   Descriptor: the band sizes, the block layout of one image and the lists of asking bands go to device memory in one small
//     copy per call (BatchDesc, ~2 KB).  It goes through a pinned staging buffer, so the caller's host arrays are consumed
//     before an entry returns.  The kernels take pointers and scalars only -- nothing that grows with B or nb is a kernel
//     argument.  grid.y is the image, grid.x walks the block layout of one image.
//   Moments (k_bb_moments + k_bb_combine): the accumulation of k_band_moments (per-lane doubles, wave64 shuffles, LDS across the
//     waves), three doubles per block; a second, tiny launch adds the partials of every (image, band) in a fixed order, one wave per
//     pair.  No float atomics and no arrival order: two runs give the same bits.
//   Selection, small bands (k_bb_select_wg): batch bands are small (the finest band of a 512 x 512 image has 64 K elements), so ONE
//     workgroup of 1024 threads per asking (image, band) runs EVERY radix pass itself: 2 x 2048-bin LDS histograms, a workgroup
//     scan, the next prefix, the band re-read from L2.  One launch whatever the dtype, no global histograms, no pick launches.
//   Selection, large bands (k_bb_hist + k_bb_pick): a band of more than kWgMaxElems elements is split over several workgroups per
//     pass as in k_band_hist (LDS histogram, 64-bit integer adds into the pair's global histogram), in rounds of kRoundSlots
//     (image, band) pairs: the selection scratch (2 MB of histograms) does not grow with B.
//   Contention: the wave-aggregated LDS adds of bandstats.hip (mostly-zero bands), in both selection kernels.
//   Thresholds (k_bb_thresh): the operators of utils.hip, beta[b * nb + k] read from device memory; beta < 0: the block returns.
//   Groups: one group is at most kGroupSlots (image, band) pairs (8192: 819 images of 10 bands); a larger batch is processed group
//     after group, each with its own copy to the host.  All scratch is sized by the group, not by B.
#include <math.h>
#include <string.h>

#include <mutex>
#include <vector>

#include "common.hpp"
#include "bandlist.hpp"

namespace pdwt {
namespace {

constexpr int kBThreads = 256;
constexpr int kBChunk = kBThreads * 16;   // elements per block-iteration, as in bandstats.hip
constexpr int kBMaxBands = 3 * 32 + 1;
constexpr int kGroupSlots = 8192;         // (image, band) pairs of one group
constexpr int kBlockBudget = 4096;        // blocks of a moments / threshold launch over a group, + one per pair at most
constexpr int kPartBlocks = kBlockBudget + kGroupSlots;
constexpr int kWgThreads = 1024;          // the one-workgroup selection
constexpr unsigned long long kWgMaxElems = 1ull << 19;  // ... takes bands up to this size (2 MB of float: re-read from L2)
constexpr int kRoundSlots = 64;           // large asking (image, band) pairs per round of hist + pick launches
constexpr int kHistBudget = 2048;         // blocks of one histogram pass over a round
constexpr int kHistMinChunks = 4;
constexpr int kBins = 2048;               // 11 bits per pass
constexpr int kDigitBits = 11;

struct BatchDesc {
    unsigned long long n[kBMaxBands];
    unsigned int blk0[kBMaxBands + 1];    // first block of band k in the block row of one image; [nb] = grid.x
    unsigned int per;                     // chunks per block
    int nb;
    int nwg, nbig;
    unsigned short wg_band[kBMaxBands];   // asking bands selected by one workgroup
    unsigned short big_band[kBMaxBands];  // asking bands selected in rounds
};

// one result record per (image, band): the size of pdwt_band_stats, converted in place on the host
struct Record {
    double sum_abs, sum_sq, max_abs;
    unsigned long long key[2];
};
static_assert(sizeof(Record) == sizeof(BandStats), "a record is converted to BandStats in place");

struct SelState {
    unsigned long long prefix[2];
    unsigned long long rank[2];
};

__device__ __forceinline__ unsigned int key_of(float x) { return __float_as_uint(x) & 0x7fffffffu; }
__device__ __forceinline__ unsigned long long key_of(double x) { return (unsigned long long)__double_as_longlong(x) & 0x7fffffffffffffffull; }

__device__ __forceinline__ int band_of_block(const unsigned int* __restrict__ blk0, int nb, unsigned int b)
{
    int k = 0;
    while (k + 1 < nb && b >= blk0[k + 1]) k++;
    return k;
}

// f(x) for every element of the chunks [lo, hi) of a band, walked from the end (what the transform that wrote the band front to
// back left in the cache).  A full chunk of a 16-byte aligned band: every load in flight before the first use.
template <typename T, bool NT, typename F>
__device__ __forceinline__ void walk_chunks(const T* __restrict__ p, unsigned long long n, unsigned long long lo, unsigned long long hi, F&& f)
{
    constexpr int NV = 16 / (int)sizeof(T);
    constexpr int U = kBChunk / (kBThreads * NV);
    typedef T NTV __attribute__((ext_vector_type(NV)));
    const bool vec = ((uintptr_t)p & 15) == 0;
    for (unsigned long long cc = hi; cc > lo; cc--) {
        const unsigned long long base = (cc - 1) * kBChunk;
        if (vec && base + kBChunk <= n) {
            NTV v[U];
#pragma unroll
            for (int u = 0; u < U; u++) {
                const NTV* q = reinterpret_cast<const NTV*>(p + base + ((unsigned long long)u * kBThreads + threadIdx.x) * NV);
                v[u] = NT ? __builtin_nontemporal_load(q) : *q;
            }
#pragma unroll
            for (int u = 0; u < U; u++) {
#pragma unroll
                for (int q = 0; q < NV; q++) f(v[u][q]);
            }
        } else {
            for (int u = 0; u < kBChunk / kBThreads; u++) {
                const unsigned long long i = base + (unsigned long long)u * kBThreads + threadIdx.x;
                if (i < n) f(p[i]);
            }
        }
    }
}

__device__ __forceinline__ double wsum(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}
__device__ __forceinline__ double wmax(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double o = __shfl_down(v, off, 64);
        v = o > v ? o : v;
    }
    return v;
}

// block (x, img): the chunks [j * per, (j + 1) * per) of band k of image img -> part[3 * (img * gridDim.x + x)]
template <typename T>
__global__ __launch_bounds__(kBThreads) void k_bb_moments(const T* const* __restrict__ tab, const BatchDesc* __restrict__ d, double* __restrict__ part)
{
    __shared__ double s_w[3][kBThreads / 64];
    const int nb = d->nb;
    const int k = band_of_block(d->blk0, nb, blockIdx.x);
    const T* p = tab[(size_t)blockIdx.y * nb + k];
    const unsigned long long n = d->n[k], nch = (n + kBChunk - 1) / kBChunk;
    const unsigned long long lo = (unsigned long long)(blockIdx.x - d->blk0[k]) * d->per;
    unsigned long long hi = lo + d->per;
    if (hi > nch) hi = nch;
    double sa = 0.0, sq = 0.0;
    T mx = T(0);
    walk_chunks<T, true>(p, n, lo, hi, [&](T x) {
        const T a = x < T(0) ? -x : x;
        const double v = (double)a;
        sa += v;
        sq = fma(v, v, sq);
        mx = a > mx ? a : mx;
    });
    sa = wsum(sa);
    sq = wsum(sq);
    const double dm = wmax((double)mx);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        s_w[0][wave] = sa;
        s_w[1][wave] = sq;
        s_w[2][wave] = dm;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double* o = part + 3 * ((size_t)blockIdx.y * gridDim.x + blockIdx.x);
        const double m01 = s_w[2][0] > s_w[2][1] ? s_w[2][0] : s_w[2][1], m23 = s_w[2][2] > s_w[2][3] ? s_w[2][2] : s_w[2][3];
        o[0] = (s_w[0][0] + s_w[0][1]) + (s_w[0][2] + s_w[0][3]);
        o[1] = (s_w[1][0] + s_w[1][1]) + (s_w[1][2] + s_w[1][3]);
        o[2] = m01 > m23 ? m01 : m23;
    }
}

// one wave per (image, band): lanes strided over the pair's blocks, then the shuffle tree -- a fixed order.  nrow = blocks per image.
__global__ __launch_bounds__(kBThreads) void k_bb_combine(const BatchDesc* __restrict__ d, const double* __restrict__ part, Record* __restrict__ out,
                                                           unsigned int nrow, unsigned int nslots)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned int slot = blockIdx.x * (kBThreads / 64) + wave;
    if (slot >= nslots) return;
    const unsigned int nb = (unsigned int)d->nb, img = slot / nb, k = slot % nb;
    double a = 0.0, q = 0.0, m = 0.0;
    for (unsigned int i = d->blk0[k] + lane; i < d->blk0[k + 1]; i += 64) {
        const double* s = part + 3 * ((size_t)img * nrow + i);
        a += s[0];
        q += s[1];
        m = s[2] > m ? s[2] : m;
    }
    a = wsum(a);
    q = wsum(q);
    m = wmax(m);
    if (lane == 0) {
        out[slot].sum_abs = a;
        out[slot].sum_sq = q;
        out[slot].max_abs = m;
    }
}

// one counting lane group -> LDS: `m` = this lane counts, `b` = its bin.  Two rounds of wave aggregation (bandstats.hip), the rest lane by lane.
__device__ __forceinline__ void hist_add(unsigned int* s_hist, bool m, unsigned int b)
{
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int round = 0; round < 2; round++) {
        if (m) {  // (inside the branch only the counting lanes are active: the first of them gives the bin, the ballot counts them alone)
            const unsigned int first = (unsigned int)__builtin_amdgcn_readfirstlane((int)b);
            const bool same = b == first;
            const unsigned long long smask = __ballot(same);
            if (lane == __ffsll((long long)smask) - 1) atomicAdd(&s_hist[first], (unsigned int)__popcll(smask));
            m = !same;
        }
    }
    if (m) atomicAdd(&s_hist[b], 1u);
}

// exclusive prefix of `own` over the workgroup, in thread order; s_wt: one word per wave
__device__ __forceinline__ unsigned int wg_excl_scan(unsigned int own, unsigned int* s_wt)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned int inc = own;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned int t = __shfl_up(inc, off, 64);
        if (lane >= off) inc += t;
    }
    if (lane == 63) s_wt[wave] = inc;
    __syncthreads();
    unsigned int base = 0;
    for (int j = 0; j < wave; j++) base += s_wt[j];
    __syncthreads();  // (s_wt may be written again)
    return base + inc - own;
}

// workgroup (x, img): the two middle order statistics of |band wg_band[x]| of image img, every radix pass in this launch.
// The two ranks share one prefix and one histogram until they part; from then on the second histogram is filled as well.
template <typename T>
__global__ __launch_bounds__(kWgThreads) void k_bb_select_wg(const T* const* __restrict__ tab, const BatchDesc* __restrict__ d, Record* __restrict__ out)
{
    using K = decltype(key_of(T(0)));
    constexpr int KEYBITS = (int)sizeof(T) * 8;
    constexpr int NV = 16 / (int)sizeof(T);
    constexpr int U = 4;
    constexpr unsigned int TILE = kWgThreads * NV * U;
    typedef T NTV __attribute__((ext_vector_type(NV)));
    __shared__ unsigned int s_hist[2][kBins];
    __shared__ unsigned int s_wt[kWgThreads / 64];
    __shared__ unsigned long long s_pref[2];
    __shared__ unsigned int s_rank[2];
    const int nb = d->nb, k = d->wg_band[blockIdx.x];
    const size_t slot = (size_t)blockIdx.y * nb + k;
    const T* __restrict__ p = tab[slot];
    const unsigned int n = (unsigned int)d->n[k];  // (<= kWgMaxElems)
    const bool vec = ((uintptr_t)p & 15) == 0;
    K p0 = 0, p1 = 0;
    unsigned int r0 = (n - 1) / 2, r1 = n / 2;
    for (int hs = KEYBITS; hs > 0; hs -= kDigitBits) {
        const int shift = hs - kDigitBits > 0 ? hs - kDigitBits : 0, width = hs - shift;
        const int hsh = hs < KEYBITS ? hs : KEYBITS - 1;  // (first pass: the sign bit of a key is 0 = the empty prefix)
        const unsigned int dmask = (1u << width) - 1u;
        const bool two = p0 != p1;
        for (int i = threadIdx.x; i < 2 * kBins; i += kWgThreads) (&s_hist[0][0])[i] = 0u;
        __syncthreads();
        auto count = [&](T x) {
            const K key = key_of(x);
            const unsigned int b = (unsigned int)(key >> shift) & dmask;
            const K hi = key >> hsh;
            hist_add(s_hist[0], hi == p0, b);
            if (two) hist_add(s_hist[1], hi == p1, b);
        };
        unsigned int i0 = 0;
        if (vec) {
            for (; i0 + TILE <= n; i0 += TILE) {
                NTV v[U];
#pragma unroll
                for (int u = 0; u < U; u++) v[u] = *reinterpret_cast<const NTV*>(p + i0 + ((unsigned int)u * kWgThreads + threadIdx.x) * NV);
#pragma unroll
                for (int u = 0; u < U; u++) {
#pragma unroll
                    for (int q = 0; q < NV; q++) count(v[u][q]);
                }
            }
        }
        for (unsigned int i = i0 + threadIdx.x; i < n; i += kWgThreads) count(p[i]);
        __syncthreads();
#pragma unroll
        for (int w = 0; w < 2; w++) {
            const unsigned int* h = s_hist[(w == 1 && two) ? 1 : 0];
            const unsigned int c0 = h[2 * threadIdx.x], c1 = h[2 * threadIdx.x + 1], own = c0 + c1;
            const unsigned int before = wg_excl_scan(own, s_wt);
            const unsigned int rank = w ? r1 : r0;
            if (before <= rank && rank < before + own) {  // exactly one thread: the counts of a prefix add up to more than its rank
                const bool second = rank >= before + c0;
                s_pref[w] = ((unsigned long long)(w ? p1 : p0) << width) | (unsigned long long)(2 * threadIdx.x + (second ? 1 : 0));
                s_rank[w] = rank - before - (second ? c0 : 0u);
            }
        }
        __syncthreads();
        p0 = (K)s_pref[0];
        p1 = (K)s_pref[1];
        r0 = s_rank[0];
        r1 = s_rank[1];
        __syncthreads();  // (read before the next pass writes them; every read of the histograms is done as well)
    }
    if (threadIdx.x == 0) {
        out[slot].key[0] = (unsigned long long)p0;
        out[slot].key[1] = (unsigned long long)p1;
    }
}

// one pass of the selection over a round of large asking pairs: block (x, y) counts the chunks [x * per, (x + 1) * per) of pair
// pair0 + y into hist[y][which][bin].  first: no prefix yet.
template <typename T>
__global__ __launch_bounds__(kBThreads) void k_bb_hist(const T* const* __restrict__ tab, const BatchDesc* __restrict__ d, const SelState* __restrict__ st,
                                                       unsigned long long* __restrict__ hist, unsigned int pair0, unsigned int per, int first, int shift,
                                                       int hsh, unsigned int dmask)
{
    using K = decltype(key_of(T(0)));
    __shared__ unsigned int s_hist[2][kBins];
    const unsigned int pair = pair0 + blockIdx.y, nbig = (unsigned int)d->nbig;
    const int k = d->big_band[pair % nbig];
    const unsigned long long n = d->n[k], nch = (n + kBChunk - 1) / kBChunk;
    const unsigned long long lo = (unsigned long long)blockIdx.x * per;
    if (lo >= nch) return;  // (uniform: the grid is as wide as the largest band needs)
    unsigned long long hi = lo + per;
    if (hi > nch) hi = nch;
    const T* p = tab[(size_t)(pair / nbig) * d->nb + k];
    K p0 = 0, p1 = 0;
    if (!first) {
        p0 = (K)st[blockIdx.y].prefix[0];
        p1 = (K)st[blockIdx.y].prefix[1];
    }
    const bool two = p0 != p1;
    for (int i = threadIdx.x; i < 2 * kBins; i += kBThreads) (&s_hist[0][0])[i] = 0u;
    __syncthreads();
    walk_chunks<T, false>(p, n, lo, hi, [&](T x) {
        const K key = key_of(x);
        const unsigned int b = (unsigned int)(key >> shift) & dmask;
        const K h = key >> hsh;
        hist_add(s_hist[0], h == p0, b);
        if (two) hist_add(s_hist[1], h == p1, b);
    });
    __syncthreads();
    unsigned long long* g = hist + (size_t)blockIdx.y * 2 * kBins;
    for (int i = threadIdx.x; i < (two ? 2 : 1) * kBins; i += kBThreads) {
        const unsigned int c = (&s_hist[0][0])[i];
        if (c) atomicAdd(g + i, (unsigned long long)c);  // (integer adds commute: the counts do not depend on arrival order)
    }
}

// one workgroup per pair of the round: find the bin that holds each rank, extend the prefix, reduce the rank, clear the histograms;
// after the last pass the two keys go to the pair's record
__global__ __launch_bounds__(kBThreads) void k_bb_pick(const BatchDesc* __restrict__ d, SelState* __restrict__ st, unsigned long long* __restrict__ hist,
                                                       Record* __restrict__ out, unsigned int pair0, int first, int last, int width)
{
    __shared__ unsigned long long s_sum[kBThreads];
    constexpr int PER = kBins / kBThreads;  // 8 consecutive bins per thread
    const unsigned int pair = pair0 + blockIdx.x, nbig = (unsigned int)d->nbig;
    const int k = d->big_band[pair % nbig];
    SelState s;
    if (first) {
        const unsigned long long n = d->n[k];
        s.prefix[0] = s.prefix[1] = 0;
        s.rank[0] = (n - 1) / 2;
        s.rank[1] = n / 2;
    } else {
        s = st[blockIdx.x];
    }
    const bool two = s.prefix[0] != s.prefix[1];
    unsigned long long* g = hist + (size_t)blockIdx.x * 2 * kBins;
    for (int w = 0; w < 2; w++) {
        const unsigned long long* h = g + ((w == 1 && two) ? kBins : 0);
        unsigned long long c[PER], own = 0;
#pragma unroll
        for (int i = 0; i < PER; i++) {
            c[i] = h[threadIdx.x * PER + i];
            own += c[i];
        }
        __syncthreads();  // (s_sum of the previous round has been read)
        s_sum[threadIdx.x] = own;
        __syncthreads();
        unsigned long long before = 0;
        for (int j = 0; j < (int)threadIdx.x; j++) before += s_sum[j];
        const unsigned long long rank = s.rank[w];
        if (before <= rank && rank < before + own) {  // exactly one thread
            unsigned long long acc = before, np = 0, nr = 0;
#pragma unroll
            for (int i = 0; i < PER; i++) {
                if (acc <= rank && rank < acc + c[i]) {
                    np = (s.prefix[w] << width) | (unsigned long long)(threadIdx.x * PER + i);
                    nr = rank - acc;
                }
                acc += c[i];
            }
            st[blockIdx.x].prefix[w] = np;
            st[blockIdx.x].rank[w] = nr;
            if (last) out[(size_t)(pair / nbig) * d->nb + k].key[w] = np;
        }
    }
    __syncthreads();  // every read of the histograms is done
    for (int i = threadIdx.x; i < 2 * kBins; i += kBThreads) g[i] = 0ull;
}

__device__ __forceinline__ float copysign_t(float a, float s) { return copysignf(a, s); }
__device__ __forceinline__ double copysign_t(double a, double s) { return copysign(a, s); }
// the operators of utils.hip (ew_op): soft = copysign(max(|x| - b, 0), x); hard = x if |x| - b > 0, else 0 * x
template <int OP, typename T>
__device__ __forceinline__ T thresh_op(T x, T b)
{
    if constexpr (OP == BL_SOFT) {
        const T m = (T)fabs(x) - b;
        return copysign_t(m > T(0) ? m : T(0), x);
    } else {
        return ((T)fabs(x) - b > T(0) ? T(1) : T(0)) * x;
    }
}

// block (x, img): its run of chunks of band k of image img, in place; beta[img * nb + k] < 0: nothing
template <typename T, int OP>
__global__ __launch_bounds__(kBThreads) void k_bb_thresh(T* const* __restrict__ tab, const BatchDesc* __restrict__ d, const T* __restrict__ beta)
{
    constexpr int NV = 16 / (int)sizeof(T);
    constexpr int U = kBChunk / (kBThreads * NV);
    typedef T NTV __attribute__((ext_vector_type(NV)));
    const int nb = d->nb;
    const int k = band_of_block(d->blk0, nb, blockIdx.x);
    const size_t slot = (size_t)blockIdx.y * nb + k;
    const T b = beta[slot];
    if (b < T(0)) return;
    T* p = tab[slot];
    const unsigned long long n = d->n[k], nch = (n + kBChunk - 1) / kBChunk;
    const unsigned long long lo = (unsigned long long)(blockIdx.x - d->blk0[k]) * d->per;
    unsigned long long hi = lo + d->per;
    if (hi > nch) hi = nch;
    const bool vec = ((uintptr_t)p & 15) == 0;
    for (unsigned long long cc = lo; cc < hi; cc++) {
        const unsigned long long base = cc * kBChunk;
        if (vec && base + kBChunk <= n) {
            NTV v[U];
#pragma unroll
            for (int u = 0; u < U; u++) v[u] = *reinterpret_cast<const NTV*>(p + base + ((unsigned long long)u * kBThreads + threadIdx.x) * NV);
#pragma unroll
            for (int u = 0; u < U; u++) {
#pragma unroll
                for (int q = 0; q < NV; q++) v[u][q] = thresh_op<OP, T>(v[u][q], b);
                *reinterpret_cast<NTV*>(p + base + ((unsigned long long)u * kBThreads + threadIdx.x) * NV) = v[u];
            }
        } else {
            for (int u = 0; u < kBChunk / kBThreads; u++) {
                const unsigned long long i = base + (unsigned long long)u * kBThreads + threadIdx.x;
                if (i < n) p[i] = thresh_op<OP, T>(p[i], b);
            }
        }
    }
}

#define PDWT_CHECK_LAUNCH() PDWT_HIP_TRY(hipGetLastError())

// per-device scratch of the batch entries, allocated on first use; every size is fixed (it depends on the group, not on B).
// It is separate from the scratch of bandstats.hip: the single-image path is not touched.
constexpr size_t kDescBytes = (sizeof(BatchDesc) + 255) & ~(size_t)255;
constexpr size_t kBetaBytes = (size_t)kGroupSlots * sizeof(double);
constexpr size_t kPartBytes = 3 * (size_t)kPartBlocks * sizeof(double);
constexpr size_t kResBytes = (size_t)kGroupSlots * sizeof(Record);
constexpr size_t kStBytes = (size_t)kRoundSlots * sizeof(SelState);
constexpr size_t kHistBytes = (size_t)kRoundSlots * 2 * kBins * sizeof(unsigned long long);  // 2 MB: the selection scratch
struct Scratch {
    BatchDesc* desc;
    void* beta;
    char* pin;           // pinned host staging of the descriptor and the betas: the caller's host arrays are consumed before an entry returns
    hipEvent_t pin_free; // recorded behind the last copy out of `pin`
    bool pin_busy;
    double* part;
    Record* res;
    SelState* st;
    unsigned long long* hist;
    void* base;
};

std::mutex g_bmu;
std::mutex g_batch_mu[64];
Scratch g_bscr[64] = {};

Scratch* scratch(int* dev_out)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
    *dev_out = dev;
    std::lock_guard<std::mutex> lk(g_bmu);
    Scratch& s = g_bscr[dev];
    if (!s.base) {
        const size_t total = kDescBytes + kBetaBytes + kPartBytes + kResBytes + kStBytes + kHistBytes;
        void* b = nullptr;
        if (hipMalloc(&b, total) != hipSuccess) return nullptr;
        // the histograms start at 0 (and k_bb_pick leaves them at 0); zeroed on the library stream
        if (hipMemsetAsync(b, 0, total, stream()) != hipSuccess) {
            (void)hipFree(b);
            return nullptr;
        }
        void* h = nullptr;
        if (hipHostMalloc(&h, kDescBytes + kBetaBytes, hipHostMallocDefault) != hipSuccess || hipEventCreateWithFlags(&s.pin_free, hipEventDisableTiming) != hipSuccess) {
            if (h) (void)hipHostFree(h);
            (void)hipFree(b);
            return nullptr;
        }
        s.pin = (char*)h;
        s.pin_busy = false;
        char* c = (char*)b;
        s.desc = (BatchDesc*)c, c += kDescBytes;
        s.beta = c, c += kBetaBytes;
        s.part = (double*)c, c += kPartBytes;
        s.res = (Record*)c, c += kResBytes;
        s.st = (SelState*)c, c += kStBytes;
        s.hist = (unsigned long long*)c;
        s.base = b;
    }
    return &s;
}

// host -> device through the pinned staging buffer (offset `off` of it), stream-ordered.  The source is read before this returns; the
// staging buffer is reused only after the copies out of it have run (an event behind them: no wait for the kernels).
int stage_h2d(Scratch* s, void* dst, const void* src, size_t nbytes, size_t off, bool first)
{
    if (first && s->pin_busy) PDWT_HIP_TRY(hipEventSynchronize(s->pin_free));
    memcpy(s->pin + off, src, nbytes);
    PDWT_HIP_TRY(hipMemcpyAsync(dst, s->pin + off, nbytes, hipMemcpyHostToDevice, stream()));
    return PDWT_OK;
}
int stage_done(Scratch* s)
{
    PDWT_HIP_TRY(hipEventRecord(s->pin_free, stream()));
    s->pin_busy = true;
    return PDWT_OK;
}

// the block layout of one image: band k gets ceil(chunks / per) blocks when take[k], per chosen so that a group of `images` stays
// within kBlockBudget + one block per pair
void layout(BatchDesc& d, const size_t* n, int nb, const bool* take, int images)
{
    unsigned long long tot = 0;
    for (int k = 0; k < nb; k++)
        if (take[k]) tot += (n[k] + kBChunk - 1) / kBChunk;
    unsigned long long per = (tot * (unsigned long long)images + kBlockBudget - 1) / kBlockBudget;
    if (per < 1) per = 1;
    d.per = (unsigned int)per;
    d.blk0[0] = 0;
    for (int k = 0; k < nb; k++) {
        const unsigned long long nch = take[k] ? (n[k] + kBChunk - 1) / kBChunk : 0;
        d.blk0[k + 1] = d.blk0[k] + (unsigned int)((nch + per - 1) / per);
    }
}

bool sizes_ok(const size_t* n, int nb)
{
    for (int k = 0; k < nb; k++)
        if ((n[k] + kBChunk - 1) / kBChunk > 0xffffffull) return false;  // (block counts of one image stay far inside 32 bits)
    return true;
}

template <typename T> double key_value(unsigned long long key);
template <> double key_value<float>(unsigned long long key)
{
    const unsigned int u = (unsigned int)key;
    float f;
    memcpy(&f, &u, sizeof(f));
    return (double)f;
}
template <> double key_value<double>(unsigned long long key)
{
    double v;
    memcpy(&v, &key, sizeof(v));
    return v;
}

template <typename T>
int band_batch_stats(const T* const* d_tab, const size_t* n, int B, int nb, const unsigned char* want_median, BandStats* out)
{
    if (!d_tab || !n || !out || B < 1 || nb < 1 || nb > kBMaxBands || !sizes_ok(n, nb)) return PDWT_EINVAL;
    constexpr int KEYBITS = (int)sizeof(T) * 8;
    const int gmax = kGroupSlots / nb, g_images = B < gmax ? B : gmax;
    BatchDesc d;
    memset(&d, 0, sizeof(d));
    d.nb = nb;
    bool take[kBMaxBands];
    bool any_moments = false;
    unsigned long long big_chunks = 0;
    for (int k = 0; k < nb; k++) {
        d.n[k] = n[k];
        const int want = want_median ? want_median[k] : 0;
        take[k] = n[k] && want != 2;
        any_moments = any_moments || take[k];
        if (want && n[k]) {
            if (n[k] <= kWgMaxElems) {
                d.wg_band[d.nwg++] = (unsigned short)k;
            } else {
                d.big_band[d.nbig++] = (unsigned short)k;
                const unsigned long long nch = (n[k] + kBChunk - 1) / kBChunk;
                big_chunks = nch > big_chunks ? nch : big_chunks;
            }
        }
    }
    layout(d, n, nb, take, g_images);
    if (any_moments || d.nwg || d.nbig) {
        int dev = 0;
        Scratch* s = scratch(&dev);
        if (!s) return PDWT_ENOMEM;
        std::lock_guard<std::mutex> lk(g_batch_mu[dev]);  // the scratch is shared by every batch on the device, until its results are out
        if (const int rc = stage_h2d(s, s->desc, &d, sizeof(d), 0, true); rc != PDWT_OK) return rc;
        if (const int rc = stage_done(s); rc != PDWT_OK) return rc;
        std::vector<Record> res((size_t)g_images * nb);
        for (int g0 = 0; g0 < B; g0 += gmax) {
            const int bg = B - g0 < gmax ? B - g0 : gmax;
            const T* const* tab = d_tab + (size_t)g0 * nb;
            const unsigned int nslots = (unsigned int)bg * nb;
            KTimer kt(K_ABS_SUM);
            if (any_moments) {
                hipLaunchKernelGGL((k_bb_moments<T>), dim3(d.blk0[nb], bg), dim3(kBThreads), 0, stream(), tab, s->desc, s->part);
                PDWT_CHECK_LAUNCH();
                hipLaunchKernelGGL(k_bb_combine, dim3((nslots + kBThreads / 64 - 1) / (kBThreads / 64)), dim3(kBThreads), 0, stream(), s->desc, s->part,
                                   s->res, d.blk0[nb], nslots);
                PDWT_CHECK_LAUNCH();
            }
            if (d.nwg) {
                hipLaunchKernelGGL((k_bb_select_wg<T>), dim3(d.nwg, bg), dim3(kWgThreads), 0, stream(), tab, s->desc, s->res);
                PDWT_CHECK_LAUNCH();
            }
            const unsigned int npairs = (unsigned int)bg * d.nbig;
            for (unsigned int pair0 = 0; pair0 < npairs; pair0 += kRoundSlots) {
                const unsigned int np = npairs - pair0 < (unsigned)kRoundSlots ? npairs - pair0 : (unsigned)kRoundSlots;
                // blocks per pair: the budget of a pass over the pairs of the round, every block at least kHistMinChunks chunks
                unsigned long long target = kHistBudget / np, per = (big_chunks + target - 1) / target;
                if (per < kHistMinChunks) per = kHistMinChunks;
                const unsigned int gx = (unsigned int)((big_chunks + per - 1) / per);
                for (int hs = KEYBITS; hs > 0; hs -= kDigitBits) {
                    const int shift = hs - kDigitBits > 0 ? hs - kDigitBits : 0, width = hs - shift;
                    const int hsh = hs < KEYBITS ? hs : KEYBITS - 1;
                    const int first = hs == KEYBITS, last = shift == 0;
                    hipLaunchKernelGGL((k_bb_hist<T>), dim3(gx, np), dim3(kBThreads), 0, stream(), tab, s->desc, s->st, s->hist, pair0, (unsigned int)per,
                                       first, shift, hsh, (1u << width) - 1u);
                    PDWT_CHECK_LAUNCH();
                    hipLaunchKernelGGL(k_bb_pick, dim3(np), dim3(kBThreads), 0, stream(), s->desc, s->st, s->hist, s->res, pair0, first, last, width);
                    PDWT_CHECK_LAUNCH();
                }
            }
            // one copy per group: the moments and the keys of every pair
            if (const int rc = pdwt_memcpy_d2h(res.data(), s->res, (size_t)nslots * sizeof(Record)); rc != PDWT_OK) return rc;
            for (unsigned int i = 0; i < nslots; i++) {
                const int k = (int)(i % (unsigned)nb);
                const int want = want_median ? want_median[k] : 0;
                const Record& r = res[i];
                BandStats& o = out[(size_t)g0 * nb + i];
                o.n = (double)n[k];
                o.sum_abs = want == 2 ? NAN : n[k] ? r.sum_abs : 0.0;
                o.sum_sq = want == 2 ? NAN : n[k] ? r.sum_sq : 0.0;
                o.max_abs = want == 2 ? NAN : n[k] ? r.max_abs : 0.0;
                o.median_abs = (want && n[k]) ? 0.5 * (key_value<T>(r.key[0]) + key_value<T>(r.key[1])) : NAN;
            }
        }
    } else {
        for (size_t i = 0; i < (size_t)B * nb; i++) {
            const int want = want_median ? want_median[i % nb] : 0;
            out[i].n = 0.0;
            out[i].sum_abs = out[i].sum_sq = out[i].max_abs = want == 2 ? NAN : 0.0;
            out[i].median_abs = NAN;
        }
    }
    return PDWT_OK;
}

template <typename T>
int band_batch_thresh(int op, T* const* d_tab, const size_t* n, const T* beta, int B, int nb)
{
    if (!d_tab || !n || !beta || B < 1 || nb < 1 || nb > kBMaxBands || (op != BL_SOFT && op != BL_HARD) || !sizes_ok(n, nb)) return PDWT_EINVAL;
    const int gmax = kGroupSlots / nb, g_images = B < gmax ? B : gmax;
    BatchDesc d;
    memset(&d, 0, sizeof(d));
    d.nb = nb;
    bool take[kBMaxBands];
    for (int k = 0; k < nb; k++) {
        d.n[k] = n[k];
        take[k] = false;
        for (int b = 0; b < B && !take[k]; b++) take[k] = n[k] && !(beta[(size_t)b * nb + k] < T(0));
    }
    layout(d, n, nb, take, g_images);
    if (!d.blk0[nb]) return PDWT_OK;  // every beta is negative
    int dev = 0;
    Scratch* s = scratch(&dev);
    if (!s) return PDWT_ENOMEM;
    std::lock_guard<std::mutex> lk(g_batch_mu[dev]);
    for (int g0 = 0; g0 < B; g0 += gmax) {
        const int bg = B - g0 < gmax ? B - g0 : gmax;
        T* const* tab = d_tab + (size_t)g0 * nb;
        // descriptor and betas of the group through the staging buffer: `beta` may be freed as soon as this entry returns
        if (const int rc = stage_h2d(s, s->desc, &d, sizeof(d), 0, true); rc != PDWT_OK) return rc;
        if (const int rc = stage_h2d(s, s->beta, beta + (size_t)g0 * nb, (size_t)bg * nb * sizeof(T), kDescBytes, false); rc != PDWT_OK) return rc;
        if (const int rc = stage_done(s); rc != PDWT_OK) return rc;
        KTimer kt(K_SOFT_THRESH);
        if (op == BL_SOFT) hipLaunchKernelGGL((k_bb_thresh<T, BL_SOFT>), dim3(d.blk0[nb], bg), dim3(kBThreads), 0, stream(), tab, s->desc, (const T*)s->beta);
        else hipLaunchKernelGGL((k_bb_thresh<T, BL_HARD>), dim3(d.blk0[nb], bg), dim3(kBThreads), 0, stream(), tab, s->desc, (const T*)s->beta);
        PDWT_CHECK_LAUNCH();
    }
    return PDWT_OK;
}

}  // namespace
}  // namespace pdwt

using namespace pdwt;

extern "C" {
int pdwt_bandbatch_stats_f32(const float* const* d_ptr, const size_t* n, int B, int nb, const unsigned char* want_median, pdwt_band_stats* out)
{
    return band_batch_stats<float>(d_ptr, n, B, nb, want_median, reinterpret_cast<BandStats*>(out));
}
int pdwt_bandbatch_stats_f64(const double* const* d_ptr, const size_t* n, int B, int nb, const unsigned char* want_median, pdwt_band_stats* out)
{
    return band_batch_stats<double>(d_ptr, n, B, nb, want_median, reinterpret_cast<BandStats*>(out));
}
int pdwt_bandbatch_thresh_f32(int op, float* const* d_ptr, const size_t* n, const float* beta, int B, int nb) { return band_batch_thresh<float>(op, d_ptr, n, beta, B, nb); }
int pdwt_bandbatch_thresh_f64(int op, double* const* d_ptr, const size_t* n, const double* beta, int B, int nb) { return band_batch_thresh<double>(op, d_ptr, n, beta, B, nb); }
}
