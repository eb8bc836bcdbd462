// bandstats.hip -- per-band statistics of the coefficients: sum |c|, sum c^2, max |c| (one pass over all bands) and the exact
// median of |c| (radix select), over an explicit band list like k_soft_thresh / k_abs_sum of utils.hip.  No reference
// counterpart (its TODO.txt lists "Compute norm related to threshold"); what it replaces is the host round trip
// get_coeff -> numpy median -> threshold.
//
// MI355X design
//   Work split: every block belongs to ONE band and owns one contiguous run of that band's 4096-element chunks (the block
//     counts are proportional to the band sizes, at least one per band), so a block has one destination for what it gathers.
//   Moments (k_band_moments): per-lane double accumulation of |c| and c^2, max in T -> wave64 shuffles -> LDS across the 4 waves
//     -> three doubles per block with plain (write-through) stores -> the LAST block to arrive adds each band's partials in a
//     fixed order.  No float atomics: the bits do not depend on the order in which blocks finish.
//   Selection (k_band_hist + k_band_pick): radix select on the bit pattern of |c| (for non-negative IEEE values the unsigned
//     order of the bits is the numeric order; -0.0 maps to +0.0; a NaN orders above +inf), 11 bits per pass: 3 passes for
//     float, 6 for double.  A pass reads each asking band once and counts the elements whose high bits equal the prefix found
//     so far into a 2048-bin histogram: LDS per workgroup, then 64-bit integer adds into the band's global histogram (integer
//     adds commute: the counts do not depend on arrival order).  k_band_pick (one workgroup per asking band) scans the bins,
//     extends the prefix, reduces the rank and clears the histogram.  The two ranks of a median ((n-1)/2 and n/2) ride the same
//     passes: they share one prefix and one histogram until they part, from then on a second histogram is filled as well.
//     Nothing synchronises between the passes; one copy to the host at the end.
//   Contention: bands are often mostly zeros or constant, and then most lanes of a wave want one LDS bin.  Before the LDS add
//     the wave aggregates twice: the lanes that agree with the first counting lane are added as ONE add of their number, then
//     the same among the lanes left over; only what remains after the two rounds is added lane by lane.
#include <math.h>
#include <string.h>

#include <mutex>

#include "common.hpp"
#include "bandlist.hpp"

namespace pdwt {
namespace {

constexpr int kSThreads = 256;
constexpr int kSChunk = kSThreads * 16;  // elements per block-iteration, as in utils.hip
constexpr int kSMaxBands = 3 * 32 + 1;
constexpr int kMomBlocks = 2048;         // block budget of the moments launch (256 CUs x 8), + one per band at most
constexpr int kHistBlocks = 1024;        // block budget of a histogram pass: every block flushes up to 2048 bins
constexpr int kHistMinChunks = 4;        // ... so a block counts at least this many chunks when the band has them
constexpr int kBins = 2048;              // 11 bits per pass
constexpr int kDigitBits = 11;

template <typename T>
struct StatTable {
    const T* ptr[kSMaxBands];
    unsigned long long n[kSMaxBands];
    unsigned int blk0[kSMaxBands + 1];  // first block of each band; [nb] = grid size
    unsigned int nchunk[kSMaxBands];
    unsigned short slot[kSMaxBands];    // where the band's results go (moments: output row; select: request state + histograms)
    int nb;
};

// state of one asking band between the passes of a selection: [0] = the lower rank, [1] = the upper one
struct SelState {
    unsigned long long prefix[2];
    unsigned long long rank[2];
};
struct SelInit {
    unsigned long long rank[2][kSMaxBands];
};

template <typename T> struct V16s;
template <> struct V16s<float> { static constexpr int N = 4; };
template <> struct V16s<double> { static constexpr int N = 2; };

__device__ __forceinline__ unsigned int key_of(float x) { return __float_as_uint(x) & 0x7fffffffu; }
__device__ __forceinline__ unsigned long long key_of(double x) { return (unsigned long long)__double_as_longlong(x) & 0x7fffffffffffffffull; }

__device__ __forceinline__ int band_of_block(const unsigned int* blk0, int nb, unsigned int b)
{
    int k = 0;
    while (k + 1 < nb && b >= blk0[k + 1]) k++;
    return k;
}

// f(x) for every element of the calling block's run of chunks of band k, walked from its end (what a pass that wrote the band
// front to back left in the cache).  NT: non-temporal loads (nothing is read twice by the caller's launch).
template <typename T, bool VEC, bool NT, typename F>
__device__ __forceinline__ void walk_run(const StatTable<T>& tab, int k, F&& f)
{
    const T* __restrict__ p = tab.ptr[k];
    const unsigned long long n = tab.n[k];
    const unsigned int nblk = tab.blk0[k + 1] - tab.blk0[k], j = blockIdx.x - tab.blk0[k];
    const unsigned int nch = tab.nchunk[k], per = (nch + nblk - 1) / nblk;
    const unsigned long long lo = (unsigned long long)j * per;
    unsigned long long hi = lo + per;
    if (hi > nch) hi = nch;
    for (unsigned long long cc = hi; cc > lo; cc--) {
        const unsigned long long base = (cc - 1) * kSChunk;
        if constexpr (VEC) {
            constexpr int NV = V16s<T>::N;
            constexpr int U = kSChunk / (kSThreads * NV);
            typedef T NTV __attribute__((ext_vector_type(NV)));
            if (base + kSChunk <= n) {  // full chunk: no bounds checks, every load in flight before the first use
                NTV v[U];
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const NTV* q = reinterpret_cast<const NTV*>(p + base + ((unsigned long long)u * kSThreads + threadIdx.x) * NV);
                    v[u] = NT ? __builtin_nontemporal_load(q) : *q;
                }
#pragma unroll
                for (int u = 0; u < U; u++) {
#pragma unroll
                    for (int q = 0; q < NV; q++) f(v[u][q]);
                }
            } else {
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const unsigned long long i = base + ((unsigned long long)u * kSThreads + threadIdx.x) * NV;
                    if (i + NV <= n) {
                        const NTV v = *reinterpret_cast<const NTV*>(p + i);
#pragma unroll
                        for (int q = 0; q < NV; q++) f(v[q]);
                    } else {
                        for (unsigned long long e = i; e < n; e++) f(p[e]);
                    }
                }
            }
        } else {
            for (int u = 0; u < kSChunk / kSThreads; u++) {
                const unsigned long long i = base + (unsigned long long)u * kSThreads + threadIdx.x;
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

// part: 3 doubles per block (sum |c|, sum c^2, max |c|); out: 3 doubles per band; ticket: arrival counter, 0 between launches
template <typename T, bool VEC>
__global__ __launch_bounds__(kSThreads) void k_band_moments(StatTable<T> tab, double* __restrict__ part, double* __restrict__ out,
                                                            unsigned int* __restrict__ ticket)
{
    __shared__ double s_w[3][kSThreads / 64];
    __shared__ int s_last;
    const int k = band_of_block(tab.blk0, tab.nb, blockIdx.x);
    double sa = 0.0, sq = 0.0;
    T mx = T(0);
    walk_run<T, VEC, true>(tab, k, [&](T x) {
        const T a = x < T(0) ? -x : x;
        const double d = (double)a;
        sa += d;
        sq = fma(d, d, sq);
        mx = a > mx ? a : mx;
    });
    sa = wsum(sa);
    sq = wsum(sq);
    double dm = wmax((double)mx);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        s_w[0][wave] = sa;
        s_w[1][wave] = sq;
        s_w[2][wave] = dm;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        // write-through stores, drained before the ticket is taken (the scheme of k_abs_sum, utils.hip)
        double m01 = s_w[2][0] > s_w[2][1] ? s_w[2][0] : s_w[2][1], m23 = s_w[2][2] > s_w[2][3] ? s_w[2][2] : s_w[2][3];
        __hip_atomic_store(part + 3 * (size_t)blockIdx.x + 0, (s_w[0][0] + s_w[0][1]) + (s_w[0][2] + s_w[0][3]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(part + 3 * (size_t)blockIdx.x + 1, (s_w[1][0] + s_w[1][1]) + (s_w[1][2] + s_w[1][3]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(part + 3 * (size_t)blockIdx.x + 2, m01 > m23 ? m01 : m23, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned int t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = (t == gridDim.x - 1);
    }
    __syncthreads();
    if (s_last) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        // one wave per band, lanes strided over the band's blocks, then the shuffle tree: a fixed order
        for (int b = wave; b < tab.nb; b += kSThreads / 64) {
            double a = 0.0, q = 0.0, m = 0.0;
            for (unsigned int i = tab.blk0[b] + lane; i < tab.blk0[b + 1]; i += 64) {
                a += __hip_atomic_load(part + 3 * (size_t)i + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                q += __hip_atomic_load(part + 3 * (size_t)i + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const double o = __hip_atomic_load(part + 3 * (size_t)i + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                m = o > m ? o : m;
            }
            a = wsum(a);
            q = wsum(q);
            m = wmax(m);
            if (lane == 0) {
                double* o = out + 3 * (size_t)tab.slot[b];
                o[0] = a;
                o[1] = q;
                o[2] = m;
            }
        }
        if (threadIdx.x == 0) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // next launch
    }
}

// one counting lane group -> LDS: `m` = this lane counts, `d` = its bin.  Two rounds of wave aggregation (file header), the rest lane by lane.
__device__ __forceinline__ void hist_add(unsigned int* s_hist, bool m, unsigned int d)
{
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int round = 0; round < 2; round++) {
        if (m) {  // (inside the branch only the counting lanes are active: the first of them gives the bin, the ballot counts them alone)
            const unsigned int first = (unsigned int)__builtin_amdgcn_readfirstlane((int)d);
            const bool same = d == first;
            const unsigned long long smask = __ballot(same);
            if (lane == __ffsll((long long)smask) - 1) atomicAdd(&s_hist[first], (unsigned int)__popcll(smask));
            m = !same;
        }
    }
    if (m) atomicAdd(&s_hist[d], 1u);
}

// one pass of the selection over the asking bands: hist[slot][which][bin] += number of elements of the band whose key has the
// high bits prefix[which] and the digit `bin` at `shift`.  FIRST: no prefix yet, every element counts.  hs = shift + width.
template <typename T, bool VEC, bool FIRST>
__global__ __launch_bounds__(kSThreads) void k_band_hist(StatTable<T> tab, const SelState* __restrict__ st, unsigned long long* __restrict__ hist,
                                                         int shift, int hs, unsigned int dmask)
{
    __shared__ unsigned int s_hist[2][kBins];
    const int k = band_of_block(tab.blk0, tab.nb, blockIdx.x);
    const int slot = tab.slot[k];
    using K = decltype(key_of(T(0)));
    K p0 = 0, p1 = 0;
    if constexpr (!FIRST) {
        p0 = (K)st[slot].prefix[0];
        p1 = (K)st[slot].prefix[1];
    }
    const bool two = p0 != p1;  // the two ranks have parted: count for both prefixes
    for (int i = threadIdx.x; i < 2 * kBins; i += kSThreads) (&s_hist[0][0])[i] = 0u;
    __syncthreads();
    walk_run<T, VEC, false>(tab, k, [&](T x) {
        const K key = key_of(x);
        const unsigned int d = (unsigned int)(key >> shift) & dmask;
        if constexpr (FIRST) {
            hist_add(s_hist[0], true, d);
        } else {
            const K hi = key >> hs;
            hist_add(s_hist[0], hi == p0, d);
            if (two) hist_add(s_hist[1], hi == p1, d);
        }
    });
    __syncthreads();
    unsigned long long* g = hist + (size_t)slot * 2 * kBins;
    for (int i = threadIdx.x; i < (two ? 2 : 1) * kBins; i += kSThreads) {
        const unsigned int c = (&s_hist[0][0])[i];
        if (c) atomicAdd(g + i, (unsigned long long)c);
    }
}

// one workgroup per asking band: find the bin that holds each rank, extend the prefix, reduce the rank, clear the histograms
template <bool FIRST>
__global__ __launch_bounds__(kSThreads) void k_band_pick(SelState* __restrict__ st, unsigned long long* __restrict__ hist, SelInit init, int width)
{
    __shared__ unsigned long long s_sum[kSThreads];
    constexpr int PER = kBins / kSThreads;  // 8 consecutive bins per thread
    const int slot = blockIdx.x;
    SelState s;
    if constexpr (FIRST) {
        s.prefix[0] = s.prefix[1] = 0;
        s.rank[0] = init.rank[0][slot];
        s.rank[1] = init.rank[1][slot];
    } else {
        s = st[slot];
    }
    const bool two = s.prefix[0] != s.prefix[1];
    unsigned long long* g = hist + (size_t)slot * 2 * kBins;
    SelState r = s;
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
        if (before <= rank && rank < before + own) {  // exactly one thread: the counts of a prefix add up to more than its rank
            unsigned long long acc = before;
#pragma unroll
            for (int i = 0; i < PER; i++) {
                if (acc <= rank && rank < acc + c[i]) {
                    r.prefix[w] = (s.prefix[w] << width) | (unsigned long long)(threadIdx.x * PER + i);
                    r.rank[w] = rank - acc;
                }
                acc += c[i];
            }
            st[slot].prefix[w] = r.prefix[w];
            st[slot].rank[w] = r.rank[w];
        }
    }
    __syncthreads();  // every read of the histograms is done
    for (int i = threadIdx.x; i < 2 * kBins; i += kSThreads) g[i] = 0ull;
}

#define PDWT_CHECK_LAUNCH() PDWT_HIP_TRY(hipGetLastError())

// per-device scratch, allocated on first use and reused; its size does not depend on the band sizes
struct Scratch {
    double* part;              // 3 x (kMomBlocks + kSMaxBands) block partials
    unsigned int* ticket;
    unsigned long long* hist;  // kSMaxBands x 2 x kBins
    // results, one contiguous region copied to the host once: 3 doubles per band, then one SelState per asking band
    double* mom;
    SelState* sel;
    void* base;
};
constexpr size_t kPartBytes = 3 * (size_t)(kMomBlocks + kSMaxBands) * sizeof(double);
constexpr size_t kTicketBytes = 64;
constexpr size_t kHistBytes = (size_t)kSMaxBands * 2 * kBins * sizeof(unsigned long long);
constexpr size_t kMomBytes = 3 * (size_t)kSMaxBands * sizeof(double);
constexpr size_t kSelBytes = (size_t)kSMaxBands * sizeof(SelState);
struct HostResult {
    double mom[3 * kSMaxBands];
    SelState sel[kSMaxBands];
};
static_assert(sizeof(HostResult) == kMomBytes + kSelBytes, "the result region is copied in one piece");

std::mutex g_smu;
std::mutex g_stat_mu[64];
Scratch g_scr[64] = {};

Scratch* scratch(int* dev_out)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
    *dev_out = dev;
    std::lock_guard<std::mutex> lk(g_smu);
    Scratch& s = g_scr[dev];
    if (!s.base) {
        const size_t total = kPartBytes + kTicketBytes + kHistBytes + kMomBytes + kSelBytes;
        void* b = nullptr;
        if (hipMalloc(&b, total) != hipSuccess) return nullptr;
        // the ticket and the histograms start at 0 (and the kernels leave them at 0); zeroed on the library stream
        if (hipMemsetAsync(b, 0, total, stream()) != hipSuccess) {
            (void)hipFree(b);
            return nullptr;
        }
        char* c = (char*)b;
        s.part = (double*)c;
        s.ticket = (unsigned int*)(c + kPartBytes);
        s.hist = (unsigned long long*)(c + kPartBytes + kTicketBytes);
        s.mom = (double*)(c + kPartBytes + kTicketBytes + kHistBytes);
        s.sel = (SelState*)(c + kPartBytes + kTicketBytes + kHistBytes + kMomBytes);
        s.base = b;
    }
    return &s;
}

// blocks of band k: proportional to its chunks within `budget`, at least one, at most one per `min_chunks` chunks
template <typename T>
bool stat_push(StatTable<T>& t, const T* p, size_t n, int slot, unsigned long long total_chunks, int budget, int min_chunks, bool& vec_ok)
{
    if (t.nb >= kSMaxBands || (!p && n)) return false;
    const unsigned long long nch = (n + kSChunk - 1) / kSChunk;
    if (nch > 0xffffffffull) return false;
    unsigned long long blocks = total_chunks ? nch * (unsigned long long)budget / total_chunks : 1;
    if (blocks > nch / min_chunks) blocks = nch / min_chunks;
    if (blocks < 1) blocks = 1;
    const int k = t.nb++;
    t.ptr[k] = p;
    t.n[k] = n;
    t.nchunk[k] = (unsigned int)nch;
    t.slot[k] = (unsigned short)slot;
    t.blk0[k + 1] = t.blk0[k] + (unsigned int)blocks;
    if (((uintptr_t)p & 15) != 0) vec_ok = false;
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
    double d;
    memcpy(&d, &key, sizeof(d));
    return d;
}

}  // namespace

template <typename T>
int band_list_stats(T* const* ptr, const size_t* n, int nb, const unsigned char* want_median, BandStats* out)
{
    if (!ptr || !n || !out || nb < 1 || nb > kSMaxBands) return PDWT_EINVAL;
    for (int k = 0; k < nb; k++)
        if (!ptr[k] && n[k]) return PDWT_EINVAL;
    constexpr int KEYBITS = (int)sizeof(T) * 8;
    // the moments table: every band with elements; the selection table: the asking ones among them
    StatTable<T> mt, st;
    mt.nb = st.nb = 0;
    mt.blk0[0] = st.blk0[0] = 0;
    bool mvec = true, svec = true;
    unsigned long long mtotal = 0, stotal = 0;
    for (int k = 0; k < nb; k++) {
        const unsigned long long nch = (n[k] + kSChunk - 1) / kSChunk;
        if (!(want_median && want_median[k] == 2)) mtotal += nch;  // (2: the median alone, no moments for this band)
        if (want_median && want_median[k]) stotal += nch;
    }
    SelInit init;
    int slot_of[kSMaxBands];
    for (int k = 0; k < nb; k++) {
        slot_of[k] = -1;
        if (!n[k]) continue;
        const bool moments = !(want_median && want_median[k] == 2);
        if (moments && !stat_push<T>(mt, ptr[k], n[k], k, mtotal, kMomBlocks, 1, mvec)) return PDWT_EINVAL;
        if (want_median && want_median[k]) {
            slot_of[k] = st.nb;
            init.rank[0][st.nb] = (n[k] - 1) / 2;
            init.rank[1][st.nb] = n[k] / 2;
            if (!stat_push<T>(st, ptr[k], n[k], st.nb, stotal, kHistBlocks, kHistMinChunks, svec)) return PDWT_EINVAL;
        }
    }
    HostResult res;
    if (mt.nb || st.nb) {
        int dev = 0;
        Scratch* s = scratch(&dev);
        if (!s) return PDWT_ENOMEM;
        std::lock_guard<std::mutex> lk(g_stat_mu[dev]);  // the scratch is shared by every instance on the device, until its results are out
        if (mt.nb) {
            KTimer kt(K_ABS_SUM);
            if (mvec) hipLaunchKernelGGL((k_band_moments<T, true>), dim3(mt.blk0[mt.nb]), dim3(kSThreads), 0, stream(), mt, s->part, s->mom, s->ticket);
            else hipLaunchKernelGGL((k_band_moments<T, false>), dim3(mt.blk0[mt.nb]), dim3(kSThreads), 0, stream(), mt, s->part, s->mom, s->ticket);
            PDWT_CHECK_LAUNCH();
        }
        if (st.nb) {
            KTimer kt(K_ABS_SUM);
            for (int pass = 0; pass * kDigitBits < KEYBITS; pass++) {
                const int hs = KEYBITS - kDigitBits * pass;
                const int shift = hs - kDigitBits > 0 ? hs - kDigitBits : 0, width = hs - shift;
                const unsigned int dmask = (1u << width) - 1u;
                const dim3 grid(st.blk0[st.nb]), block(kSThreads);
                if (pass == 0) {
                    if (svec) hipLaunchKernelGGL((k_band_hist<T, true, true>), grid, block, 0, stream(), st, s->sel, s->hist, shift, hs, dmask);
                    else hipLaunchKernelGGL((k_band_hist<T, false, true>), grid, block, 0, stream(), st, s->sel, s->hist, shift, hs, dmask);
                    PDWT_CHECK_LAUNCH();
                    hipLaunchKernelGGL((k_band_pick<true>), dim3(st.nb), block, 0, stream(), s->sel, s->hist, init, width);
                } else {
                    if (svec) hipLaunchKernelGGL((k_band_hist<T, true, false>), grid, block, 0, stream(), st, s->sel, s->hist, shift, hs, dmask);
                    else hipLaunchKernelGGL((k_band_hist<T, false, false>), grid, block, 0, stream(), st, s->sel, s->hist, shift, hs, dmask);
                    PDWT_CHECK_LAUNCH();
                    hipLaunchKernelGGL((k_band_pick<false>), dim3(st.nb), block, 0, stream(), s->sel, s->hist, init, width);
                }
                PDWT_CHECK_LAUNCH();
            }
        }
        // one copy: the moments of every band and, behind them, the keys of the asking ones
        const size_t nbytes = st.nb ? kMomBytes + (size_t)st.nb * sizeof(SelState) : kMomBytes;
        if (const int rc = pdwt_memcpy_d2h(&res, s->mom, nbytes); rc != PDWT_OK) return rc;
    }
    for (int k = 0; k < nb; k++) {
        BandStats& o = out[k];
        o.n = (double)n[k];
        const bool moments = !(want_median && want_median[k] == 2);
        o.sum_abs = !moments ? NAN : n[k] ? res.mom[3 * k + 0] : 0.0;
        o.sum_sq = !moments ? NAN : n[k] ? res.mom[3 * k + 1] : 0.0;
        o.max_abs = !moments ? NAN : n[k] ? res.mom[3 * k + 2] : 0.0;
        o.median_abs = NAN;
        if (slot_of[k] >= 0) {
            const SelState& r = res.sel[slot_of[k]];
            o.median_abs = 0.5 * (key_value<T>(r.prefix[0]) + key_value<T>(r.prefix[1]));
        }
    }
    return PDWT_OK;
}

template int band_list_stats<float>(float* const*, const size_t*, int, const unsigned char*, BandStats*);
template int band_list_stats<double>(double* const*, const size_t*, int, const unsigned char*, BandStats*);

}  // namespace pdwt

using namespace pdwt;

static_assert(sizeof(pdwt_band_stats) == sizeof(BandStats), "pdwt_band_stats must mirror BandStats");

// one beta per band; beta[k] < 0 leaves band k alone (such bands are dropped here: band_list_ew thresholds whatever it is given)
template <typename T>
static int bandlist_thresh(int op, T* const* ptr, const size_t* n, const T* beta, int nb)
{
    if (!ptr || !n || !beta || nb < 1 || nb > kSMaxBands || (op != BL_SOFT && op != BL_HARD)) return PDWT_EINVAL;
    T* p[kSMaxBands];
    size_t m[kSMaxBands];
    T b[kSMaxBands];
    int cnt = 0;
    for (int k = 0; k < nb; k++) {
        if (beta[k] < T(0) || !n[k]) continue;
        if (!ptr[k]) return PDWT_EINVAL;
        p[cnt] = ptr[k], m[cnt] = n[k], b[cnt] = beta[k], cnt++;
    }
    if (!cnt) return PDWT_OK;
    return band_list_ew<T>(op, p, m, b, cnt);
}

extern "C" {
int pdwt_bandlist_stats_f32(const float* const* d_ptr, const size_t* n, int nb, const unsigned char* want_median, pdwt_band_stats* out)
{
    return band_list_stats<float>(const_cast<float* const*>(d_ptr), n, nb, want_median, reinterpret_cast<BandStats*>(out));
}
int pdwt_bandlist_stats_f64(const double* const* d_ptr, const size_t* n, int nb, const unsigned char* want_median, pdwt_band_stats* out)
{
    return band_list_stats<double>(const_cast<double* const*>(d_ptr), n, nb, want_median, reinterpret_cast<BandStats*>(out));
}
int pdwt_bandlist_thresh_f32(int op, float* const* d_ptr, const size_t* n, const float* beta, int nb) { return bandlist_thresh<float>(op, d_ptr, n, beta, nb); }
int pdwt_bandlist_thresh_f64(int op, double* const* d_ptr, const size_t* n, const double* beta, int nb) { return bandlist_thresh<double>(op, d_ptr, n, beta, nb); }
}
