// z_stages.hpp -- the pass along z of the 3-D transforms, written once for the three families that run it: the periodised volume
// transform (dwt3d.hip), one level of the boundary-mode transform and its adjoint (dwt_ext3d.hip, dwt_ext3d_adj.hip) and the same on a
// stack of volumes (dwt_ext3db.hip).  Here: the chunk, the jobs, the three kernels (analysis, synthesis, the adjoint of the analysis)
// and their launches.  A translation unit instantiates what it launches, so each family keeps kernels of its own.
//
// Lanes run across a plane (coalesced), blockIdx.y = a chunk of ZC outputs along z, blockIdx.z = a slot that the job decodes: the x-y
// quadrant of one volume (ZJob, Adj3ZJob) or a (volume, quadrant) pair of a stack (ZStackJob, Adj3ZStackJob).  A thread loads the planes of
// its chunk ONCE into a register window and computes every output of the chunk from it; all loops unroll completely.
//
// What a kernel is parametrised on besides <T, HL>:
//   Job   the decoding of grid z.  The body is the same text for either job: the column pointers are offset by the volume, which is
//         the constant 0 of a one-volume job.
//   PER   (analysis, synthesis) the treatment of the boundary, a compile-time constant: periodised (the window is read through wrap_ext /
//         wrap_per and starts HL/2 - 1 samples / HL/4 coefficients early) or by a boundary mode (ext_index on the chunks at the border,
//         zeros in the overhang of the synthesis).  The synthesis rule itself is the one of tile_stages.hpp: sample g reads the
//         coefficients (gp >> 1) + m with the taps HL-2-2m (gp even) / HL-1-2m (gp odd), gp = g + SHIFT.
// Per output the tap order, the one FMA per tap and, in the synthesis, the single addition sa + sd at the end are those of the tile
// stages: a volume's result does not depend on the family that computed it.
//
// The taps are a by-value kernel argument and are indexed in the kernel's own body only, never handed to a function and never part of
// a job: a bank that a function takes by reference is copied at the kernel's entry, which hoists all 2 * HL scalar tap loads in front
// of the loops (for the 40-tap double bank 1600 lane reads of spilled SGPRs); read in place they are loaded where they are used.  A
// kernel template on the job does not have that cost.  The lane of the adjoint is the one exception that is known to
// work: it takes the lane index as an argument and has no barrier, so a host program runs it lane by lane under a sanitizer.
#pragma once
#include "dwt_ext_adj.hpp"

namespace pdwt {

constexpr int kZThreads = 256;
constexpr int ZC = 16;                 // outputs per thread along z
constexpr int kZMaxSlots = 65535;      // slots of a launch: a grid dimension
constexpr int kA3MaxHalo = 2 * PDWT_MAX_FILTER_WIDTH - 3;  // halo cells of a line: F - 2 left, 2 hz - nz <= F - 1 right

// ---- jobs: the pointers and sizes of a pass, slot(z) = what grid z stands for, first(p) = (host) the first slot of a launch -------------
// slot z of a launch: quadrant e of volume v
struct ZSlot {
    size_t v;
    int e;
};
// where volume v starts in a stack of `planes` planes of pl elements per volume
__host__ __device__ __forceinline__ size_t z_volume(size_t v, int planes, size_t pl) { return v * (size_t)planes * pl; }
__host__ __device__ __forceinline__ ZSlot z_slot_of_pair(size_t p) { return ZSlot{p >> 2, (int)(p & 3)}; }  // pair p = 4 * v + e

template <typename T>
struct ZJob {
    const T* src[4];   // analysis: quadrants (nin planes); synthesis: z-low bands (nin planes)
    const T* src2[4];  // synthesis: z-high bands
    T* lo[4];          // analysis: z-low bands; synthesis: quadrants (nout planes)
    T* hi[4];          // analysis: z-high bands
    int nin, nout, plane, mode;  // (mode: the boundary-mode analysis)
    __host__ __device__ __forceinline__ ZSlot slot(unsigned z) const { return ZSlot{0, (int)z}; }
    void first(size_t) {}
};
// the same on stacks of V volumes (V x nin, V x nout planes); grid z = the pairs from pair0, a launch may begin inside a volume
template <typename T>
struct ZStackJob : ZJob<T> {
    size_t pair0;
    __host__ __device__ __forceinline__ ZSlot slot(unsigned z) const { return z_slot_of_pair(pair0 + z); }
    void first(size_t p) { pair0 = p; }
};

template <typename T>
struct Adj3ZJob {
    const T* lo[4];  // z-low cotangent bands of the quadrants (hz planes)
    const T* hi[4];  // z-high
    T* q[4];         // quadrant cotangents (nz planes)
    int nz, hz, plane;  // (grid z = the quadrant)
    void first(size_t) {}
};
template <typename T>
struct Adj3ZStackJob : Adj3ZJob<T> {
    size_t pair0;
    __host__ __device__ __forceinline__ ZSlot slot(unsigned z) const { return z_slot_of_pair(pair0 + z); }
    void first(size_t p) { pair0 = p; }
};

// ---- what the boundary treatment decides (scalars only) ----------------------------------------------------------------------------
// first plane of the analysis window of the chunk from output i0; first coefficient plane of the synthesis window of the chunk from
// sample g0 (its sample shift: SHIFT in the kernel)
template <bool PER, int HL>
__device__ __forceinline__ int z_ana_start(int i0) { return PER ? 2 * i0 - (HL / 2 - 1) : 2 * i0 + 2 - HL; }
template <bool PER, int HL>
__device__ __forceinline__ int z_syn_start(int g0) { return PER ? g0 / 2 - HL / 4 : g0 / 2; }

// ---- analysis: output i reads the extended planes 2i + 1 - k (boundary modes) / 2i + HL/2 - k (periodised), k = 0 .. HL-1 ------------
// The window of the chunk from i0 holds 2 * ZC + HL - 2 planes.  Boundary modes: each plane index goes through ext_index (-1: the plane
// is 0); a chunk whose window lies inside the volume skips the map (a workgroup-uniform branch).
template <typename T, int HL, bool PER, typename Job>
__global__ __launch_bounds__(kZThreads) void k_z_analysis(Job job, Taps2<T> taps)
{
    const int k = blockIdx.x * kZThreads + threadIdx.x;
    if (k >= job.plane) return;
    const ZSlot p = job.slot(blockIdx.z);
    const int e = p.e, i0 = blockIdx.y * ZC;
    constexpr int W = 2 * ZC + HL - 2;
    const int n = job.nin, s0 = z_ana_start<PER, HL>(i0);
    const size_t pl = (size_t)job.plane;
    const T* __restrict__ x = job.src[e] + z_volume(p.v, job.nin, pl) + k;
    T v[W];
    if constexpr (PER) {
#pragma unroll
        for (int w = 0; w < W; w++) v[w] = x[(size_t)wrap_ext(s0 + w, n) * pl];
    } else if (s0 >= 0 && s0 + W <= n) {
#pragma unroll
        for (int w = 0; w < W; w++) v[w] = x[(size_t)(s0 + w) * pl];
    } else {
#pragma unroll
        for (int w = 0; w < W; w++) {
            const int s = ext_index(s0 + w, n, job.mode);
            v[w] = s < 0 ? T(0) : x[(size_t)s * pl];
        }
    }
    T* __restrict__ lo = job.lo[e] + z_volume(p.v, job.nout, pl) + k;
    T* __restrict__ hi = job.hi[e] + z_volume(p.v, job.nout, pl) + k;
#pragma unroll
    for (int u = 0; u < ZC; u++) {
        if (i0 + u < job.nout) {
            T sl = T(0), sh = T(0);
#pragma unroll
            for (int j = 0; j < HL; j++) {
                sl = fma_t<T>(v[2 * u + j], taps.a[HL - 1 - j], sl);
                sh = fma_t<T>(v[2 * u + j], taps.b[HL - 1 - j], sh);
            }
            lo[(size_t)(i0 + u) * pl] = sl;
            hi[(size_t)(i0 + u) * pl] = sh;
        }
    }
}

// ---- synthesis: the chunk of ZC samples from the even g0 reads tile_inv_win(ZC, HL, PER) coefficient planes -------------------------
// Boundary modes: no wrap; planes past the band are loaded as 0 (only in the overhang of the last chunk, whose samples are not stored).
template <typename T, int HL, bool PER, typename Job>
__global__ __launch_bounds__(kZThreads) void k_z_synthesis(Job job, Taps2<T> taps)
{
    const int k = blockIdx.x * kZThreads + threadIdx.x;
    if (k >= job.plane) return;
    const ZSlot p = job.slot(blockIdx.z);
    const int e = p.e, g0 = blockIdx.y * ZC;  // even
    constexpr int h2 = HL / 2, SHIFT = PER ? syn_shift(HL) : 0, W = tile_inv_win(ZC, HL, PER);
    const int nin = job.nin, q0 = z_syn_start<PER, HL>(g0);
    const size_t pl = (size_t)job.plane;
    const T* __restrict__ a = job.src[e] + z_volume(p.v, job.nin, pl) + k;
    const T* __restrict__ d = job.src2[e] + z_volume(p.v, job.nin, pl) + k;
    T va[W], vd[W];
#pragma unroll
    for (int w = 0; w < W; w++) {
        if constexpr (PER) {
            const size_t s = (size_t)wrap_per(q0 + w, nin) * pl;
            va[w] = a[s];
            vd[w] = d[s];
        } else {
            const bool in = q0 + w < nin;
            const size_t s = (size_t)(q0 + w) * pl;
            va[w] = in ? a[s] : T(0);
            vd[w] = in ? d[s] : T(0);
        }
    }
    T* __restrict__ out = job.lo[e] + z_volume(p.v, job.nout, pl) + k;
#pragma unroll
    for (int u = 0; u < ZC; u++) {
        if (g0 + u < job.nout) {
            const int gp = u + SHIFT, lp = gp >> 1, odd = gp & 1;  // compile-time after unrolling
            T sa = T(0), sd = T(0);
#pragma unroll
            for (int m = 0; m < h2; m++) {
                sa = fma_t<T>(va[lp + m], taps.a[HL - 2 + odd - 2 * m], sa);
                sd = fma_t<T>(vd[lp + m], taps.b[HL - 2 + odd - 2 * m], sd);
            }
            out[(size_t)(g0 + u) * pl] = sa + sd;
        }
    }
}

// ---- the adjoint of the boundary-mode analysis -------------------------------------------------------------------------------------
// A line along z has nz samples, the bank the even length F, hz = (nz + F - 1) / 2.  Cotangent stacks lo[q], hi[q] (hz planes of
// `plane` elements) of the four x-y quadrants q, in the notation of dwt_ext_adj.hpp:
//   u[s]    = sum_i lo[i] L[2i + 1 - s] + hi[i] H[2i + 1 - s]      s = 2 - F .. 2 hz - 1; planes i outside 0 .. hz - 1 count as 0
//   Q[q][k] = sum of u[s] over the s with ext_index(s, nz, mode) == k, ascending s with s = k in its place, starting from 0
// With the reversed taps L'[j] = L[F-1-j] (taps_adj) u[s] = sum_m lo[floor(s / 2) + m] L'[F - 2 + (s & 1) - 2m], m = 0 .. F/2 - 1: for a
// sample cell s = k that is the formula of the boundary-mode synthesis (no plane below 0, none past hz - 1), for a halo cell the same sum
// bounded on both sides.  The fold runs in the same pass: a line has at most 2F - 3 halo cells, whose targets the host computes once
// with ext_index (Adj3ZHalo); a chunk of samples that no halo cell repeats does nothing extra, any other evaluates u of the halo cells
// that map into it straight from the two stacks and adds them in the fixed order.  No frame in scratch, no atomics: every output
// element is written once by one thread.

// the halo cells of a line in the order of adj_halo_s (left ascending, then right ascending), passed to the kernel by value.  It carries
// a copy of the bank for those cells: they index the taps at run time (a rolled loop), the sample cells at compile time; a by-value
// argument that is read both ways ends as a copy in scratch for the longer banks, one that is only indexed at run time is read in place.
template <typename T>
struct Adj3ZHalo {
    int tgt[kA3MaxHalo];  // the sample that halo cell h repeats (ext_index)
    int nh;               // halo cells; 0 in mode zero (no pre-images: every chunk takes the plain path)
    int z0, z1;           // the longest run [z0, z1) of samples that no halo cell repeats
    Taps2<T> taps;        // = the kernel's taps argument (taps_adj)
};

// (host) the table of a line of nz samples, the way adj_gap of dwt_ext_adj.hip finds the run
template <typename T>
inline Adj3ZHalo<T> adj3_z_halo(int nz, int F, int mode, const Taps2<T>& taps)
{
    Adj3ZHalo<T> hm{};
    hm.taps = taps;
    hm.nh = mode == EXT_ZERO ? 0 : adj_halo_len(nz, F);
    hm.z0 = 0, hm.z1 = nz;
    if (!hm.nh) return hm;
    for (int h = 0; h < hm.nh; h++) hm.tgt[h] = ext_index(adj_halo_s(h, nz, F), nz, mode);
    // sort a copy of the targets and take the widest gap (before the first, between two, after the last)
    int t[kA3MaxHalo];
    for (int h = 0; h < hm.nh; h++) {
        int j = h;
        for (; j > 0 && t[j - 1] > hm.tgt[h]; j--) t[j] = t[j - 1];
        t[j] = hm.tgt[h];
    }
    hm.z0 = 0, hm.z1 = t[0];
    for (int i = 0; i < hm.nh; i++) {
        const int a = t[i] + 1, b = i + 1 < hm.nh ? t[i + 1] : nz;
        if (b - a > hm.z1 - hm.z0) hm.z0 = a, hm.z1 = b;
    }
    return hm;
}

template <typename T>
__host__ __device__ __forceinline__ T adj3_fma(T a, T b, T c)
{
    if constexpr (sizeof(T) == 4) return __builtin_fmaf(a, b, c);
    else return __builtin_fma(a, b, c);
}

// u[s] of ANY cell of the extended line, straight from the two stacks (a, d: the lane's column, plane stride pl), bounded on both sides
template <typename T, int HL>
__host__ __device__ __forceinline__ T adj3_z_cell(const T* __restrict__ a, const T* __restrict__ d, size_t pl, int hz, int s, const Taps2<T>& taps)
{
    const int odd = s & 1, i0 = (s - odd) / 2;  // floor(s / 2), s may be negative
    T sa = T(0), sd = T(0);
#pragma unroll 1
    for (int m = 0; m < HL / 2; m++) {  // (rolled: 16 copies of this loop are inlined; the tap index is uniform)
        const int i = i0 + m;
        if ((unsigned)i < (unsigned)hz) {
            sa = adj3_fma<T>(a[(size_t)i * pl], taps.a[HL - 2 + odd - 2 * m], sa);
            sd = adj3_fma<T>(d[(size_t)i * pl], taps.b[HL - 2 + odd - 2 * m], sd);
        }
    }
    return sa + sd;
}

// The samples g0 .. g0 + ZC - 1 (g0 even) of column k of quadrant e: the register window of the boundary-mode synthesis on the two
// cotangent stacks, then per sample its own cell and, in a chunk that a halo cell maps into, the fold.  taps: taps_adj.
template <typename T, int HL>
__host__ __device__ __forceinline__ void ext3_adj_z_lane(const Adj3ZJob<T>& job, const Taps2<T>& taps, const Adj3ZHalo<T>& hm, int e, int g0, int k)
{
    constexpr int h2 = HL / 2, W = ZC / 2 + h2 - 1;
    const int nz = job.nz, hz = job.hz, q0 = g0 / 2;
    const size_t pl = (size_t)job.plane;
    const T* __restrict__ a = job.lo[e] + k;
    const T* __restrict__ d = job.hi[e] + k;
    T va[W], vd[W];
#pragma unroll
    for (int w = 0; w < W; w++) {
        const bool in = q0 + w < hz;
        const size_t s = (size_t)(q0 + w) * pl;
        va[w] = in ? a[s] : T(0);
        vd[w] = in ? d[s] : T(0);
    }
    const int gend = g0 + ZC < nz ? g0 + ZC : nz;
    const bool plain = hm.nh == 0 || (g0 >= hm.z0 && gend <= hm.z1);  // (uniform over the workgroup) no halo cell repeats a sample of the chunk
    T* __restrict__ out = job.q[e] + k;
#pragma unroll
    for (int u = 0; u < ZC; u++) {
        if (g0 + u < nz) {
            const int lp = u >> 1, odd = u & 1;  // compile-time after unrolling
            T sa = T(0), sd = T(0);
#pragma unroll
            for (int m = 0; m < h2; m++) {
                sa = adj3_fma<T>(va[lp + m], taps.a[HL - 2 + odd - 2 * m], sa);
                sd = adj3_fma<T>(vd[lp + m], taps.b[HL - 2 + odd - 2 * m], sd);
            }
            T acc = sa + sd;
            if (!plain) {
                // left halo cells ascending, the sample's own cell, right halo cells ascending (nh >= HL - 2: the own cell is always met)
                const T own = acc;
                acc = T(0);
                for (int h = 0; h <= hm.nh; h++) {
                    if (h == HL - 2) acc += own;
                    if (h < hm.nh && hm.tgt[h] == g0 + u) acc += adj3_z_cell<T, HL>(a, d, pl, hz, adj_halo_s(h, nz, HL), hm.taps);
                }
            }
            out[(size_t)(g0 + u) * pl] = acc;
        }
    }
}

// The same of slot z of a stack job: the lane on the stacks of that volume, as slot 0 of a job of its own (the slot index is then a
// constant: the job stays in registers).
template <typename T, int HL>
__host__ __device__ __forceinline__ void ext3_adj_z_lane(const Adj3ZStackJob<T>& job, const Taps2<T>& taps, const Adj3ZHalo<T>& hm, unsigned z, int g0, int k)
{
    const ZSlot p = job.slot(z);
    const size_t pl = (size_t)job.plane;
    Adj3ZJob<T> one{};
    one.lo[0] = job.lo[p.e] + z_volume(p.v, job.hz, pl);
    one.hi[0] = job.hi[p.e] + z_volume(p.v, job.hz, pl);
    one.q[0] = job.q[p.e] + z_volume(p.v, job.nz, pl);
    one.nz = job.nz, one.hz = job.hz, one.plane = job.plane;
    ext3_adj_z_lane<T, HL>(one, taps, hm, 0, g0, k);
}

// grid as the synthesis: blockIdx.y = a chunk of ZC samples, blockIdx.z = the slot
template <typename T, int HL, typename Job>
__global__ __launch_bounds__(kZThreads) void k_z_adjoint(Job job, Taps2<T> taps, Adj3ZHalo<T> hm)
{
    const int k = blockIdx.x * kZThreads + threadIdx.x;
    if (k >= job.plane) return;
    ext3_adj_z_lane<T, HL>(job, taps, hm, blockIdx.z, blockIdx.y * ZC, k);
}

// ---- launches: `slots` slots of the job from the first one, in launches of at most a grid dimension ------------------------------------
template <typename F>
inline int z_chunks(size_t total, F&& f)  // f(first, count) over 0 .. total in chunks of kZMaxSlots; stops at the first error
{
    for (size_t p0 = 0; p0 < total; p0 += kZMaxSlots) {
        const int cnt = (int)(total - p0 < (size_t)kZMaxSlots ? total - p0 : (size_t)kZMaxSlots);
        if (const int rc = f(p0, cnt); rc != PDWT_OK) return rc;
    }
    return PDWT_OK;
}

template <bool PER, typename T, typename Job>
inline int run_z(int hlen, bool analysis, Job zj, size_t slots, const Taps2<T>& taps)
{
    return z_chunks(slots, [&](size_t p0, int cnt) {
        zj.first(p0);
        const dim3 grid(idiv_up(zj.plane, kZThreads), idiv_up(zj.nout, ZC), cnt);
        return with_filter_length(hlen, [&](auto hl) {
            constexpr int HL = decltype(hl)::value;
            return launch_lds(analysis ? k_z_analysis<T, HL, PER, Job> : k_z_synthesis<T, HL, PER, Job>, grid, dim3(kZThreads), 0, zj, taps);
        });
    });
}
template <typename T, typename Job>
inline int run_z_adjoint(int hlen, Job zj, size_t slots, const Taps2<T>& taps, const Adj3ZHalo<T>& hm)
{
    return z_chunks(slots, [&](size_t p0, int cnt) {
        zj.first(p0);
        const dim3 grid(idiv_up(zj.plane, kZThreads), idiv_up(zj.nz, ZC), cnt);
        return with_filter_length(hlen, [&](auto hl) { return launch_lds(k_z_adjoint<T, decltype(hl)::value, Job>, grid, dim3(kZThreads), 0, zj, taps, hm); });
    });
}

}  // namespace pdwt
