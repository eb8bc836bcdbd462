// dwt_ext3d_adj.hpp -- the z stage of the ADJOINT of the 3-D forward transform with signal-extension boundary modes (dwt_ext3d_adj.hip;
// include/pdwt_hip.h "Adjoints of the 3-D boundary-mode DWT").  The x-y half of a level adjoint is the 2-D level adjoint of
// dwt_ext_adj.hip on B = nz planes; what is new is the adjoint along z, stated here in the notation of dwt_ext_adj.hpp.
//
// A line along z has nz samples, the bank the even length F, hz = (nz + F - 1) / 2.  Cotangent stacks lo[q], hi[q] (hz planes of
// `plane` elements) of the four x-y quadrants q:
//   u[s]    = sum_i lo[i] L[2i + 1 - s] + hi[i] H[2i + 1 - s]      s = 2 - F .. 2 hz - 1; planes i outside 0 .. hz - 1 count as 0
//   Q[q][k] = sum of u[s] over the s with ext_index(s, nz, mode) == k, ascending s with s = k in its place, starting from 0
// With the reversed taps L'[j] = L[F-1-j] (taps_adj) u[s] = sum_m lo[floor(s / 2) + m] L'[F - 2 + (s & 1) - 2m], m = 0 .. F/2 - 1: for a
// sample cell s = k that is the formula of k_ext3_syn_z (no plane below 0, none past hz - 1), for a halo cell the same sum bounded on
// both sides.  The fold runs in the same pass: a line has at most 2F - 3 halo cells, whose targets the host computes once with ext_index
// (Adj3ZHalo); a chunk of samples that no halo cell repeats does nothing extra, any other evaluates u of the halo cells that map into
// it straight from the two stacks and adds them in the fixed order.  No frame in scratch, no atomics: every output element is written
// once by one thread.
//
// The per-thread body takes the lane index as an argument and has no barrier, so a host program runs it lane by lane under a sanitizer.
#pragma once
#include "dwt_ext_adj.hpp"

namespace pdwt {

constexpr int kA3ZThreads = 256;
constexpr int A3ZC = 16;                                      // samples per thread along z (X3ZC of dwt_ext3d.hip)
constexpr int kA3MaxHalo = 2 * PDWT_MAX_FILTER_WIDTH - 3;     // halo cells of a line: F - 2 left, 2 hz - nz <= F - 1 right

template <typename T>
struct Adj3ZJob {
    const T* lo[4];  // z-low cotangent bands of the quadrants (hz planes)
    const T* hi[4];  // z-high
    T* q[4];         // quadrant cotangents (nz planes)
    int nz, hz, plane;
};

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

// The samples g0 .. g0 + A3ZC - 1 (g0 even) of column k of quadrant e: the register window of k_ext3_syn_z on the two cotangent stacks,
// then per sample its own cell and, in a chunk that a halo cell maps into, the fold.  taps: taps_adj.
template <typename T, int HL>
__host__ __device__ __forceinline__ void ext3_adj_z_lane(const Adj3ZJob<T>& job, const Taps2<T>& taps, const Adj3ZHalo<T>& hm, int e, int g0, int k)
{
    constexpr int h2 = HL / 2, W = A3ZC / 2 + h2 - 1;
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
    const int gend = g0 + A3ZC < nz ? g0 + A3ZC : nz;
    const bool plain = hm.nh == 0 || (g0 >= hm.z0 && gend <= hm.z1);  // (uniform over the workgroup) no halo cell repeats a sample of the chunk
    T* __restrict__ out = job.q[e] + k;
#pragma unroll
    for (int u = 0; u < A3ZC; u++) {
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

}  // namespace pdwt
