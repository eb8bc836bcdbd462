// dwt_ext3db.hpp -- what the z kernels of the batched 3-D boundary-mode transform (dwt_ext3db.hip) share: the jobs, the decoding of grid z
// into a (volume, quadrant) pair, the offset of a volume in a stack, and the lane of the z adjoint on a stack.  The lane takes the grid
// indices as arguments and has no barrier, so a host program runs it pair by pair, chunk by chunk and column by column under a
// sanitizer, like ext3_adj_z_lane of dwt_ext3d_adj.hpp, which it calls.
#pragma once
#include "dwt_ext3d_adj.hpp"

namespace pdwt {

template <typename T>
struct Ext3bZJob {
    const T* src[4];   // forward: quadrant stacks (V x nin planes); inverse: z-low band stacks (V x nin planes)
    const T* src2[4];  // inverse: z-high band stacks
    T* lo[4];          // forward: z-low band stacks; inverse: quadrant stacks (V x nout planes)
    T* hi[4];          // forward: z-high band stacks
    int nin, nout, plane, mode;
    size_t pair0;      // the first (volume, quadrant) pair of the launch
};

template <typename T>
struct Adj3bZJob {
    Adj3ZJob<T> j;     // the stacks of the V volumes: lo, hi (V x hz planes), q (V x nz planes)
    size_t pair0;
};

// pair p = 4 * v + e of a launch whose grid z starts at pair0
struct X3bPair {
    size_t v;
    int e;
};
__host__ __device__ inline X3bPair x3b_pair(size_t pair0, unsigned z)
{
    const size_t p = pair0 + z;
    return X3bPair{p >> 2, (int)(p & 3)};
}
// where volume v starts in a stack of `planes` planes of pl elements per volume
__host__ __device__ inline size_t x3b_offset(size_t v, int planes, size_t pl) { return v * (size_t)planes * pl; }

// The samples g0 .. g0 + A3ZC - 1 of column k of pair pair0 + z: ext3_adj_z_lane on the stacks of that volume, as slot 0 of a job of its
// own (the slot index is then a constant: the job stays in registers).
template <typename T, int HL>
__host__ __device__ __forceinline__ void ext3b_adj_z_lane(const Adj3bZJob<T>& job, const Taps2<T>& taps, const Adj3ZHalo<T>& hm, unsigned z, int g0, int k)
{
    const X3bPair p = x3b_pair(job.pair0, z);
    const size_t pl = (size_t)job.j.plane;
    Adj3ZJob<T> one{};
    one.lo[0] = job.j.lo[p.e] + x3b_offset(p.v, job.j.hz, pl);
    one.hi[0] = job.j.hi[p.e] + x3b_offset(p.v, job.j.hz, pl);
    one.q[0] = job.j.q[p.e] + x3b_offset(p.v, job.j.nz, pl);
    one.nz = job.j.nz, one.hz = job.j.hz, one.plane = job.j.plane;
    ext3_adj_z_lane<T, HL>(one, taps, hm, 0, g0, k);
}

}  // namespace pdwt
