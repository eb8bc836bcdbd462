// dwt_ext3d_xy.hpp -- the x-y pass of dwt_ext3d.hip as other translation units see it: the job and the launch (the tile: tile_stages.hpp).
// The kernels (k_ext3_fwd_xy / k_ext3_inv_xy: the staging of dwt_ext.hpp and the stages of tile_stages.hpp on plane blockIdx.z) are
// instantiated in dwt_ext3d.hip alone;
// the batched 2-D transform (dwt_ext2db.hip) runs them with the planes = the images of a batch and the four quadrant pointers aimed at
// its band stacks.
#pragma once
#include "dwt_ext.hpp"

namespace pdwt {

template <typename T>
struct Ext3XYJob {
    const T* src;    // forward: the level's input (nz, nr, nc)
    T* dst;          // inverse: the level's output
    T* q[4];         // quadrants (nz, hr, hc): A, H, V, D of dwt_ext.hpp = 2 * x band + y band
    int nr, nc, hr, hc, mode;
};

// one launch over the nz planes: grid (tiles along x, tiles along y, nz).  The caller has checked the sizes (nz <= 65535, the rows of
// tiles a grid dimension).  Defined and instantiated for float and double in dwt_ext3d.hip.
template <typename T>
int run_ext3_xy(int hlen, bool fwd, const Ext3XYJob<T>& xy, int nz, const Taps2<T>& taps);

// what both directions refuse: the limits of the volume transforms (vol_sizes_ok: nz a grid dimension, a plane indexed with 32 bits)
// and of the 2-D level (a bad bank length, an axis shorter than hlen - 1, more rows of tiles than a grid dimension)
inline bool ext3_level_ok(int nz, int nr, int nc, int hlen)
{
    if (hlen < 2 || hlen > PDWT_MAX_FILTER_WIDTH || (hlen & 1)) return false;
    if (nz < 1 || nr < 1 || nc < 1 || nz < hlen - 1 || nr < hlen - 1 || nc < hlen - 1) return false;
    if (nz > 65535 || nr > (1 << 30) || nc > (1 << 30)) return false;
    if ((unsigned long long)nr * (unsigned long long)nc >= (1ull << 31)) return false;  // (the expanded plane is no larger: n >= hlen - 1)
    return idiv_up(ext_half(nr, hlen), TFY) <= 65535 && idiv_up(nr, TIY) <= 65535;
}

// band k (aaa, aad, ada, add, daa, dad, dda, ddd: bits z y x) of quadrant q (2 * x band + y band) and z band zb
inline int ext3_band(int q, int zb) { return 4 * zb + 2 * (q & 1) + (q >> 1); }

}  // namespace pdwt
