// dwt_ext3d_adj.hip -- the adjoint operators of one level of the 3-D transform with signal-extension boundary modes (include/pdwt_hip.h
// "Adjoints of the 3-D boundary-mode DWT"): what a gradient method needs of pdwt_ext3d_forward_level_* / pdwt_ext3d_inverse_level_*.
//   adjoint of the forward (a mode): the forward runs x-y, then z, so the adjoint runs z, then x-y
//     k_z_adjoint          the eight cotangent bands -> the four quadrant cotangents (nz, hr, hc) in scratch: the geometry of the synthesis
//                          (lanes across the expanded plane, blockIdx.y = a chunk of 16 samples along z, blockIdx.z = the quadrant) with
//                          the reversed analysis taps, and the fold of the extension along z in the same launch (z_stages.hpp, Adj3ZJob)
//     adj2_forward_level   the 2-D level adjoint of dwt_ext_adj.hip on B = nz planes: the quadrants are its A, H, V, D stacks
//   adjoint of the inverse (no mode): the forward level in mode zero with the bank L' = reversed IL, H' = reversed IH; no kernel.
// Traffic of the z pass per level: the eight band stacks read once, the four quadrant stacks written once; a border chunk re-reads at
// most (2F - 3) F band elements per column.
#include "dwt_ext3d_level.hpp"

namespace pdwt {

static bool adj3_level_ok(int nz, int nr, int nc, int hlen) { return ext3_level_ok(nz, nr, nc, hlen) && adj2_level_ok(nz, nr, nc, hlen); }

// scratch of a level: [the four quadrant cotangents, padded | the frames of the nz planes of the x-y adjoint]
static size_t adj3_quad_elems(int nz, int nr, int nc, int hlen) { return pad64(4 * (size_t)nz * ext_half(nr, hlen) * ext_half(nc, hlen)); }

template <typename T>
static int adj3_forward_level(T* dst, T* const* b, int nz, int nr, int nc, int mode, const typename FiltersOf<T>::type* f, T* tmp)
{
    if (!dst || !b || !f || !tmp || mode < 0 || mode >= EXT_NUM_MODES || !adj3_level_ok(nz, nr, nc, f->hlen)) return PDWT_EINVAL;
    for (int k = 0; k < 8; k++)
        if (!b[k]) return PDWT_EINVAL;
    return ext3_adjoint_step<false, T>(Ext3Step<T>{1, nz, nr, nc, f->hlen, tmp}, dst, b, mode, f, taps_adj<T>(f), tmp + adj3_quad_elems(nz, nr, nc, f->hlen));
}

}  // namespace pdwt

using namespace pdwt;

extern "C" {
long long pdwt_ext3d_adjoint_level_tmp_elems(int nz, int nr, int nc, int hlen)
{
    if (!adj3_level_ok(nz, nr, nc, hlen)) return PDWT_EINVAL;
    return (long long)adj3_quad_elems(nz, nr, nc, hlen) + (long long)nz * (long long)adj_frame_elems(nr, nc, hlen);
}
int pdwt_ext3d_adjoint_z_run(int nz, int hlen, int mode, int* z0, int* z1)
{
    if (hlen < 2 || hlen > PDWT_MAX_FILTER_WIDTH || (hlen & 1) || nz < 1 || nz < hlen - 1 || nz > 65535 || mode < 0 || mode >= EXT_NUM_MODES) return PDWT_EINVAL;
    const Adj3ZHalo<float> hm = adj3_z_halo<float>(nz, hlen, mode, Taps2<float>{});
    if (z0) *z0 = hm.z0;
    if (z1) *z1 = hm.z1;
    return PDWT_OK;
}
int pdwt_ext3d_forward_adjoint_level_f32(float* d_dst, float* const* d_bands, int nz, int nr, int nc, int mode, const pdwt_filters_f32* f, float* d_tmp)
{
    return adj3_forward_level<float>(d_dst, d_bands, nz, nr, nc, mode, f, d_tmp);
}
int pdwt_ext3d_forward_adjoint_level_f64(double* d_dst, double* const* d_bands, int nz, int nr, int nc, int mode, const pdwt_filters_f64* f, double* d_tmp)
{
    return adj3_forward_level<double>(d_dst, d_bands, nz, nr, nc, mode, f, d_tmp);
}
int pdwt_ext3d_inverse_adjoint_level_f32(const float* d_src, float* const* d_bands, int nz, int nr, int nc, const pdwt_filters_f32* f, float* d_tmp)
{
    pdwt_filters_f32 g;
    if (!adj_inverse_bank<float>(g, f) || !adj3_level_ok(nz, nr, nc, f->hlen)) return PDWT_EINVAL;
    return pdwt_ext3d_forward_level_f32(d_src, d_bands, nz, nr, nc, EXT_ZERO, &g, d_tmp);
}
int pdwt_ext3d_inverse_adjoint_level_f64(const double* d_src, double* const* d_bands, int nz, int nr, int nc, const pdwt_filters_f64* f, double* d_tmp)
{
    pdwt_filters_f64 g;
    if (!adj_inverse_bank<double>(g, f) || !adj3_level_ok(nz, nr, nc, f->hlen)) return PDWT_EINVAL;
    return pdwt_ext3d_forward_level_f64(d_src, d_bands, nz, nr, nc, EXT_ZERO, &g, d_tmp);
}
}
