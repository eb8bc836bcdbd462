// dwt_ext3d.hip -- one level of the 3-D transform of volumes with signal-extension boundary modes (include/pdwt_hip.h "3-D DWT with
// boundary modes"; the class: BoundaryWavelets3D, include/wt_ext.h).  The one-axis formula of dwt_ext.hpp along x, then y, then z: a
// level takes an nz x nr x nc approximation to eight bands of ((nz + F - 1) / 2) x ((nr + F - 1) / 2) x ((nc + F - 1) / 2); the inverse
// runs z, y, x and needs no extension and no mode.  Two launches per level and direction, in the shape of dwt3d.hip:
//   forward   x-y: volume (nz, nr, nc) -> 4 quadrants (nz, hr, hc) in d_tmp    the tile stages of tile_stages.hpp, blockIdx.z = the plane
//             z:   4 quadrants         -> the 8 bands (hz, hr, hc)            k_z_analysis / k_z_synthesis of z_stages.hpp (boundary modes, ZJob)
//   inverse   z first (bands -> quadrants), then x-y (quadrants -> volume).
// A forward launch reads the extension only through ext_index.  Per output the tap order and the one-FMA-per-tap accumulation are
// those of dwt_ext.hip (x-y) and of the z kernels of z_stages.hpp (z).  Haar runs the bank's own taps.  Every access is a scalar
// element access: buffers need only be aligned to their element type.
// Traffic per level and direction: one read of the input (plus the tile halos) and one write of the quadrants, then one read of the
// quadrants and one write of the bands.
#include "dwt_ext3d_level.hpp"

namespace pdwt {

// (Ext3XYJob: dwt_ext3d_xy.hpp; the z jobs and kernels: z_stages.hpp)

// ---- x-y passes: the staging of dwt_ext.hpp and the stages of tile_stages.hpp on plane blockIdx.z ------------------------------------
template <typename T, int HL>
__global__ __launch_bounds__(kTileThreads) void k_ext3_fwd_xy(Ext3XYJob<T> job, Taps2<T> taps)
{
    extern __shared__ double smem_d[];  // (double: 8-byte alignment for either precision)
    constexpr int RI = tile_fwd_win(TFY, HL), CI = tile_fwd_win(TFX, HL);
    T* in = reinterpret_cast<T*>(smem_d);                  // [RI][CI]
    T* rb = in + RI * CI;                                  // [2][RI][TFX]: row pass lo | hi
    int* map = reinterpret_cast<int*>(rb + 2 * RI * TFX);  // [RI + CI]: border tiles only
    const int tid = threadIdx.x;
    const int ox0 = blockIdx.x * TFX, oy0 = blockIdx.y * TFY;
    const T* plane = job.src + (size_t)blockIdx.z * job.nr * job.nc;
    const size_t zoff = (size_t)blockIdx.z * job.hr * job.hc;
    ext_stage_window<T, RI, CI, kTileThreads>(in, map, plane, job.nr, job.nc, 2 * oy0 + 2 - HL, 2 * ox0 + 2 - HL, job.mode, tid);
    tile_rows_analysis<T, HL, RI, CI, TFX, kTileThreads>(in, rb, taps, tid);
    tile_cols_analysis_write<T, HL, RI, TFX, TFY, kTileThreads>(rb, taps, job.q[0] + zoff, job.q[1] + zoff, job.q[2] + zoff, job.q[3] + zoff, job.hr, job.hc,
                                                                oy0, ox0, tid);
}

template <typename T, int HL>
__global__ __launch_bounds__(kTileThreads) void k_ext3_inv_xy(Ext3XYJob<T> job, Taps2<T> taps)
{
    extern __shared__ double smem_d[];
    constexpr int WR = tile_inv_win(TIY, HL, false), WC = tile_inv_win(TIX, HL, false);
    T* in = reinterpret_cast<T*>(smem_d);  // [4][WR][WC]
    T* cb = in + 4 * WR * WC;              // [2][TIY][WC]
    const int tid = threadIdx.x;
    const int g0x = blockIdx.x * TIX, g0y = blockIdx.y * TIY;  // even
    const size_t zoff = (size_t)blockIdx.z * job.hr * job.hc;
    const T* const q[4] = {job.q[0] + zoff, job.q[1] + zoff, job.q[2] + zoff, job.q[3] + zoff};
    ext_stage_children<T, WR, WC, kTileThreads>(in, q, job.hr, job.hc, g0y / 2, g0x / 2, tid);
    tile_cols_synthesis<T, HL, 0, WR, WC, TIY, kTileThreads>(in, cb, taps, tid);
    tile_rows_synthesis_write<T, HL, 0, WC, TIY, TIX, kTileThreads>(cb, taps, job.dst + (size_t)blockIdx.z * job.nr * job.nc, job.nr, job.nc, g0y, g0x, tid);
}

// ---- launches ----------------------------------------------------------------------------------------------------------------------
template <typename T, int HL>
static int launch_ext3_xy(bool fwd, const Ext3XYJob<T>& xy, int nz, const Taps2<T>& taps)
{
    const size_t lds = fwd ? tile_fwd_lds<T, HL>(true) : tile_inv_lds<T, HL>(false);
    const dim3 grid = fwd ? dim3(idiv_up(xy.hc, TFX), idiv_up(xy.hr, TFY), nz) : dim3(idiv_up(xy.nc, TIX), idiv_up(xy.nr, TIY), nz);
    return launch_lds(fwd ? k_ext3_fwd_xy<T, HL> : k_ext3_inv_xy<T, HL>, grid, dim3(kTileThreads), lds, xy, taps);
}

// (external linkage: dwt_ext2db.hip runs the same instantiations on the images of a batch)
template <typename T>
int run_ext3_xy(int hlen, bool fwd, const Ext3XYJob<T>& xy, int nz, const Taps2<T>& taps)
{
    return with_filter_length(hlen, [&](auto hl) { return launch_ext3_xy<T, decltype(hl)::value>(fwd, xy, nz, taps); });
}
template int run_ext3_xy<float>(int, bool, const Ext3XYJob<float>&, int, const Taps2<float>&);
template int run_ext3_xy<double>(int, bool, const Ext3XYJob<double>&, int, const Taps2<double>&);

// (ext3_level_ok, what both directions refuse, and ext3_band, the band of a quadrant: dwt_ext3d_xy.hpp)

template <typename T>
static int ext3_forward_level(const T* src, T* const* b, int nz, int nr, int nc, int mode, const typename FiltersOf<T>::type* f, T* tmp)
{
    if (!src || !b || !f || !tmp || mode < 0 || mode >= EXT_NUM_MODES || !ext3_level_ok(nz, nr, nc, f->hlen)) return PDWT_EINVAL;
    for (int k = 0; k < 8; k++)
        if (!b[k]) return PDWT_EINVAL;
    // (the quadrants at the start of the scratch; the step: dwt_ext3d_level.hpp)
    return ext3_forward_step<false, T>(Ext3Step<T>{1, nz, nr, nc, f->hlen, tmp}, src, b, mode, taps_fwd<T>(f));
}

template <typename T>
static int ext3_inverse_level(T* dst, T* const* b, int nz, int nr, int nc, const typename FiltersOf<T>::type* f, T* tmp)
{
    if (!dst || !b || !f || !tmp || !ext3_level_ok(nz, nr, nc, f->hlen)) return PDWT_EINVAL;
    for (int k = 0; k < 8; k++)
        if (!b[k]) return PDWT_EINVAL;
    return ext3_inverse_step<false, T>(Ext3Step<T>{1, nz, nr, nc, f->hlen, tmp}, dst, b, taps_inv<T>(f));
}

}  // namespace pdwt

using namespace pdwt;

extern "C" {
int pdwt_num_bands_ext3d(int Nz, int Nr, int Nc, int hlen, int levels)
{
    if (levels < 1 || levels > kVolMaxLevels || !ext3_level_ok(Nz, Nr, Nc, hlen)) return PDWT_EINVAL;
    return 7 * levels + 1;
}
long long pdwt_ext3d_band_shape(int Nz, int Nr, int Nc, int hlen, int levels, int num, int* band_Nz, int* band_Nr, int* band_Nc)
{
    const int nb = pdwt_num_bands_ext3d(Nz, Nr, Nc, hlen, levels);
    if (nb < 0 || num < 0 || num >= nb) return PDWT_EINVAL;
    const int lev = num == 0 ? levels : levels - (num - 1) / 7;  // [A_L, level L ... level 1]
    for (int l = 0; l < lev; l++) Nz = ext_half(Nz, hlen), Nr = ext_half(Nr, hlen), Nc = ext_half(Nc, hlen);
    if (band_Nz) *band_Nz = Nz;
    if (band_Nr) *band_Nr = Nr;
    if (band_Nc) *band_Nc = Nc;
    return (long long)Nz * Nr * Nc;
}
// the scratch of an instance: [the four quadrants of level 1 | one level-1 approximation], each padded as tmp3 of dwt3d.hip does
long long pdwt_ext3d_tmp_approx_offset(int Nz, int Nr, int Nc, int hlen)
{
    if (!ext3_level_ok(Nz, Nr, Nc, hlen)) return PDWT_EINVAL;
    return (long long)pad64(4 * (size_t)Nz * ext_half(Nr, hlen) * ext_half(Nc, hlen));
}
long long pdwt_ext3d_tmp_elems(int Nz, int Nr, int Nc, int hlen)
{
    const long long off = pdwt_ext3d_tmp_approx_offset(Nz, Nr, Nc, hlen);
    if (off < 0) return PDWT_EINVAL;
    return off + (long long)pad64((size_t)ext_half(Nz, hlen) * ext_half(Nr, hlen) * ext_half(Nc, hlen));
}
int pdwt_ext3d_forward_level_f32(const float* d_src, float* const* d_bands, int nz, int nr, int nc, int mode, const pdwt_filters_f32* f, float* d_tmp)
{
    return ext3_forward_level<float>(d_src, d_bands, nz, nr, nc, mode, f, d_tmp);
}
int pdwt_ext3d_forward_level_f64(const double* d_src, double* const* d_bands, int nz, int nr, int nc, int mode, const pdwt_filters_f64* f, double* d_tmp)
{
    return ext3_forward_level<double>(d_src, d_bands, nz, nr, nc, mode, f, d_tmp);
}
int pdwt_ext3d_inverse_level_f32(float* d_dst, float* const* d_bands, int nz, int nr, int nc, const pdwt_filters_f32* f, float* d_tmp)
{
    return ext3_inverse_level<float>(d_dst, d_bands, nz, nr, nc, f, d_tmp);
}
int pdwt_ext3d_inverse_level_f64(double* d_dst, double* const* d_bands, int nz, int nr, int nc, const pdwt_filters_f64* f, double* d_tmp)
{
    return ext3_inverse_level<double>(d_dst, d_bands, nz, nr, nc, f, d_tmp);
}
}
