// dwt_ext.hip -- one level of the 2-D transform with signal-extension boundary modes (include/pdwt_hip.h "2-D DWT with boundary
// modes"; the class: include/wt_ext.h).  Unlike every other transform of the library this one does not periodise: the image is
// extended past its borders by the mode (zero, constant, symmetric, reflect, periodic: PyWavelets' names and semantics) and the
// bands have the expanded size (n + hlen - 1) / 2 per axis.  The inverse needs no extension at all.
// Two tile kernels in the shape of the packet kernels (wpt2d.hip): the staging is that of dwt_ext.hpp, the passes are the stages of
// tile_stages.hpp, which the packet and volume kernels run too:
//   k_ext_fwd  16 x 32 positions of the four bands per workgroup: stage the input window in LDS (interior tiles with plain addressing,
//              border tiles through the index map of the mode), row pass into LDS, column pass out of it, four band stores
//   k_ext_inv  32 x 64 samples of the parent per workgroup: stage the four child windows (0 past the bands), column synthesis into
//              LDS, row synthesis into the parent
// Haar (hlen 2) runs the same kernels with the bank's own taps.  Traffic per level and direction: one read of the source (plus the
// tile halos) and one write of the destination.
#include "dwt_ext.hpp"

namespace pdwt {

// The tile of tile_stages.hpp.  (tests/test_newer_bank_matrix_cpu.py reads these four from this file; the kernels use the shared constants.)
constexpr int EFX = 32, EFY = 16, EIX = 64, EIY = 32;
static_assert(EFX == TFX && EFY == TFY && EIX == TIX && EIY == TIY, "the tile shape is defined in tile_stages.hpp");

template <typename T>
struct ExtFwdJob {
    const T* src;
    T *a, *h, *v, *d;
    int nr, nc, hr, hc, mode;
};
template <typename T>
struct ExtInvJob {
    T* dst;
    const T* q[4];  // A, H, V, D
    int nr, nc, hr, hc;
};

template <typename T, int HL>
__global__ __launch_bounds__(kTileThreads) void k_ext_fwd(ExtFwdJob<T> job, Taps2<T> taps)
{
    extern __shared__ double smem_d[];  // (double: 8-byte alignment for either precision)
    constexpr int RI = tile_fwd_win(TFY, HL), CI = tile_fwd_win(TFX, HL);
    T* in = reinterpret_cast<T*>(smem_d);                  // [RI][CI]
    T* rb = in + RI * CI;                                  // [2][RI][TFX]: row pass lo | hi
    int* map = reinterpret_cast<int*>(rb + 2 * RI * TFX);  // [RI + CI]: border tiles only
    const int tid = threadIdx.x;
    const int ox0 = blockIdx.x * TFX, oy0 = blockIdx.y * TFY;
    // position i reads xe[2i + 1 - k], k = 0 .. HL-1: the window of the tile starts at 2 * o0 + 1 - (HL - 1)
    ext_stage_window<T, RI, CI, kTileThreads>(in, map, job.src, job.nr, job.nc, 2 * oy0 + 2 - HL, 2 * ox0 + 2 - HL, job.mode, tid);
    tile_rows_analysis<T, HL, RI, CI, TFX, kTileThreads>(in, rb, taps, tid);
    tile_cols_analysis_write<T, HL, RI, TFX, TFY, kTileThreads>(rb, taps, job.a, job.h, job.v, job.d, job.hr, job.hc, oy0, ox0, tid);
}

template <typename T, int HL>
__global__ __launch_bounds__(kTileThreads) void k_ext_inv(ExtInvJob<T> job, Taps2<T> taps)
{
    extern __shared__ double smem_d[];
    constexpr int WR = tile_inv_win(TIY, HL, false), WC = tile_inv_win(TIX, HL, false);
    T* in = reinterpret_cast<T*>(smem_d);  // [4][WR][WC]
    T* cb = in + 4 * WR * WC;              // [2][TIY][WC]
    const int tid = threadIdx.x;
    const int g0x = blockIdx.x * TIX, g0y = blockIdx.y * TIY;  // even
    ext_stage_children<T, WR, WC, kTileThreads>(in, job.q, job.hr, job.hc, g0y / 2, g0x / 2, tid);
    tile_cols_synthesis<T, HL, 0, WR, WC, TIY, kTileThreads>(in, cb, taps, tid);
    tile_rows_synthesis_write<T, HL, 0, WC, TIY, TIX, kTileThreads>(cb, taps, job.dst, job.nr, job.nc, g0y, g0x, tid);
}

// ---- drivers -----------------------------------------------------------------------------------------------------------------
template <typename T, int HL>
static int launch_ext_fwd(const ExtFwdJob<T>& job, const Taps2<T>& taps)
{
    constexpr size_t lds = tile_fwd_lds<T, HL>(true);
    if (lds > 64 * 1024)
        if (const int rc = lds_opt_in_ptr((const void*)k_ext_fwd<T, HL>); rc != PDWT_OK) return rc;
    hipLaunchKernelGGL((k_ext_fwd<T, HL>), dim3(idiv_up(job.hc, TFX), idiv_up(job.hr, TFY)), dim3(kTileThreads), lds, stream(), job, taps);
    PDWT_HIP_TRY(hipGetLastError());
    return PDWT_OK;
}
template <typename T, int HL>
static int launch_ext_inv(const ExtInvJob<T>& job, const Taps2<T>& taps)
{
    constexpr size_t lds = tile_inv_lds<T, HL>(false);
    if (lds > 64 * 1024)
        if (const int rc = lds_opt_in_ptr((const void*)k_ext_inv<T, HL>); rc != PDWT_OK) return rc;
    hipLaunchKernelGGL((k_ext_inv<T, HL>), dim3(idiv_up(job.nc, TIX), idiv_up(job.nr, TIY)), dim3(kTileThreads), lds, stream(), job, taps);
    PDWT_HIP_TRY(hipGetLastError());
    return PDWT_OK;
}

// what both directions refuse: a bad bank length, a line shorter than hlen - 1 (the halo of hlen - 2 samples must fold once), sizes
// the 32-bit indices or the grid cannot take
static bool ext_level_ok(int nr, int nc, int hlen)
{
    if (hlen < 2 || hlen > PDWT_MAX_FILTER_WIDTH || (hlen & 1)) return false;
    if (nr < 1 || nc < 1 || nr < hlen - 1 || nc < hlen - 1 || nr > (1 << 30) || nc > (1 << 30)) return false;
    if ((unsigned long long)nr * (unsigned long long)nc >= (1ull << 31)) return false;
    // rows of tiles are a grid dimension, in either direction
    return idiv_up(ext_half(nr, hlen), TFY) <= 65535 && idiv_up(nr, TIY) <= 65535;
}

template <typename T>
static int ext_forward_level(const T* src, T* a, T* h, T* v, T* d, int nr, int nc, int mode, const typename FiltersOf<T>::type* f)
{
    if (!src || !a || !h || !v || !d || !f || mode < 0 || mode >= EXT_NUM_MODES || !ext_level_ok(nr, nc, f->hlen)) return PDWT_EINVAL;
    const int hlen = f->hlen;
    const ExtFwdJob<T> job{src, a, h, v, d, nr, nc, ext_half(nr, hlen), ext_half(nc, hlen), mode};
    const Taps2<T> taps = taps_fwd<T>(f);
    return with_filter_length<2>(hlen, [&](auto hl) { return launch_ext_fwd<T, decltype(hl)::value>(job, taps); });
}

template <typename T>
static int ext_inverse_level(T* dst, const T* a, const T* h, const T* v, const T* d, int nr, int nc, const typename FiltersOf<T>::type* f)
{
    if (!dst || !a || !h || !v || !d || !f || !ext_level_ok(nr, nc, f->hlen)) return PDWT_EINVAL;
    const int hlen = f->hlen;
    const ExtInvJob<T> job{dst, {a, h, v, d}, nr, nc, ext_half(nr, hlen), ext_half(nc, hlen)};
    const Taps2<T> taps = taps_inv<T>(f);
    return with_filter_length<2>(hlen, [&](auto hl) { return launch_ext_inv<T, decltype(hl)::value>(job, taps); });
}

}  // namespace pdwt

using namespace pdwt;

extern "C" {
int pdwt_num_bands_ext(int Nr, int Nc, int hlen, int levels)
{
    if (levels < 1 || levels > 32 || !ext_level_ok(Nr, Nc, hlen)) return PDWT_EINVAL;
    return 3 * levels + 1;
}
long long pdwt_ext_band_shape(int Nr, int Nc, int hlen, int levels, int num, int* band_Nr, int* band_Nc)
{
    const int nb = pdwt_num_bands_ext(Nr, Nc, hlen, levels);
    if (nb < 0 || num < 0 || num >= nb) return PDWT_EINVAL;
    const int lev = num == 0 ? levels : (num - 1) / 3 + 1;  // [A_L, H1, V1, D1, ..., H_L, V_L, D_L]
    for (int l = 0; l < lev; l++) Nr = ext_half(Nr, hlen), Nc = ext_half(Nc, hlen);
    if (band_Nr) *band_Nr = Nr;
    if (band_Nc) *band_Nc = Nc;
    return (long long)Nr * Nc;
}
int pdwt_ext2d_forward_level_f32(const float* d_src, float* d_a, float* d_h, float* d_v, float* d_d, int nr, int nc, int mode, const pdwt_filters_f32* f)
{
    return ext_forward_level<float>(d_src, d_a, d_h, d_v, d_d, nr, nc, mode, f);
}
int pdwt_ext2d_forward_level_f64(const double* d_src, double* d_a, double* d_h, double* d_v, double* d_d, int nr, int nc, int mode, const pdwt_filters_f64* f)
{
    return ext_forward_level<double>(d_src, d_a, d_h, d_v, d_d, nr, nc, mode, f);
}
int pdwt_ext2d_inverse_level_f32(float* d_dst, const float* d_a, const float* d_h, const float* d_v, const float* d_d, int nr, int nc, const pdwt_filters_f32* f)
{
    return ext_inverse_level<float>(d_dst, d_a, d_h, d_v, d_d, nr, nc, f);
}
int pdwt_ext2d_inverse_level_f64(double* d_dst, const double* d_a, const double* d_h, const double* d_v, const double* d_d, int nr, int nc, const pdwt_filters_f64* f)
{
    return ext_inverse_level<double>(d_dst, d_a, d_h, d_v, d_d, nr, nc, f);
}
}
