// dwt_ext3d.hip -- one level of the 3-D transform of volumes with signal-extension boundary modes (include/pdwt_hip.h "3-D DWT with
// boundary modes"; the class: BoundaryWavelets3D, include/wt_ext.h).  The one-axis formula of dwt_ext.hpp along x, then y, then z: a
// level takes an nz x nr x nc approximation to eight bands of ((nz + F - 1) / 2) x ((nr + F - 1) / 2) x ((nc + F - 1) / 2); the inverse
// runs z, y, x and needs no extension and no mode.  Two launches per level and direction, in the shape of dwt3d.hip:
//   forward   x-y: volume (nz, nr, nc) -> 4 quadrants (nz, hr, hc) in d_tmp    the tile stages of tile_stages.hpp, blockIdx.z = the plane
//             z:   4 quadrants         -> the 8 bands (hz, hr, hc)            lanes across an expanded plane, 16 outputs per thread along z
//   inverse   z first (bands -> quadrants), then x-y (quadrants -> volume).
// A forward launch reads the extension only through ext_index.  Per output the tap order and the one-FMA-per-tap accumulation are
// those of dwt_ext.hip (x-y) and of k_ana_z / k_syn_z of dwt3d.hip (z).  Haar runs the bank's own taps.  Every access is a scalar
// element access: buffers need only be aligned to their element type.
// Traffic per level and direction: one read of the input (plus the tile halos) and one write of the quadrants, then one read of the
// quadrants and one write of the bands.
#include "dwt_ext3d_xy.hpp"

namespace pdwt {

// (Ext3XYJob: dwt_ext3d_xy.hpp)
constexpr int kX3ZThreads = 256;
constexpr int X3ZC = 16;             // outputs per thread along z

template <typename T>
struct Ext3ZJob {
    const T* src[4];   // forward: quadrants (nin planes); inverse: z-low bands (nin planes)
    const T* src2[4];  // inverse: z-high bands
    T* lo[4];          // forward: z-low bands; inverse: quadrants
    T* hi[4];          // forward: z-high bands
    int nin, nout, plane, mode;
};

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

// ---- z passes: X3ZC outputs per thread along z from a register window --------------------------------------------------------------
// Lanes run across an expanded plane (coalesced), blockIdx.y = chunk of X3ZC outputs along z, blockIdx.z = quadrant.  (Written here
// like the z kernels of dwt3d.hip, and for the reason given there.)
// Analysis: output i reads xe[2i + 1 - k], k = 0 .. HL-1, so the window of the chunk from i0 holds the 2 * X3ZC + HL - 2 planes from
// the extended index 2 * i0 + 2 - HL; each plane index goes through ext_index (-1: the plane is 0).  A chunk whose window lies inside
// the volume skips the map (a workgroup-uniform branch).
template <typename T, int HL>
__global__ __launch_bounds__(kX3ZThreads) void k_ext3_ana_z(Ext3ZJob<T> job, Taps2<T> taps)
{
    const int k = blockIdx.x * kX3ZThreads + threadIdx.x;
    if (k >= job.plane) return;
    const int e = blockIdx.z, i0 = blockIdx.y * X3ZC;
    constexpr int W = 2 * X3ZC + HL - 2;
    const int n = job.nin, s0 = 2 * i0 + 2 - HL;
    const size_t pl = (size_t)job.plane;
    const T* __restrict__ x = job.src[e] + k;
    T v[W];
    if (s0 >= 0 && s0 + W <= n) {
#pragma unroll
        for (int w = 0; w < W; w++) v[w] = x[(size_t)(s0 + w) * pl];
    } else {
#pragma unroll
        for (int w = 0; w < W; w++) {
            const int s = ext_index(s0 + w, n, job.mode);
            v[w] = s < 0 ? T(0) : x[(size_t)s * pl];
        }
    }
    T* __restrict__ lo = job.lo[e] + k;
    T* __restrict__ hi = job.hi[e] + k;
#pragma unroll
    for (int u = 0; u < X3ZC; u++) {
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

// Synthesis: sample k reads the coefficients (k >> 1) + m, m < HL/2, with the taps HL-2-2m (k even) / HL-1-2m (k odd); no wrap.  The
// chunk of X3ZC samples from the even g0 reads the X3ZC/2 + HL/2 - 1 coefficient planes from g0 / 2; planes past the band are loaded
// as 0 (only in the overhang of the last chunk, whose samples are not stored).
template <typename T, int HL>
__global__ __launch_bounds__(kX3ZThreads) void k_ext3_syn_z(Ext3ZJob<T> job, Taps2<T> taps)
{
    const int k = blockIdx.x * kX3ZThreads + threadIdx.x;
    if (k >= job.plane) return;
    const int e = blockIdx.z, g0 = blockIdx.y * X3ZC;  // even
    constexpr int h2 = HL / 2, W = X3ZC / 2 + h2 - 1;
    const int nin = job.nin, q0 = g0 / 2;
    const size_t pl = (size_t)job.plane;
    const T* __restrict__ a = job.src[e] + k;
    const T* __restrict__ d = job.src2[e] + k;
    T va[W], vd[W];
#pragma unroll
    for (int w = 0; w < W; w++) {
        const bool in = q0 + w < nin;
        const size_t s = (size_t)(q0 + w) * pl;
        va[w] = in ? a[s] : T(0);
        vd[w] = in ? d[s] : T(0);
    }
    T* __restrict__ out = job.lo[e] + k;
#pragma unroll
    for (int u = 0; u < X3ZC; u++) {
        if (g0 + u < job.nout) {
            const int lp = u >> 1, odd = u & 1;  // compile-time after unrolling
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

// ---- launches ----------------------------------------------------------------------------------------------------------------------
template <typename T, int HL>
static int launch_ext3_xy(bool fwd, const Ext3XYJob<T>& xy, int nz, const Taps2<T>& taps)
{
    const size_t lds = fwd ? tile_fwd_lds<T, HL>(true) : tile_inv_lds<T, HL>(false);
    const dim3 grid = fwd ? dim3(idiv_up(xy.hc, TFX), idiv_up(xy.hr, TFY), nz) : dim3(idiv_up(xy.nc, TIX), idiv_up(xy.nr, TIY), nz);
    return launch_lds(fwd ? k_ext3_fwd_xy<T, HL> : k_ext3_inv_xy<T, HL>, grid, dim3(kTileThreads), lds, xy, taps);
}
template <typename T, int HL>
static int launch_ext3_z(bool fwd, const Ext3ZJob<T>& zj, const Taps2<T>& taps)
{
    const dim3 grid(idiv_up(zj.plane, kX3ZThreads), idiv_up(zj.nout, X3ZC), 4);
    return launch_lds(fwd ? k_ext3_ana_z<T, HL> : k_ext3_syn_z<T, HL>, grid, dim3(kX3ZThreads), 0, zj, taps);
}

// (external linkage: dwt_ext2db.hip runs the same instantiations on the images of a batch)
template <typename T>
int run_ext3_xy(int hlen, bool fwd, const Ext3XYJob<T>& xy, int nz, const Taps2<T>& taps)
{
    return with_filter_length(hlen, [&](auto hl) { return launch_ext3_xy<T, decltype(hl)::value>(fwd, xy, nz, taps); });
}
template int run_ext3_xy<float>(int, bool, const Ext3XYJob<float>&, int, const Taps2<float>&);
template int run_ext3_xy<double>(int, bool, const Ext3XYJob<double>&, int, const Taps2<double>&);
template <typename T>
static int run_ext3_z(int hlen, bool fwd, const Ext3ZJob<T>& zj, const Taps2<T>& taps)
{
    return with_filter_length(hlen, [&](auto hl) { return launch_ext3_z<T, decltype(hl)::value>(fwd, zj, taps); });
}

// (ext3_level_ok, what both directions refuse, and ext3_band, the band of a quadrant: dwt_ext3d_xy.hpp)

template <typename T>
static int ext3_forward_level(const T* src, T* const* b, int nz, int nr, int nc, int mode, const typename FiltersOf<T>::type* f, T* tmp)
{
    if (!src || !b || !f || !tmp || mode < 0 || mode >= EXT_NUM_MODES || !ext3_level_ok(nz, nr, nc, f->hlen)) return PDWT_EINVAL;
    for (int k = 0; k < 8; k++)
        if (!b[k]) return PDWT_EINVAL;
    const int hlen = f->hlen, hz = ext_half(nz, hlen), hr = ext_half(nr, hlen), hc = ext_half(nc, hlen);
    const size_t sq = (size_t)nz * hr * hc;
    Ext3XYJob<T> xy{};
    Ext3ZJob<T> zj{};
    xy.src = src;
    xy.nr = nr, xy.nc = nc, xy.hr = hr, xy.hc = hc, xy.mode = mode;
    for (int q = 0; q < 4; q++) {
        xy.q[q] = tmp + q * sq;
        zj.src[q] = tmp + q * sq;
        zj.lo[q] = b[ext3_band(q, 0)];
        zj.hi[q] = b[ext3_band(q, 1)];
    }
    zj.nin = nz, zj.nout = hz, zj.plane = hr * hc, zj.mode = mode;
    const Taps2<T> taps = taps_fwd<T>(f);
    // x-y into the quadrants (reads the input), then z into the bands (band aaa may be the input's own buffer: already read)
    if (const int rc = run_ext3_xy<T>(hlen, true, xy, nz, taps); rc != PDWT_OK) return rc;
    return run_ext3_z<T>(hlen, true, zj, taps);
}

template <typename T>
static int ext3_inverse_level(T* dst, T* const* b, int nz, int nr, int nc, const typename FiltersOf<T>::type* f, T* tmp)
{
    if (!dst || !b || !f || !tmp || !ext3_level_ok(nz, nr, nc, f->hlen)) return PDWT_EINVAL;
    for (int k = 0; k < 8; k++)
        if (!b[k]) return PDWT_EINVAL;
    const int hlen = f->hlen, hz = ext_half(nz, hlen), hr = ext_half(nr, hlen), hc = ext_half(nc, hlen);
    const size_t sq = (size_t)nz * hr * hc;
    Ext3XYJob<T> xy{};
    Ext3ZJob<T> zj{};
    xy.dst = dst;
    xy.nr = nr, xy.nc = nc, xy.hr = hr, xy.hc = hc, xy.mode = 0;
    for (int q = 0; q < 4; q++) {
        zj.src[q] = b[ext3_band(q, 0)];
        zj.src2[q] = b[ext3_band(q, 1)];
        zj.lo[q] = tmp + q * sq;
        xy.q[q] = tmp + q * sq;
    }
    zj.nin = hz, zj.nout = nz, zj.plane = hr * hc, zj.mode = 0;
    const Taps2<T> taps = taps_inv<T>(f);
    // z into the quadrants (reads the bands), then x-y into the output (may be the buffer of band aaa: already read)
    if (const int rc = run_ext3_z<T>(hlen, false, zj, taps); rc != PDWT_OK) return rc;
    return run_ext3_xy<T>(hlen, false, xy, nz, taps);
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
