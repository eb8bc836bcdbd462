// dwt3d.hip -- the separable, decimated, periodised 3-D DWT (include/pdwt_hip.h "3-D separable DWT").
//
// One level = the reference's 1-D level (SURVEY A-1 / A-2: the decimating analysis and the zero-stuffing synthesis of
// oracle/pdwt_oracle_impl.h ana_lines / syn_lines) along x, then y, then z, in TWO launches per level and direction:
//   forward   x-y: volume (z, y, x) -> 4 quadrants (z, hy, hx) in d_tmp    one plane tile per workgroup, rows and columns in LDS
//             z:   4 quadrants      -> the 8 bands (hz, hy, hx)           lanes across a plane, 16 outputs per thread along z
//   inverse   z first (bands -> quadrants), then x-y (quadrants -> volume).
// The x-y kernels are the shared tile stages of tile_stages.hpp (with the packet and the boundary-mode tile kernels) on one plane; the
// z kernels are those of z_stages.hpp (with the boundary-mode volume transforms), instantiated here for the periodised window.
// Per output sample the tap order and the one-FMA-per-tap accumulation are the oracle's: the 3-D result is bit-identical to
// composing the 1-D level along the axes (Haar excepted, within 1 ulp: the oracle's 1-D Haar level scales a +- b in double).
// Traffic per level: one read of the input (plus the tile halos) and one write of the quadrants, then one read of the quadrants
// and one write of the bands -- twice the compulsory bytes of a fully fused level.
#include "z_stages.hpp"

namespace pdwt {

// ---- x-y level: one plane tile per workgroup ------------------------------------------------------------
// Forward: a workgroup owns TFY x TFX output positions (half resolution) of one plane z.  It stages the input rows / columns the tile
// needs (with the periodic halo, wrap_ext per sample index) in LDS, runs the row pass into an LDS buffer (lo | hi per row) and the
// column pass out of it, and writes the four quadrants (x band, y band) of the tile: one read of the plane (plus halo) and one write
// of its four quadrants.  Inverse: TIY x TIX output samples of one plane; the windows of the four quadrants staged with wrap_per, the
// synthesis along y into an LDS buffer (x low | x high), then along x into the output.  The stages and their summation order (the
// oracle's row, then column; its syn_lines rule): tile_stages.hpp.
template <typename T>
struct XYJob {
    const T* src;     // forward: the level's input volume (z, ny, nx); inverse: unused
    T* dst;           // inverse: the level's output volume; forward: unused
    T* q[4];          // quadrants (z, hy, hx): index 2 * x band + y band (0 = low-pass)
    int nx, ny, hx, hy;
};

template <typename T, int HL>
__global__ __launch_bounds__(kTileThreads) void k_fwd_xy(XYJob<T> job, Taps2<T> taps)
{
    extern __shared__ double smem_d[];  // (double: 8-byte alignment for either precision)
    constexpr int RI = tile_fwd_win(TFY, HL), CI = tile_fwd_win(TFX, HL), c = HL / 2 - 1;
    T* in = reinterpret_cast<T*>(smem_d);  // [RI][CI]
    T* rb = in + RI * CI;                  // [2][RI][TFX]: row pass lo | hi
    const int tid = threadIdx.x, z = blockIdx.z;
    const int ox0 = blockIdx.x * TFX, oy0 = blockIdx.y * TFY;
    const size_t zoff = (size_t)z * job.hy * job.hx;
    tile_stage_window_per<T, RI, CI, kTileThreads>(in, job.src + (size_t)z * job.ny * job.nx, job.ny, job.nx, 2 * oy0 - c, 2 * ox0 - c, tid);
    tile_rows_analysis<T, HL, RI, CI, TFX, kTileThreads>(in, rb, taps, tid);
    tile_cols_analysis_write<T, HL, RI, TFX, TFY, kTileThreads>(rb, taps, job.q[0] + zoff, job.q[1] + zoff, job.q[2] + zoff, job.q[3] + zoff, job.hy, job.hx,
                                                                oy0, ox0, tid);
}

template <typename T, int HL>
__global__ __launch_bounds__(kTileThreads) void k_inv_xy(XYJob<T> job, Taps2<T> taps)
{
    extern __shared__ double smem_d[];
    constexpr int c = HL / 4, SH = syn_shift(HL);
    constexpr int WR = tile_inv_win(TIY, HL, true), WC = tile_inv_win(TIX, HL, true);
    T* in = reinterpret_cast<T*>(smem_d);  // [4][WR][WC]
    T* cb = in + 4 * WR * WC;              // [2][TIY][WC]: y synthesis of the x-low / x-high pairs
    const int tid = threadIdx.x, z = blockIdx.z;
    const int g0x = blockIdx.x * TIX, g0y = blockIdx.y * TIY;  // even
    const size_t zoff = (size_t)z * job.hy * job.hx;
    tile_stage_children_per<T, WR, WC, kTileThreads>(in, [&](int qd) { return job.q[qd] + zoff; }, job.hy, job.hx, g0y / 2 - c, g0x / 2 - c, tid);
    tile_cols_synthesis<T, HL, SH, WR, WC, TIY, kTileThreads>(in, cb, taps, tid);
    tile_rows_synthesis_write<T, HL, SH, WC, TIY, TIX, kTileThreads>(cb, taps, job.dst + (size_t)z * job.ny * job.nx, job.ny, job.nx, g0y, g0x, tid);
}

// ---- z pass: k_z_analysis / k_z_synthesis of z_stages.hpp, periodised, on the quadrants of one volume (ZJob) -----------------------
template <typename T, int HL>
static int launch_xy(bool fwd, const XYJob<T>& xy, int nz, const Taps2<T>& taps)
{
    const size_t lds = fwd ? tile_fwd_lds<T, HL>(false) : tile_inv_lds<T, HL>(true);
    const dim3 grid = fwd ? dim3(idiv_up(xy.hx, TFX), idiv_up(xy.hy, TFY), nz) : dim3(idiv_up(xy.nx, TIX), idiv_up(xy.ny, TIY), nz);
    return launch_lds(fwd ? k_fwd_xy<T, HL> : k_inv_xy<T, HL>, grid, dim3(kTileThreads), lds, xy, taps);
}

// pass 0: x-y; pass 1: z over the four quadrants
template <typename T>
static int run_pass(int hlen, int dir, int pass, const XYJob<T>& xy, const ZJob<T>& zj, int nz, const Taps2<T>& taps)
{
    if (pass == 1) return run_z<true, T>(hlen, dir == 0, zj, 4, taps);
    return with_filter_length(hlen, [&](auto hl) { return launch_xy<T, decltype(hl)::value>(dir == 0, xy, nz, taps); });
}

// ---- geometry ------------------------------------------------------------------------------------
struct Geom3 {
    int L;
    int z[kVolMaxLevels + 1], y[kVolMaxLevels + 1], x[kVolMaxLevels + 1];  // level-l volume, l = 0 .. L
};
static bool geom3(const pdwt_info3d& w, Geom3* g)
{
    if (!vol_sizes_ok(w)) return false;
    g->L = w.nlevels;
    g->z[0] = w.Nz;
    g->y[0] = w.Nr;
    g->x[0] = w.Nc;
    for (int l = 1; l <= w.nlevels; l++) {
        g->z[l] = div2(g->z[l - 1]);
        g->y[l] = div2(g->y[l - 1]);
        g->x[l] = div2(g->x[l - 1]);
    }
    return true;
}

// d_tmp = [Q: the 4 quadrants (z, hy, hx) | A: hz*hy*hx] at level-1 geometry (the largest of every level)
struct Tmp3 {
    size_t q, abuf, total;
};
static Tmp3 tmp3(const Geom3& g)
{
    Tmp3 t;
    const size_t z = g.z[0], hz = g.z[1], hy = g.y[1], hx = g.x[1];
    t.q = 0;
    t.abuf = pad64(4 * z * hy * hx);
    t.total = t.abuf + pad64(hz * hy * hx);
    return t;
}

template <typename T>
static int forward3d(T* img, T** c, T* tmp, pdwt_info3d w, const typename FiltersOf<T>::type* f)
{
    Geom3 g;
    if (!img || !c || !tmp || !f || !geom3(w, &g) || f->hlen != w.hlen || w.hlen < 2 || (w.hlen & 1)) return PDWT_EINVAL;
    const Taps2<T> taps = taps_fwd<T>(f);
    const Tmp3 tl = tmp3(g);
    T* const qb = tmp + tl.q;
    T* const abuf = tmp + tl.abuf;
    for (int l = 0; l < g.L; l++) {
        const int lev = l + 1;
        const size_t sq = (size_t)g.z[l] * g.y[l + 1] * g.x[l + 1];
        XYJob<T> xy{};
        xy.src = (l == 0) ? img : abuf;
        for (int q = 0; q < 4; q++) xy.q[q] = qb + q * sq;
        xy.nx = g.x[l], xy.ny = g.y[l], xy.hx = g.x[l + 1], xy.hy = g.y[l + 1];
        ZJob<T> zj{};
        for (int q = 0; q < 4; q++) {
            zj.src[q] = qb + q * sq;
            zj.lo[q] = (q == 0) ? ((lev == g.L) ? c[0] : abuf) : c[band3(g.L, lev, kZLow[q])];
            zj.hi[q] = c[band3(g.L, lev, kZHigh[q])];
        }
        zj.nin = g.z[l], zj.nout = g.z[l + 1], zj.plane = g.y[l + 1] * g.x[l + 1];
        // x-y into the quadrants (reads the level's input), then z into the bands (may overwrite abuf: already read)
        if (const int rc = run_pass<T>(w.hlen, 0, 0, xy, zj, g.z[l], taps); rc != PDWT_OK) return rc;
        if (const int rc = run_pass<T>(w.hlen, 0, 1, xy, zj, g.z[l], taps); rc != PDWT_OK) return rc;
    }
    return PDWT_OK;
}

template <typename T>
static int inverse3d(T* img, T** c, T* tmp, pdwt_info3d w, const typename FiltersOf<T>::type* f)
{
    Geom3 g;
    if (!img || !c || !tmp || !f || !geom3(w, &g) || f->hlen != w.hlen || w.hlen < 2 || (w.hlen & 1)) return PDWT_EINVAL;
    const Taps2<T> taps = taps_inv<T>(f);
    const Tmp3 tl = tmp3(g);
    T* const qb = tmp + tl.q;
    T* const abuf = tmp + tl.abuf;
    for (int l = g.L - 1; l >= 0; l--) {
        const int lev = l + 1;
        const size_t sq = (size_t)g.z[l] * g.y[l + 1] * g.x[l + 1];
        ZJob<T> zj{};
        for (int q = 0; q < 4; q++) {
            zj.src[q] = (q == 0) ? ((lev == g.L) ? c[0] : abuf) : c[band3(g.L, lev, kZLow[q])];
            zj.src2[q] = c[band3(g.L, lev, kZHigh[q])];
            zj.lo[q] = qb + q * sq;
        }
        zj.nin = g.z[l + 1], zj.nout = g.z[l], zj.plane = g.y[l + 1] * g.x[l + 1];
        XYJob<T> xy{};
        for (int q = 0; q < 4; q++) xy.q[q] = qb + q * sq;
        xy.dst = (l == 0) ? img : abuf;
        xy.nx = g.x[l], xy.ny = g.y[l], xy.hx = g.x[l + 1], xy.hy = g.y[l + 1];
        // z into the quadrants (reads abuf), then x-y into the level's output (may overwrite abuf: already read)
        if (const int rc = run_pass<T>(w.hlen, 1, 1, xy, zj, g.z[l], taps); rc != PDWT_OK) return rc;
        if (const int rc = run_pass<T>(w.hlen, 1, 0, xy, zj, g.z[l], taps); rc != PDWT_OK) return rc;
    }
    return PDWT_OK;
}

// ---- band table ----------------------------------------------------------------------------------
static long long band_size3(const pdwt_info3d& w, int num, int* bz, int* by, int* bx)
{
    Geom3 g;
    if (!geom3(w, &g) || num < 0 || num > 7 * g.L) return PDWT_EINVAL;
    const int lev = (num == 0) ? g.L : g.L - (num - 1) / 7;
    if (bz) *bz = g.z[lev];
    if (by) *by = g.y[lev];
    if (bx) *bx = g.x[lev];
    return (long long)g.z[lev] * g.y[lev] * g.x[lev];
}

// the band walks of vol3d.hpp over this geometry
template <typename T>
static T** create3(pdwt_info3d w)
{
    Geom3 g;
    if (!geom3(w, &g)) return nullptr;
    return vol_create_bands<T>(g.L, [&](int k) { return band_size3(w, k, nullptr, nullptr, nullptr); });
}
template <typename T>
static int thresh3(int op, T** c, T beta, pdwt_info3d w, int do_thresh_appcoeffs, int normalize)
{
    Geom3 g;
    if (!c || !geom3(w, &g)) return PDWT_EINVAL;
    return vol_thresh<T>(op, c, beta, g.L, do_thresh_appcoeffs, normalize, [&](int k) { return band_size3(w, k, nullptr, nullptr, nullptr); });
}
template <typename T>
static int norm1_3(T** c, pdwt_info3d w, double* out)
{
    Geom3 g;
    if (!c || !out || !geom3(w, &g)) return PDWT_EINVAL;
    return vol_norm1<T>(c, g.L, out, [&](int k) { return band_size3(w, k, nullptr, nullptr, nullptr); });
}

}  // namespace pdwt

using namespace pdwt;

extern "C" {
int pdwt_num_bands3d(pdwt_info3d w)
{
    Geom3 g;
    return geom3(w, &g) ? 7 * g.L + 1 : PDWT_EINVAL;
}
long long pdwt_band_size3d(pdwt_info3d w, int num, int* bz, int* by, int* bx) { return band_size3(w, num, bz, by, bx); }
size_t pdwt_tmp_elems3d(pdwt_info3d w)
{
    Geom3 g;
    return geom3(w, &g) ? tmp3(g).total : 0;
}
float** pdwt_create_coeffs_buffer3d_f32(pdwt_info3d w) { return create3<float>(w); }
double** pdwt_create_coeffs_buffer3d_f64(pdwt_info3d w) { return create3<double>(w); }
int pdwt_free_coeffs_buffer3d_f32(float** c, pdwt_info3d) { return vol_free_bands(c); }
int pdwt_free_coeffs_buffer3d_f64(double** c, pdwt_info3d) { return vol_free_bands(c); }
int pdwt_forward3d_separable_f32(float* img, float** c, float* tmp, pdwt_info3d w, const pdwt_filters_f32* f) { return forward3d<float>(img, c, tmp, w, f); }
int pdwt_forward3d_separable_f64(double* img, double** c, double* tmp, pdwt_info3d w, const pdwt_filters_f64* f) { return forward3d<double>(img, c, tmp, w, f); }
int pdwt_inverse3d_separable_f32(float* img, float** c, float* tmp, pdwt_info3d w, const pdwt_filters_f32* f) { return inverse3d<float>(img, c, tmp, w, f); }
int pdwt_inverse3d_separable_f64(double* img, double** c, double* tmp, pdwt_info3d w, const pdwt_filters_f64* f) { return inverse3d<double>(img, c, tmp, w, f); }
int pdwt_soft_thresh3d_f32(float** c, float beta, pdwt_info3d w, int app, int norm) { return thresh3<float>(BL_SOFT, c, beta, w, app, norm); }
int pdwt_soft_thresh3d_f64(double** c, double beta, pdwt_info3d w, int app, int norm) { return thresh3<double>(BL_SOFT, c, beta, w, app, norm); }
int pdwt_hard_thresh3d_f32(float** c, float beta, pdwt_info3d w, int app, int norm) { return thresh3<float>(BL_HARD, c, beta, w, app, norm); }
int pdwt_hard_thresh3d_f64(double** c, double beta, pdwt_info3d w, int app, int norm) { return thresh3<double>(BL_HARD, c, beta, w, app, norm); }
int pdwt_norm1_3d_f32(float** c, pdwt_info3d w, double* out) { return norm1_3<float>(c, w, out); }
int pdwt_norm1_3d_f64(double** c, pdwt_info3d w, double* out) { return norm1_3<double>(c, w, out); }
}
