// swt3d.hip -- the separable, stationary (undecimated, a-trous) 3-D transform (include/pdwt_hip.h "3-D stationary transform").
//
// One level j = the 1-D a-trous level of oracle/pdwt_oracle_impl.h (swt_ana_lines / swt_syn_lines, SURVEY A-3 / A-4) at tap
// spacing f = 2^(j-1) along x, then y, then z, in TWO launches per level and direction (the structure of dwt3d.hip):
//   forward   x-y: volume -> 4 full-size quadrants in d_tmp       one plane tile per workgroup, rows and columns in LDS
//             z:   4 quadrants -> the 8 bands of the level         lanes across a plane, a register window along z
//   inverse   z first (bands -> quadrants), then x-y (quadrants -> volume).
// Dilation: every tile works on the POLYPHASE SUBLATTICE r + f*m of each axis.  Output r + f*m reads the inputs r + f*(m - c + j),
// j = 0 .. hlen-1, which are the contiguous samples m - c .. m - c + hlen - 1 of the same sublattice, so a tile of T outputs
// stages T + hlen - 1 samples per axis at every level (a contiguous tile would need T + (hlen-1)*f).  Workgroups of the f
// residues of one tile are adjacent in the grid, so the strided loads and stores of one residue share cache lines with the others.
// Per output the tap order and the one FMA per tap are the oracle's analysis; the synthesis uses pre-halved taps in one FMA
// (the 2-D SWT kernels' deviation).
// Traffic per level: forward 1 read + 4 writes (x-y) + 4 reads + 8 writes (z) = 17 volumes against 9 compulsory; inverse mirrored.
#include "vol3d.hpp"

namespace pdwt {

constexpr int kSXYThreads = 256;
constexpr int STX = 32, STY = 16;  // x-y tile: STY x STX outputs on the (y, x) sublattices

template <typename T>
struct SXYJob {
    const T* src;  // forward: the level's input volume (z, ny, nx)
    T* dst;        // inverse: the level's output volume
    T* q[4];       // quadrants (z, ny, nx): index 2 * x band + y band (0 = low-pass)
    int nx, ny, f;
    int tiles_x;   // tiles along x: f residues x ceil(ceil(nx / f) / STX)
};

template <typename T, int HL>
constexpr size_t swt_fwd_xy_lds()
{
    return sizeof(T) * ((size_t)(STY + HL - 1) * (STX + HL - 1) + 2 * (size_t)(STY + HL - 1) * STX);
}
template <typename T, int HL>
constexpr size_t swt_inv_xy_lds()
{
    return sizeof(T) * (2 * (size_t)(STY + HL - 1) * (STX + HL - 1) + 2 * (size_t)STY * (STX + HL - 1));
}

// sa += sum_j pa[j * stride] * ta[HL-1-j], sd += sum_j pd[j * stride] * tb[HL-1-j] (one FMA per tap, j ascending).  The taps are
// re-read per chunk of 8 behind a fresh opaque zero: hoisted all at once, the 2*40 taps of the inverse overflowed the SGPRs.
template <typename T, int HL>
__device__ __forceinline__ void fma_taps2(const T* pa, const T* pd, int stride, const Taps2<T>& taps, T& sa, T& sd)
{
#pragma unroll
    for (int j0 = 0; j0 < HL; j0 += 8) {
        const int z0 = opaque_zero();
#pragma unroll
        for (int j = j0; j < (j0 + 8 < HL ? j0 + 8 : HL); j++) {
            sa = fma_t<T>(pa[j * stride], taps.a[HL - 1 - j + z0], sa);
            sd = fma_t<T>(pd[j * stride], taps.b[HL - 1 - j + z0], sd);
        }
    }
}

// tile b of an axis with f residues: residue b % f (fastest, so the residues of one tile run side by side), first sublattice index
__device__ __forceinline__ void sublattice(int b, int f, int tile, int* r, int* m0)
{
    *r = b % f;
    *m0 = (b / f) * tile;
}

// ---- forward x-y: rows then columns of one STY x STX sublattice tile of plane blockIdx.z --------------------
template <typename T, int HL>
__global__ __launch_bounds__(kSXYThreads) void k_swt_fwd_xy(SXYJob<T> job, Taps2<T> taps)
{
    extern __shared__ double smem_d[];
    constexpr int C = HL / 2 - 1, RI = STY + HL - 1, CI = STX + HL - 1;
    T* in = reinterpret_cast<T*>(smem_d);  // [RI][CI]
    T* rb = in + RI * CI;                  // [2][RI][STX]: row pass lo | hi
    const int tid = threadIdx.x, f = job.f, nx = job.nx, ny = job.ny;
    int rx, mx0, ry, my0;
    sublattice(blockIdx.x % job.tiles_x, f, STX, &rx, &mx0);
    sublattice(blockIdx.x / job.tiles_x, f, STY, &ry, &my0);
    const size_t zoff = (size_t)blockIdx.z * ny * nx;  // 64-bit plane offset
    const T* __restrict__ plane = job.src + zoff;
    for (int e = tid; e < RI * CI; e += kSXYThreads) {
        const int r = e / CI, cc = e - r * CI;
        in[e] = plane[(size_t)wrap_per(ry + f * (my0 - C + r), ny) * nx + wrap_per(rx + f * (mx0 - C + cc), nx)];
    }
    __syncthreads();
    for (int e = tid; e < RI * STX; e += kSXYThreads) {
        const int r = e / STX, ox = e % STX;
        const T* p = in + r * CI + ox;
        const int z0 = opaque_zero();
        T sl = T(0), sh = T(0);
#pragma unroll
        for (int j = 0; j < HL; j++) {
            const T v = p[j];
            sl = fma_t<T>(v, taps.a[HL - 1 - j + z0], sl);
            sh = fma_t<T>(v, taps.b[HL - 1 - j + z0], sh);
        }
        rb[e] = sl;
        rb[RI * STX + e] = sh;
    }
    __syncthreads();
    for (int e = tid; e < STY * STX; e += kSXYThreads) {
        const int oy = e / STX, ox = e % STX;
        const int gy = ry + f * (my0 + oy), gx = rx + f * (mx0 + ox);
        if (gy >= ny || gx >= nx) continue;
        const size_t o = zoff + (size_t)gy * nx + gx;
#pragma unroll
        for (int xb = 0; xb < 2; xb++) {
            const T* p = rb + xb * RI * STX + oy * STX + ox;
            const int z0 = opaque_zero();
            T sl = T(0), sh = T(0);
#pragma unroll
            for (int j = 0; j < HL; j++) {
                const T v = p[j * STX];
                sl = fma_t<T>(v, taps.a[HL - 1 - j + z0], sl);
                sh = fma_t<T>(v, taps.b[HL - 1 - j + z0], sh);
            }
            job.q[2 * xb][o] = sl;
            job.q[2 * xb + 1][o] = sh;
        }
    }
}

// ---- inverse x-y: y synthesis of each x band (its two quadrants staged in turn), then x synthesis into the plane ----------
template <typename T, int HL>
__global__ __launch_bounds__(kSXYThreads) void k_swt_inv_xy(SXYJob<T> job, Taps2<T> taps)
{
    extern __shared__ double smem_d[];
    constexpr int C = HL / 2, RI = STY + HL - 1, CI = STX + HL - 1;
    T* in = reinterpret_cast<T*>(smem_d);  // [2][RI][CI]: y low | y high of one x band
    T* cb = in + 2 * RI * CI;              // [2][STY][CI]: y synthesis of the x-low / x-high band
    const int tid = threadIdx.x, f = job.f, nx = job.nx, ny = job.ny;
    int rx, mx0, ry, my0;
    sublattice(blockIdx.x % job.tiles_x, f, STX, &rx, &mx0);
    sublattice(blockIdx.x / job.tiles_x, f, STY, &ry, &my0);
    const size_t zoff = (size_t)blockIdx.z * ny * nx;
#pragma unroll 1
    for (int xb = 0; xb < 2; xb++) {
        for (int e = tid; e < 2 * RI * CI; e += kSXYThreads) {
            const int yb = e / (RI * CI), rem = e - yb * (RI * CI), r = rem / CI, cc = rem - r * CI;
            in[e] = job.q[2 * xb + yb][zoff + (size_t)wrap_per(ry + f * (my0 - C + r), ny) * nx + wrap_per(rx + f * (mx0 - C + cc), nx)];
        }
        __syncthreads();
        for (int e = tid; e < STY * CI; e += kSXYThreads) {
            const int oy = e / CI, cc = e - oy * CI;
            const T* pa = in + oy * CI + cc;
            T sa = T(0), sd = T(0);
            fma_taps2<T, HL>(pa, pa + RI * CI, CI, taps, sa, sd);
            cb[xb * STY * CI + e] = sa + sd;
        }
        __syncthreads();  // (the next x band restages `in`)
    }
    T* __restrict__ plane = job.dst + zoff;
    for (int e = tid; e < STY * STX; e += kSXYThreads) {
        const int oy = e / STX, ox = e % STX;
        const int gy = ry + f * (my0 + oy), gx = rx + f * (mx0 + ox);
        if (gy >= ny || gx >= nx) continue;
        const T* pa = cb + oy * CI + ox;
        T sa = T(0), sd = T(0);
        fma_taps2<T, HL>(pa, pa + STY * CI, 1, taps, sa, sd);
        plane[(size_t)gy * nx + gx] = sa + sd;
    }
}

// ---- z pass: ZC outputs per thread on the z sublattice, from a register window of ZC + HL - 1 planes -----------------------
// Lanes run across a plane (coalesced), blockIdx.y = (residue, chunk of ZC sublattice outputs), blockIdx.z = quadrant.
constexpr int kSZThreads = 256;
template <typename T, int HL>
constexpr int swt_zc()
{
    return (sizeof(T) == 8 && HL > 24) ? 8 : 16;  // the inverse holds two windows: <= 2 x 47 doubles for the long banks
}

template <typename T>
struct SZJob {
    const T* src[4];   // forward: quadrants; inverse: low branches
    const T* src2[4];  // inverse: high branches
    T* lo[4];          // forward: low outputs; inverse: outputs (quadrants)
    T* hi[4];          // forward: high outputs
    int n, plane, f;
};

template <typename T, int HL>
__global__ __launch_bounds__(kSZThreads) void k_swt_ana_z(SZJob<T> job, Taps2<T> taps)
{
    const int k = blockIdx.x * kSZThreads + threadIdx.x;
    if (k >= job.plane) return;
    constexpr int ZC = swt_zc<T, HL>(), C = HL / 2 - 1, W = ZC + HL - 1;
    const int e = blockIdx.z, f = job.f, n = job.n;
    int rz, m0;
    sublattice(blockIdx.y, f, ZC, &rz, &m0);
    const size_t pl = (size_t)job.plane;
    const T* __restrict__ x = job.src[e] + k;
    T v[W];
#pragma unroll
    for (int w = 0; w < W; w++) v[w] = x[(size_t)wrap_per(rz + f * (m0 - C + w), n) * pl];
    T* __restrict__ lo = job.lo[e] + k;
    T* __restrict__ hi = job.hi[e] + k;
#pragma unroll
    for (int u = 0; u < ZC; u++) {
        const int g = rz + f * (m0 + u);
        if (g < n) {
            T sl = T(0), sh = T(0);
#pragma unroll
            for (int j = 0; j < HL; j++) {
                sl = fma_t<T>(v[u + j], taps.a[HL - 1 - j], sl);
                sh = fma_t<T>(v[u + j], taps.b[HL - 1 - j], sh);
            }
            lo[(size_t)g * pl] = sl;
            hi[(size_t)g * pl] = sh;
        }
    }
}

template <typename T, int HL>
__global__ __launch_bounds__(kSZThreads) void k_swt_syn_z(SZJob<T> job, Taps2<T> taps)
{
    const int k = blockIdx.x * kSZThreads + threadIdx.x;
    if (k >= job.plane) return;
    constexpr int ZC = swt_zc<T, HL>(), C = HL / 2, W = ZC + HL - 1;
    const int e = blockIdx.z, f = job.f, n = job.n;
    int rz, m0;
    sublattice(blockIdx.y, f, ZC, &rz, &m0);
    const size_t pl = (size_t)job.plane;
    const T* __restrict__ a = job.src[e] + k;
    const T* __restrict__ d = job.src2[e] + k;
    T va[W], vd[W];
#pragma unroll
    for (int w = 0; w < W; w++) {
        const size_t s = (size_t)wrap_per(rz + f * (m0 - C + w), n) * pl;
        va[w] = a[s];
        vd[w] = d[s];
    }
    T* __restrict__ out = job.lo[e] + k;
#pragma unroll
    for (int u = 0; u < ZC; u++) {
        const int g = rz + f * (m0 + u);
        if (g < n) {
            T sa = T(0), sd = T(0);
#pragma unroll
            for (int j = 0; j < HL; j++) {
                sa = fma_t<T>(va[u + j], taps.a[HL - 1 - j], sa);
                sd = fma_t<T>(vd[u + j], taps.b[HL - 1 - j], sd);
            }
            out[(size_t)g * pl] = sa + sd;
        }
    }
}

// ---- launches --------------------------------------------------------------------------------------------
static int tiles_of(int n, int f, int tile) { return f * idiv_up(idiv_up(n, f), tile); }

template <typename T, int HL>
static int swt_launch(int dir, int pass, const SXYJob<T>& xy, const SZJob<T>& zj, int nz, const Taps2<T>& taps)
{
    if (pass == 0) {  // x-y
        const bool fwd = dir == 0;
        const size_t lds = fwd ? swt_fwd_xy_lds<T, HL>() : swt_inv_xy_lds<T, HL>();
        const dim3 grid((unsigned)xy.tiles_x * (unsigned)tiles_of(xy.ny, xy.f, STY), 1, nz);
        return launch_lds(fwd ? k_swt_fwd_xy<T, HL> : k_swt_inv_xy<T, HL>, grid, dim3(kSXYThreads), lds, xy, taps);
    }
    const dim3 grid(idiv_up(zj.plane, kSZThreads), tiles_of(zj.n, zj.f, swt_zc<T, HL>()), 4);  // z
    return launch_lds(dir == 0 ? k_swt_ana_z<T, HL> : k_swt_syn_z<T, HL>, grid, dim3(kSZThreads), 0, zj, taps);
}

template <typename T>
static int swt_run_pass(int hlen, int dir, int pass, const SXYJob<T>& xy, const SZJob<T>& zj, int nz, const Taps2<T>& taps)
{
    return with_filter_length(hlen, [&](auto hl) { return swt_launch<T, decltype(hl)::value>(dir, pass, xy, zj, nz, taps); });
}

// ---- geometry ------------------------------------------------------------------------------------
// Nz <= 65535 (a grid dimension), Nr * Nc < 2^31 (a plane is indexed in 32 bits), an even hlen of the table, and the level clamp
// (hlen - 1) * 2^(L-1) < min(Nz, Nr, Nc): one periodic wrap reaches every tap, and every sublattice index r + f*(m - c + j) of
// the kernels stays far inside 32 bits (min(N)^2 <= Nr * Nc < 2^31).
static bool swt_geom(const pdwt_info3d& w)
{
    if (!vol_sizes_ok(w)) return false;
    if (w.hlen < 2 || w.hlen > PDWT_MAX_FILTER_WIDTH || (w.hlen & 1)) return false;
    int n = w.Nz < w.Nr ? w.Nz : w.Nr;
    if (w.Nc < n) n = w.Nc;
    return (long long)(w.hlen - 1) << (w.nlevels - 1) < n;
}
static size_t swt_vol(const pdwt_info3d& w) { return (size_t)w.Nz * w.Nr * w.Nc; }
// d_tmp = the 4 full-size x-y quadrants of a level
static size_t swt_tmp_elems(const pdwt_info3d& w) { return 4 * pad64(swt_vol(w)); }

template <typename T>
static int swt_forward3d(T* img, T** c, T* tmp, pdwt_info3d w, const typename FiltersOf<T>::type* f)
{
    if (!img || !c || !tmp || !f || !swt_geom(w) || f->hlen != w.hlen) return PDWT_EINVAL;
    const Taps2<T> taps = taps_fwd<T>(f);
    const size_t sq = pad64(swt_vol(w));
    for (int lev = 1; lev <= w.nlevels; lev++) {
        SXYJob<T> xy{};
        xy.src = (lev == 1) ? img : c[0];  // the approximation of the level above passes through band 0
        for (int q = 0; q < 4; q++) xy.q[q] = tmp + q * sq;
        xy.nx = w.Nc, xy.ny = w.Nr, xy.f = 1 << (lev - 1);
        xy.tiles_x = tiles_of(w.Nc, xy.f, STX);
        SZJob<T> zj{};
        for (int q = 0; q < 4; q++) {
            zj.src[q] = tmp + q * sq;
            zj.lo[q] = (q == 0) ? c[0] : c[band3(w.nlevels, lev, kZLow[q])];
            zj.hi[q] = c[band3(w.nlevels, lev, kZHigh[q])];
        }
        zj.n = w.Nz, zj.plane = w.Nr * w.Nc, zj.f = xy.f;
        // x-y into the quadrants (reads band 0), then z into the bands (overwrites band 0: already read)
        if (const int rc = swt_run_pass<T>(w.hlen, 0, 0, xy, zj, w.Nz, taps); rc != PDWT_OK) return rc;
        if (const int rc = swt_run_pass<T>(w.hlen, 0, 1, xy, zj, w.Nz, taps); rc != PDWT_OK) return rc;
    }
    return PDWT_OK;
}

// The intermediate approximations A_{L-1} .. A_1 pass through img (the output anyway), so every band stays intact.
template <typename T>
static int swt_inverse3d(T* img, T** c, T* tmp, pdwt_info3d w, const typename FiltersOf<T>::type* f)
{
    if (!img || !c || !tmp || !f || !swt_geom(w) || f->hlen != w.hlen) return PDWT_EINVAL;
    const Taps2<T> taps = taps_inv<T>(f, T(0.5));  // pre-halved: one FMA per tap
    const size_t sq = pad64(swt_vol(w));
    for (int lev = w.nlevels; lev >= 1; lev--) {
        SZJob<T> zj{};
        for (int q = 0; q < 4; q++) {
            zj.src[q] = (q == 0) ? ((lev == w.nlevels) ? c[0] : img) : c[band3(w.nlevels, lev, kZLow[q])];
            zj.src2[q] = c[band3(w.nlevels, lev, kZHigh[q])];
            zj.lo[q] = tmp + q * sq;
        }
        zj.n = w.Nz, zj.plane = w.Nr * w.Nc, zj.f = 1 << (lev - 1);
        SXYJob<T> xy{};
        for (int q = 0; q < 4; q++) xy.q[q] = tmp + q * sq;
        xy.dst = img;
        xy.nx = w.Nc, xy.ny = w.Nr, xy.f = zj.f;
        xy.tiles_x = tiles_of(w.Nc, xy.f, STX);
        // z into the quadrants (reads img), then x-y into img (already read)
        if (const int rc = swt_run_pass<T>(w.hlen, 1, 1, xy, zj, w.Nz, taps); rc != PDWT_OK) return rc;
        if (const int rc = swt_run_pass<T>(w.hlen, 1, 0, xy, zj, w.Nz, taps); rc != PDWT_OK) return rc;
    }
    return PDWT_OK;
}

// ---- band table: 7L+1 full-size bands, through the band walks of vol3d.hpp ------------------------------------------
template <typename T>
static T** swt_create(pdwt_info3d w)
{
    if (!swt_geom(w)) return nullptr;
    return vol_create_bands<T>(w.nlevels, [&](int) { return swt_vol(w); });
}
template <typename T>
static int swt_thresh(int op, T** c, T beta, pdwt_info3d w, int do_thresh_appcoeffs, int normalize)
{
    if (!c || !swt_geom(w)) return PDWT_EINVAL;
    return vol_thresh<T>(op, c, beta, w.nlevels, do_thresh_appcoeffs, normalize, [&](int) { return swt_vol(w); });
}
template <typename T>
static int swt_norm1(T** c, pdwt_info3d w, double* out)
{
    if (!c || !out || !swt_geom(w)) return PDWT_EINVAL;
    return vol_norm1<T>(c, w.nlevels, out, [&](int) { return swt_vol(w); });
}

}  // namespace pdwt

using namespace pdwt;

extern "C" {
int pdwt_num_bands_swt3d(pdwt_info3d w) { return swt_geom(w) ? 7 * w.nlevels + 1 : PDWT_EINVAL; }
long long pdwt_band_size_swt3d(pdwt_info3d w, int num, int* bz, int* by, int* bx)
{
    if (!swt_geom(w) || num < 0 || num > 7 * w.nlevels) return PDWT_EINVAL;
    if (bz) *bz = w.Nz;
    if (by) *by = w.Nr;
    if (bx) *bx = w.Nc;
    return (long long)swt_vol(w);
}
size_t pdwt_tmp_elems_swt3d(pdwt_info3d w) { return swt_geom(w) ? swt_tmp_elems(w) : 0; }
float** pdwt_create_coeffs_buffer_swt3d_f32(pdwt_info3d w) { return swt_create<float>(w); }
double** pdwt_create_coeffs_buffer_swt3d_f64(pdwt_info3d w) { return swt_create<double>(w); }
int pdwt_free_coeffs_buffer_swt3d_f32(float** c, pdwt_info3d) { return vol_free_bands(c); }
int pdwt_free_coeffs_buffer_swt3d_f64(double** c, pdwt_info3d) { return vol_free_bands(c); }
int pdwt_forward3d_swt_f32(float* img, float** c, float* tmp, pdwt_info3d w, const pdwt_filters_f32* f) { return swt_forward3d<float>(img, c, tmp, w, f); }
int pdwt_forward3d_swt_f64(double* img, double** c, double* tmp, pdwt_info3d w, const pdwt_filters_f64* f) { return swt_forward3d<double>(img, c, tmp, w, f); }
int pdwt_inverse3d_swt_f32(float* img, float** c, float* tmp, pdwt_info3d w, const pdwt_filters_f32* f) { return swt_inverse3d<float>(img, c, tmp, w, f); }
int pdwt_inverse3d_swt_f64(double* img, double** c, double* tmp, pdwt_info3d w, const pdwt_filters_f64* f) { return swt_inverse3d<double>(img, c, tmp, w, f); }
int pdwt_soft_thresh_swt3d_f32(float** c, float beta, pdwt_info3d w, int app, int norm) { return swt_thresh<float>(BL_SOFT, c, beta, w, app, norm); }
int pdwt_soft_thresh_swt3d_f64(double** c, double beta, pdwt_info3d w, int app, int norm) { return swt_thresh<double>(BL_SOFT, c, beta, w, app, norm); }
int pdwt_hard_thresh_swt3d_f32(float** c, float beta, pdwt_info3d w, int app, int norm) { return swt_thresh<float>(BL_HARD, c, beta, w, app, norm); }
int pdwt_hard_thresh_swt3d_f64(double** c, double beta, pdwt_info3d w, int app, int norm) { return swt_thresh<double>(BL_HARD, c, beta, w, app, norm); }
int pdwt_norm1_swt3d_f32(float** c, pdwt_info3d w, double* out) { return swt_norm1<float>(c, w, out); }
int pdwt_norm1_swt3d_f64(double** c, pdwt_info3d w, double* out) { return swt_norm1<double>(c, w, out); }
}
