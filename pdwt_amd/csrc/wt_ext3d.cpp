// wt_ext3d.cpp -- host side of `BoundaryWavelets3D` (include/wt_ext.h) above the level entry points of include/pdwt_hip.h ("3-D DWT
// with boundary modes"), and its flat C handle API (pdwt_bw3_*, name for name with pdwt_bw1_* of wt_ext.cpp).  Plain host C++, built
// into libpdwt.so (float) and libpdwtd.so (-DDOUBLEPRECISION).  The geometry, the band table and the walk over the levels live here;
// the device only ever sees one level.  Thresholds, norms and statistics go through the band-list entries (bandstats_host.hpp).
#include <limits.h>
#include <new>
#include <stddef.h>
#include <string.h>

#include "../../include/pdwt_hip.h"
#include "../../include/wt_ext.h"
#include "bandstats_host.hpp"

static_assert(7 * BW3_MAX_LEVELS + 1 <= pdwt_bl::kMaxBands, "the level clamp stays within the band limit of the band-list kernels");

#ifndef DOUBLEPRECISION
#define SFX(name) name##_f32
typedef pdwt_filters_f32 bw3_filters_t;
#else
#define SFX(name) name##_f64
typedef pdwt_filters_f64 bw3_filters_t;
#endif

namespace {
constexpr int kL3 = BW3_MAX_LEVELS;

struct bw3_priv {
    bw3_filters_t f;
    int dev;                                    // the device current at construction; every method runs there
    int nz[kL3 + 1], nr[kL3 + 1], nc[kL3 + 1];  // [0] the volume, [l] the bands of level l
    DTYPE* d_bands;                             // the one allocation behind d_coeffs
    DTYPE* d_tmp;                               // [the four x-y quadrants | the approximation of the levels 1 .. L-1], level-1 size
    DTYPE* d_approx;                            // the second part of d_tmp
};
inline bw3_priv* P3(void* p) { return (bw3_priv*)p; }

struct DevScopeB3 {
    int prev, mine;
    explicit DevScopeB3(const void* st) : prev(-1), mine(st ? ((const bw3_priv*)st)->dev : -1)
    {
        if (mine < 0) return;
        prev = pdwt_get_device();
        if (prev != mine) pdwt_set_device(mine);
    }
    ~DevScopeB3()
    {
        if (mine >= 0 && prev >= 0 && prev != mine) pdwt_set_device(prev);
    }
};
void report3(const char* where, int rc) { printf("ERROR: BoundaryWavelets3D%s failed (code %d): %s\n", where, rc, pdwt_last_error_string()); }

// level (1 = finest) of band num of [A_L, level L ... level 1]
inline int band_level3(int L, int num) { return num == 0 ? L : L - (num - 1) / 7; }
// the size limits alone (Nz <= 65535, Nr * Nc < 2^31), as the level entries state them: a Haar level has no minimum length
inline bool sizes_ok(int Nz, int Nr, int Nc) { return pdwt_num_bands_ext3d(Nz, Nr, Nc, 2, 1) > 0; }
}  // namespace
#define ON_MY_DEVICE_B3() DevScopeB3 dev_scope_(priv_)

int BoundaryWavelets3D::geometry(int Nz, int Nr, int Nc, int hlen, int levels, int* nz, int* nr, int* nc)
{
    if (!sizes_ok(Nz, Nr, Nc) || hlen < 2 || hlen > PDWT_MAX_FILTER_WIDTH || (hlen & 1)) return 0;
    if (levels < 1) levels = 1;
    int N = Nz < Nr ? Nz : Nr;
    if (Nc < N) N = Nc;
    int wmaxlev = w_ilog2(N / (hlen - 1));  // the rule of Wavelets3D = PyWavelets' dwt_max_level over the three axes
    if (wmaxlev > kL3) wmaxlev = kL3;
    if (levels > wmaxlev) levels = wmaxlev;
    for (int l = 0; l <= levels; l++) {
        if (nz) nz[l] = Nz;
        if (nr) nr[l] = Nr;
        if (nc) nc[l] = Nc;
        Nz = (Nz + hlen - 1) >> 1, Nr = (Nr + hlen - 1) >> 1, Nc = (Nc + hlen - 1) >> 1;
    }
    return levels;
}

BoundaryWavelets3D::BoundaryWavelets3D(DTYPE* vol, int Nz, int Nr, int Nc, const char* wname_, int levels, int mode, int memisonhost)
    : d_image(NULL), d_coeffs(NULL), state(W_INIT), priv_(NULL)
{
    winfos.Nz = Nz, winfos.Nr = Nr, winfos.Nc = Nc, winfos.nlevels = levels, winfos.hlen = 0, winfos.mode = mode;
    strncpy(wname, wname_ ? wname_ : "", 127);
    wname[127] = 0;
    if (Nz < 1 || Nr < 1 || Nc < 1 || !wname_) {
        puts("ERROR: BoundaryWavelets3D(): invalid volume size or wavelet name");
        state = W_CREATION_ERROR;
        return;
    }
    if (!sizes_ok(Nz, Nr, Nc)) {
        puts("ERROR: BoundaryWavelets3D(): unsupported volume size (Nz <= 65535 and Nr * Nc < 2^31 are required)");
        state = W_CREATION_ERROR;
        return;
    }
    if (mode < 0 || mode >= BW_NUM_MODES) {
        printf("ERROR: BoundaryWavelets3D(): unknown boundary mode %d (0 zero, 1 constant, 2 symmetric, 3 reflect, 4 periodic)\n", mode);
        state = W_CREATION_ERROR;
        return;
    }
    if (levels < 1) {
        puts("Warning: cannot initialize wavelet coefficients with nlevels < 1. Forcing nlevels = 1");
        winfos.nlevels = 1;
    }
    bw3_priv* p = new (std::nothrow) bw3_priv();
    if (!p) {
        state = W_CREATION_ERROR;
        return;
    }
    priv_ = p;
    p->d_bands = p->d_tmp = p->d_approx = NULL;
    p->dev = pdwt_get_device();
    const int hlen = SFX(pdwt_compute_filters_separable)(wname, 0, &p->f);
    if (hlen <= 0) {
        printf("ERROR: unknown wavelet name %s\n", wname);
        state = W_CREATION_ERROR;
        return;
    }
    p->f.hlen = hlen;
    winfos.hlen = hlen;
    const int wmaxlev = geometry(Nz, Nr, Nc, hlen, winfos.nlevels, p->nz, p->nr, p->nc);
    if (winfos.nlevels > wmaxlev) {
        printf("Warning: required level (%d) is greater than the maximum possible level for %s (%d) on a %dx%dx%d volume.\n", winfos.nlevels, wname,
               wmaxlev, Nz, Nr, Nc);
        printf("Forcing nlevels = %d\n", wmaxlev);
        winfos.nlevels = wmaxlev;
    }
    if (winfos.nlevels < 1) {
        printf("ERROR: a %dx%dx%d volume is too small for one level of %s\n", Nz, Nr, Nc, wname);
        state = W_CREATION_ERROR;
        return;
    }
    const int L = winfos.nlevels, nb = 7 * L + 1;
    const long long ntmp = pdwt_ext3d_tmp_elems(Nz, Nr, Nc, hlen), approx_off = pdwt_ext3d_tmp_approx_offset(Nz, Nr, Nc, hlen);
    if (ntmp <= 0 || approx_off <= 0) {
        puts("ERROR: BoundaryWavelets3D(): unsupported volume size (Nz <= 65535 and Nr * Nc < 2^31 are required)");
        state = W_CREATION_ERROR;
        return;
    }
    size_t off[pdwt_bl::kMaxBands], total = 0;
    for (int k = 0; k < nb; k++) {
        const int l = band_level3(L, k);
        off[k] = total;
        total += ((size_t)p->nz[l] * p->nr[l] * p->nc[l] * sizeof(DTYPE) + 255) & ~(size_t)255;
    }
    const size_t n = (size_t)Nz * Nr * Nc;
    d_image = (DTYPE*)pdwt_malloc(n * sizeof(DTYPE));
    p->d_bands = (DTYPE*)pdwt_malloc(total);
    p->d_tmp = (DTYPE*)pdwt_malloc((size_t)ntmp * sizeof(DTYPE));
    d_coeffs = (DTYPE**)calloc((size_t)nb, sizeof(DTYPE*));
    int rc = (d_image && p->d_bands && p->d_tmp && d_coeffs) ? PDWT_OK : PDWT_ENOMEM;
    if (rc == PDWT_OK) {
        p->d_approx = p->d_tmp + approx_off;  // (the layout of the scratch is the library's alone)
        for (int k = 0; k < nb; k++) d_coeffs[k] = (DTYPE*)((char*)p->d_bands + off[k]);
        rc = pdwt_memset(p->d_bands, 0, total);
    }
    if (rc == PDWT_OK) {
        if (!vol) rc = pdwt_memset(d_image, 0, n * sizeof(DTYPE));
        else if (memisonhost) rc = pdwt_memcpy_h2d(d_image, vol, n * sizeof(DTYPE));
        else rc = pdwt_memcpy_d2d_foreign(d_image, vol, n * sizeof(DTYPE));
    }
    if (rc != PDWT_OK) {
        report3("(): allocation or upload", rc);
        state = W_CREATION_ERROR;
    }
}

BoundaryWavelets3D::~BoundaryWavelets3D()
{
    ON_MY_DEVICE_B3();
    if (d_image) pdwt_free(d_image);
    free(d_coeffs);
    if (priv_) {
        bw3_priv* p = P3(priv_);
        if (p->d_bands) pdwt_free(p->d_bands);
        if (p->d_tmp) pdwt_free(p->d_tmp);
        delete p;
    }
}

// the eight bands of level l (1 .. L) in the order of the level entries: aaa, then the seven details.  The approximation is band 0 for
// l == L, else the scratch buffer: level l + 1 reads it (x-y pass) before it writes its own there (z pass), and the inverse likewise.
static void level_bands(const BoundaryWavelets3D& W, bw3_priv* p, int l, DTYPE** b)
{
    const int L = W.winfos.nlevels;
    b[0] = l == L ? W.d_coeffs[0] : p->d_approx;
    for (int k = 0; k < 7; k++) b[1 + k] = W.d_coeffs[1 + 7 * (L - l) + k];
}

void BoundaryWavelets3D::forward()
{
    ON_MY_DEVICE_B3();
    if (state == W_CREATION_ERROR) {
        puts("Warning: forward transform not computed, as there was an error when creating the wavelets");
        return;
    }
    bw3_priv* p = P3(priv_);
    for (int l = 1; l <= winfos.nlevels; l++) {
        DTYPE* b[8];
        level_bands(*this, p, l, b);
        const DTYPE* src = l == 1 ? d_image : p->d_approx;
        const int rc = SFX(pdwt_ext3d_forward_level)(src, b, p->nz[l - 1], p->nr[l - 1], p->nc[l - 1], winfos.mode, &p->f, p->d_tmp);
        if (rc != PDWT_OK) {
            report3("::forward()", rc);
            state = W_FORWARD_ERROR;
            return;
        }
    }
    state = W_FORWARD;
}

void BoundaryWavelets3D::inverse()
{
    ON_MY_DEVICE_B3();
    if (state == W_INVERSE) {
        puts("Warning: W.inverse() has already been run. Inverse is available in W.get_image()");
        return;
    }
    if (state == W_CREATION_ERROR || state == W_FORWARD_ERROR || state == W_THRESHOLD_ERROR) {
        puts("Warning: inverse transform not computed, as there was an error in a previous stage");
        return;
    }
    bw3_priv* p = P3(priv_);
    for (int l = winfos.nlevels; l >= 1; l--) {
        DTYPE* b[8];
        level_bands(*this, p, l, b);
        DTYPE* dst = l == 1 ? d_image : p->d_approx;
        const int rc = SFX(pdwt_ext3d_inverse_level)(dst, b, p->nz[l - 1], p->nr[l - 1], p->nc[l - 1], &p->f, p->d_tmp);
        if (rc != PDWT_OK) {
            report3("::inverse()", rc);
            state = W_INVERSE_ERROR;
            return;
        }
    }
    state = W_INVERSE;
}

int BoundaryWavelets3D::get_image(DTYPE* res)
{
    ON_MY_DEVICE_B3();
    if (!d_image || !res || state == W_CREATION_ERROR) return 0;
    const size_t n = (size_t)winfos.Nz * winfos.Nr * winfos.Nc;
    if (pdwt_memcpy_d2h(res, d_image, n * sizeof(DTYPE)) != PDWT_OK) return 0;
    return n > (size_t)INT_MAX ? INT_MAX : (int)n;
}

void BoundaryWavelets3D::set_image(DTYPE* vol, int mem_is_on_device)
{
    ON_MY_DEVICE_B3();
    if (!d_image || !vol || state == W_CREATION_ERROR) return;
    const size_t nb = (size_t)winfos.Nz * winfos.Nr * winfos.Nc * sizeof(DTYPE);
    const int rc = mem_is_on_device ? pdwt_memcpy_d2d_foreign(d_image, vol, nb) : pdwt_memcpy_h2d(d_image, vol, nb);
    if (rc != PDWT_OK) report3("::set_image()", rc);
    state = W_INIT;
}

int BoundaryWavelets3D::num_bands() const { return state == W_CREATION_ERROR ? 0 : 7 * winfos.nlevels + 1; }

long long BoundaryWavelets3D::coeff_shape(int num, int* nz, int* nr, int* nc) const
{
    if (state == W_CREATION_ERROR || num < 0 || num >= num_bands()) return 0;
    const bw3_priv* p = P3(priv_);
    const int l = band_level3(winfos.nlevels, num);
    if (nz) *nz = p->nz[l];
    if (nr) *nr = p->nr[l];
    if (nc) *nc = p->nc[l];
    return (long long)p->nz[l] * p->nr[l] * p->nc[l];
}

int BoundaryWavelets3D::get_coeff(DTYPE* coeff, int num)
{
    ON_MY_DEVICE_B3();
    if (state == W_INVERSE) {
        puts("Warning: get_coeff(): inverse() has been performed; run forward() first.");
        return 0;
    }
    const long long n = coeff_shape(num, NULL, NULL, NULL);
    if (n <= 0 || !coeff) return 0;
    if (pdwt_memcpy_d2h(coeff, d_coeffs[num], (size_t)n * sizeof(DTYPE)) != PDWT_OK) return 0;
    return n > (long long)INT_MAX ? INT_MAX : (int)n;
}

void BoundaryWavelets3D::set_coeff(DTYPE* coeff, int num, int mem_is_on_device)
{
    ON_MY_DEVICE_B3();
    const long long n = coeff_shape(num, NULL, NULL, NULL);
    if (n <= 0 || !coeff) {
        if (state != W_CREATION_ERROR) printf("ERROR: set_coeff(): invalid coefficient index %d\n", num);
        return;
    }
    const size_t nb = (size_t)n * sizeof(DTYPE);
    const int rc = mem_is_on_device ? pdwt_memcpy_d2d_foreign(d_coeffs[num], coeff, nb) : pdwt_memcpy_h2d(d_coeffs[num], coeff, nb);
    if (rc != PDWT_OK) report3("::set_coeff()", rc);
}

intptr_t BoundaryWavelets3D::image_int_ptr() { return (intptr_t)d_image; }
intptr_t BoundaryWavelets3D::coeff_int_ptr(int num) { return coeff_shape(num, NULL, NULL, NULL) > 0 ? (intptr_t)d_coeffs[num] : 0; }

// ---- the band list (bandstats_host.hpp) ------------------------------------------------------------------------------------------
// pointer and size of every band; nb = 0 when the coefficients are not there to be read (need_forward: only those of a forward())
static pdwt_bl::BandList band_list(const BoundaryWavelets3D& W, bool need_forward)
{
    pdwt_bl::BandList bl;
    bl.nb = 0;
    if (W.state == W_CREATION_ERROR || W.state == W_INVERSE || !W.d_coeffs) return bl;
    if (need_forward && !(W.state == W_FORWARD || W.state == W_THRESHOLD)) return bl;
    const int nb = W.num_bands();
    for (int k = 0; k < nb; k++) {
        bl.ptr[k] = W.d_coeffs[k];
        bl.n[k] = (size_t)W.coeff_shape(k, NULL, NULL, NULL);
    }
    bl.nb = nb;
    bl.finest = 7 * W.winfos.nlevels;  // ddd of level 1
    bl.samples = (double)W.winfos.Nz * W.winfos.Nr * W.winfos.Nc;
    return bl;
}

void BoundaryWavelets3D::threshold(int op, DTYPE beta, int do_thresh_appcoeffs)
{
    ON_MY_DEVICE_B3();
    if (state == W_INVERSE) {
        puts("Warning: BoundaryWavelets3D(): cannot threshold coefficients after W.inverse() (run forward() first)");
        return;
    }
    const pdwt_bl::BandList bl = band_list(*this, false);
    if (!bl.nb) return;
    DTYPE betas[pdwt_bl::kMaxBands];
    for (int k = 0; k < bl.nb; k++) betas[k] = beta;
    if (!do_thresh_appcoeffs) betas[0] = (DTYPE)-1;  // (a negative beta leaves the band alone)
    const int rc = pdwt_bl::threshold(bl, betas, op);
    if (rc != PDWT_OK) {
        report3(op ? "::hard_threshold()" : "::soft_threshold()", rc);
        state = W_THRESHOLD_ERROR;
    }
}
void BoundaryWavelets3D::soft_threshold(DTYPE beta, int do_thresh_appcoeffs) { threshold(0, beta, do_thresh_appcoeffs); }
void BoundaryWavelets3D::hard_threshold(DTYPE beta, int do_thresh_appcoeffs) { threshold(1, beta, do_thresh_appcoeffs); }

double BoundaryWavelets3D::norm1()
{
    ON_MY_DEVICE_B3();
    const pdwt_bl::BandList bl = band_list(*this, false);
    if (!bl.nb) return -1.0;
    w_band_stats s[pdwt_bl::kMaxBands];
    const int rc = pdwt_bl::stats(bl, -1, s, 0);
    if (rc != PDWT_OK) {
        report3("::norm1()", rc);
        return -1.0;
    }
    double sum = 0.0;
    for (int k = 0; k < bl.nb; k++) sum += s[k].sum_abs;
    return sum;
}

int BoundaryWavelets3D::band_stats(int num, w_band_stats* out, int with_median)
{
    ON_MY_DEVICE_B3();
    const pdwt_bl::BandList bl = band_list(*this, true);
    if (!bl.nb || num < 0 || num >= bl.nb || !out) return PDWT_EINVAL;
    const int rc = pdwt_bl::stats(bl, num, out, with_median);
    if (rc != PDWT_OK) report3("::band_stats()", rc);
    return rc;
}

int BoundaryWavelets3D::all_band_stats(w_band_stats* out, int with_median)
{
    ON_MY_DEVICE_B3();
    const pdwt_bl::BandList bl = band_list(*this, true);
    if (!bl.nb || !out) return PDWT_EINVAL;
    const int rc = pdwt_bl::stats(bl, -1, out, with_median);
    if (rc != PDWT_OK) report3("::all_band_stats()", rc);
    return rc;
}

double BoundaryWavelets3D::estimate_sigma()
{
    ON_MY_DEVICE_B3();
    const pdwt_bl::BandList bl = band_list(*this, true);
    double sigma = -1.0;
    if (!bl.nb) return -1.0;
    const int rc = pdwt_bl::estimate_sigma(bl, &sigma);
    if (rc != PDWT_OK) {
        report3("::estimate_sigma()", rc);
        return -1.0;
    }
    return sigma;
}

void BoundaryWavelets3D::threshold_bands(const DTYPE* betas, int kind)
{
    ON_MY_DEVICE_B3();
    const pdwt_bl::BandList bl = band_list(*this, true);
    if (!bl.nb || !betas || (kind != 0 && kind != 1)) return;
    const int rc = pdwt_bl::threshold(bl, betas, kind);
    if (rc != PDWT_OK) {
        report3("::threshold_bands()", rc);
        state = W_THRESHOLD_ERROR;
    }
}

double BoundaryWavelets3D::denoise(int method, double sigma, int kind, DTYPE* betas_out)
{
    ON_MY_DEVICE_B3();
    const pdwt_bl::BandList bl = band_list(*this, true);
    if (!bl.nb || (method != 0 && method != 1) || (kind != 0 && kind != 1)) return -1.0;
    DTYPE betas[pdwt_bl::kMaxBands];
    const int rc = pdwt_bl::denoise(bl, method, kind, &sigma, betas);
    if (rc != PDWT_OK) {
        report3("::denoise()", rc);
        state = W_THRESHOLD_ERROR;
        return -1.0;
    }
    if (betas_out) memcpy(betas_out, betas, (size_t)bl.nb * sizeof(DTYPE));
    return sigma;
}

// ---- flat C handle API (pdwt_amd/boundary.py), name for name with pdwt_bw1_* --------------------------------------
#define BW3(h) static_cast<BoundaryWavelets3D*>(h)
extern "C" {
void* pdwt_bw3_new(DTYPE* vol, int Nz, int Nr, int Nc, const char* wname, int levels, int mode, int memisonhost)
{
    return new (std::nothrow) BoundaryWavelets3D(vol, Nz, Nr, Nc, wname, levels, mode, memisonhost);
}
void pdwt_bw3_delete(void* h) { delete BW3(h); }
void pdwt_bw3_forward(void* h) { BW3(h)->forward(); }
void pdwt_bw3_inverse(void* h) { BW3(h)->inverse(); }
int pdwt_bw3_get_image(void* h, DTYPE* out) { return BW3(h)->get_image(out); }
void pdwt_bw3_set_image(void* h, DTYPE* vol, int mem_is_on_device) { BW3(h)->set_image(vol, mem_is_on_device); }
int pdwt_bw3_state(void* h) { return (int)BW3(h)->state; }
void pdwt_bw3_info(void* h, w_info_bw3* out) { *out = BW3(h)->winfos; }
int pdwt_bw3_geometry(int Nz, int Nr, int Nc, int hlen, int levels, int* nz, int* nr, int* nc)
{
    return BoundaryWavelets3D::geometry(Nz, Nr, Nc, hlen, levels, nz, nr, nc);
}
int pdwt_bw3_mode_index(const char* name) { return BoundaryWavelets::mode_index(name); }
int pdwt_bw3_num_bands(void* h) { return BW3(h)->num_bands(); }
long long pdwt_bw3_coeff_shape(void* h, int num, int* nz, int* nr, int* nc) { return BW3(h)->coeff_shape(num, nz, nr, nc); }
int pdwt_bw3_get_coeff(void* h, DTYPE* out, int num) { return BW3(h)->get_coeff(out, num); }
void pdwt_bw3_set_coeff(void* h, DTYPE* in, int num, int mem_is_on_device) { BW3(h)->set_coeff(in, num, mem_is_on_device); }
intptr_t pdwt_bw3_image_int_ptr(void* h) { return BW3(h)->image_int_ptr(); }
intptr_t pdwt_bw3_coeff_int_ptr(void* h, int num) { return BW3(h)->coeff_int_ptr(num); }
void pdwt_bw3_soft_threshold(void* h, DTYPE beta, int app) { BW3(h)->soft_threshold(beta, app); }
void pdwt_bw3_hard_threshold(void* h, DTYPE beta, int app) { BW3(h)->hard_threshold(beta, app); }
double pdwt_bw3_norm1(void* h) { return BW3(h)->norm1(); }
int pdwt_bw3_band_stats(void* h, int num, w_band_stats* out, int with_median) { return BW3(h)->band_stats(num, out, with_median); }
int pdwt_bw3_all_band_stats(void* h, w_band_stats* out, int with_median) { return BW3(h)->all_band_stats(out, with_median); }
double pdwt_bw3_estimate_sigma(void* h) { return BW3(h)->estimate_sigma(); }
void pdwt_bw3_threshold_bands(void* h, const DTYPE* betas, int kind) { BW3(h)->threshold_bands(betas, kind); }
double pdwt_bw3_denoise(void* h, int method, double sigma, int kind, DTYPE* betas_out) { return BW3(h)->denoise(method, sigma, kind, betas_out); }
}
#undef BW3
