// wt_ext.cpp -- host side of `BoundaryWavelets` (include/wt_ext.h) above the level entry points of include/pdwt_hip.h ("2-D DWT with
// boundary modes"), and its flat C handle API (pdwt_bw_*, the shape of wpt.cpp).  Plain host C++ like wt.cpp, built into libpdwt.so
// (float) and libpdwtd.so (-DDOUBLEPRECISION).  The geometry, the band table and the walk over the levels live here; the device only
// ever sees one level.  Thresholds, norms and statistics go through the band-list entries (bandstats_host.hpp): no kernels of its own.
// Below it `BoundaryWavelets1D`, the same along the last axis of a batch of rows, above the whole-transform entries of "Batched 1-D DWT
// with boundary modes" (pdwt_bw1_*).
#include <limits.h>
#include <new>
#include <stddef.h>
#include <string.h>

#include "../../include/pdwt_hip.h"
#include "../../include/wt_ext.h"
#include "bandstats_host.hpp"

static_assert(3 * BW_MAX_LEVELS + 1 == pdwt_bl::kMaxBands, "the level clamp is the band limit of the band-list kernels");

#ifndef DOUBLEPRECISION
#define SFX(name) name##_f32
typedef pdwt_filters_f32 bw_filters_t;
#else
#define SFX(name) name##_f64
typedef pdwt_filters_f64 bw_filters_t;
#endif

namespace {
constexpr int kL = BW_MAX_LEVELS;
const char* const kModeNames[BW_NUM_MODES] = {"zero", "constant", "symmetric", "reflect", "periodic"};

struct bw_priv {
    bw_filters_t f;
    int dev;                     // the device current at construction; every method runs there
    int nr[kL + 1], nc[kL + 1];  // [0] the image, [l] the bands of level l
    DTYPE* d_bands;              // the one allocation behind d_coeffs
    DTYPE* d_ping[2];            // intermediate approximations (levels 1 .. L-1), level-1 size each; NULL for one level
};
inline bw_priv* P(void* p) { return (bw_priv*)p; }

struct DevScopeB {
    int prev, mine;
    explicit DevScopeB(const void* st) : prev(-1), mine(st ? ((const bw_priv*)st)->dev : -1)
    {
        if (mine < 0) return;
        prev = pdwt_get_device();
        if (prev != mine) pdwt_set_device(mine);
    }
    ~DevScopeB()
    {
        if (mine >= 0 && prev >= 0 && prev != mine) pdwt_set_device(prev);
    }
};
void report(const char* where, int rc) { printf("ERROR: BoundaryWavelets%s failed (code %d): %s\n", where, rc, pdwt_last_error_string()); }

// level (1 = finest) of band num of [A_L, H1, V1, D1, ..., H_L, V_L, D_L]
inline int band_level(int L, int num) { return num == 0 ? L : (num - 1) / 3 + 1; }
}  // namespace
#define ON_MY_DEVICE_B() DevScopeB dev_scope_(priv_)

int BoundaryWavelets::geometry(int Nr, int Nc, int hlen, int levels, int* nr, int* nc)
{
    if (Nr < 1 || Nc < 1 || hlen < 2 || hlen > PDWT_MAX_FILTER_WIDTH || (hlen & 1)) return 0;
    if ((unsigned long long)Nr * (unsigned long long)Nc >= (1ull << 31)) return 0;
    if (levels < 1) levels = 1;
    int wmaxlev = w_ilog2((Nr < Nc ? Nr : Nc) / (hlen - 1));  // the rule of Wavelets (src/wt.cu:155-165) = PyWavelets' dwt_max_level
    if (wmaxlev > kL) wmaxlev = kL;
    if (levels > wmaxlev) levels = wmaxlev;
    for (int l = 0; l <= levels; l++) {
        if (nr) nr[l] = Nr;
        if (nc) nc[l] = Nc;
        Nr = (Nr + hlen - 1) >> 1, Nc = (Nc + hlen - 1) >> 1;
    }
    return levels;
}

int BoundaryWavelets::mode_index(const char* name)
{
    if (!name) return -1;
    for (int m = 0; m < BW_NUM_MODES; m++)
        if (!strcmp(name, kModeNames[m])) return m;
    return -1;
}

BoundaryWavelets::BoundaryWavelets(DTYPE* img, int Nr, int Nc, const char* wname_, int levels, int mode, int memisonhost)
    : d_image(NULL), d_coeffs(NULL), state(W_INIT), priv_(NULL)
{
    winfos.Nr = Nr, winfos.Nc = Nc, winfos.nlevels = levels, winfos.hlen = 0, winfos.mode = mode;
    strncpy(wname, wname_ ? wname_ : "", 127);
    wname[127] = 0;
    if (Nr < 1 || Nc < 1 || !wname_ || (unsigned long long)Nr * (unsigned long long)Nc >= (1ull << 31)) {
        puts("ERROR: BoundaryWavelets(): invalid image size or wavelet name");
        state = W_CREATION_ERROR;
        return;
    }
    if (mode < 0 || mode >= BW_NUM_MODES) {
        printf("ERROR: BoundaryWavelets(): unknown boundary mode %d (0 zero, 1 constant, 2 symmetric, 3 reflect, 4 periodic)\n", mode);
        state = W_CREATION_ERROR;
        return;
    }
    if (levels < 1) {
        puts("Warning: cannot initialize wavelet coefficients with nlevels < 1. Forcing nlevels = 1");
        winfos.nlevels = 1;
    }
    bw_priv* p = new (std::nothrow) bw_priv();
    if (!p) {
        state = W_CREATION_ERROR;
        return;
    }
    priv_ = p;
    p->d_bands = NULL, p->d_ping[0] = p->d_ping[1] = NULL;
    p->dev = pdwt_get_device();
    const int hlen = SFX(pdwt_compute_filters_separable)(wname, 0, &p->f);
    if (hlen <= 0) {
        printf("ERROR: unknown wavelet name %s\n", wname);
        state = W_CREATION_ERROR;
        return;
    }
    p->f.hlen = hlen;
    winfos.hlen = hlen;
    const int wmaxlev = geometry(Nr, Nc, hlen, winfos.nlevels, p->nr, p->nc);
    if (winfos.nlevels > wmaxlev) {
        printf("Warning: required level (%d) is greater than the maximum possible level for %s (%d) on a %dx%d image.\n", winfos.nlevels, wname, wmaxlev, Nr, Nc);
        printf("Forcing nlevels = %d\n", wmaxlev);
        winfos.nlevels = wmaxlev;
    }
    if (winfos.nlevels < 1) {
        printf("ERROR: a %dx%d image is too small for one level of %s\n", Nr, Nc, wname);
        state = W_CREATION_ERROR;
        return;
    }
    const int L = winfos.nlevels, nb = 3 * L + 1;
    size_t off[pdwt_bl::kMaxBands], total = 0;
    for (int k = 0; k < nb; k++) {
        const int l = band_level(L, k);
        off[k] = total;
        total += ((size_t)p->nr[l] * p->nc[l] * sizeof(DTYPE) + 255) & ~(size_t)255;
    }
    const size_t n = (size_t)Nr * Nc, n1 = (size_t)p->nr[1] * p->nc[1];
    d_image = (DTYPE*)pdwt_malloc(n * sizeof(DTYPE));
    p->d_bands = (DTYPE*)pdwt_malloc(total);
    d_coeffs = (DTYPE**)calloc((size_t)nb, sizeof(DTYPE*));
    int rc = (d_image && p->d_bands && d_coeffs) ? PDWT_OK : PDWT_ENOMEM;
    if (rc == PDWT_OK && L > 1) {
        p->d_ping[0] = (DTYPE*)pdwt_malloc(n1 * sizeof(DTYPE));
        p->d_ping[1] = (DTYPE*)pdwt_malloc(n1 * sizeof(DTYPE));
        if (!p->d_ping[0] || !p->d_ping[1]) rc = PDWT_ENOMEM;
    }
    if (rc == PDWT_OK) {
        for (int k = 0; k < nb; k++) d_coeffs[k] = (DTYPE*)((char*)p->d_bands + off[k]);
        rc = pdwt_memset(p->d_bands, 0, total);
    }
    if (rc == PDWT_OK) {
        if (!img) rc = pdwt_memset(d_image, 0, n * sizeof(DTYPE));
        else if (memisonhost) rc = pdwt_memcpy_h2d(d_image, img, n * sizeof(DTYPE));
        else rc = pdwt_memcpy_d2d_foreign(d_image, img, n * sizeof(DTYPE));
    }
    if (rc != PDWT_OK) {
        report("(): allocation or upload", rc);
        state = W_CREATION_ERROR;
    }
}

BoundaryWavelets::~BoundaryWavelets()
{
    ON_MY_DEVICE_B();
    if (d_image) pdwt_free(d_image);
    free(d_coeffs);
    if (priv_) {
        bw_priv* p = P(priv_);
        if (p->d_bands) pdwt_free(p->d_bands);
        if (p->d_ping[0]) pdwt_free(p->d_ping[0]);
        if (p->d_ping[1]) pdwt_free(p->d_ping[1]);
        delete p;
    }
}

// The approximation of level l (1 .. L): band 0 for l == L, else a ping buffer.  Level l is written from level l - 1 (forward) or read
// to rebuild it (inverse), so consecutive levels alternate between the two buffers and neither direction touches a band it reads.
static DTYPE* approx_of(const BoundaryWavelets& W, bw_priv* p, int l) { return l == W.winfos.nlevels ? W.d_coeffs[0] : p->d_ping[(l - 1) & 1]; }

void BoundaryWavelets::forward()
{
    ON_MY_DEVICE_B();
    if (state == W_CREATION_ERROR) {
        puts("Warning: forward transform not computed, as there was an error when creating the wavelets");
        return;
    }
    bw_priv* p = P(priv_);
    const DTYPE* src = d_image;
    for (int l = 1; l <= winfos.nlevels; l++) {
        DTYPE* a = approx_of(*this, p, l);
        DTYPE** b = d_coeffs + 3 * (l - 1) + 1;
        const int rc = SFX(pdwt_ext2d_forward_level)(src, a, b[0], b[1], b[2], p->nr[l - 1], p->nc[l - 1], winfos.mode, &p->f);
        if (rc != PDWT_OK) {
            report("::forward()", rc);
            state = W_FORWARD_ERROR;
            return;
        }
        src = a;
    }
    state = W_FORWARD;
}

void BoundaryWavelets::inverse()
{
    ON_MY_DEVICE_B();
    if (state == W_INVERSE) {
        puts("Warning: W.inverse() has already been run. Inverse is available in W.get_image()");
        return;
    }
    if (state == W_CREATION_ERROR || state == W_FORWARD_ERROR || state == W_THRESHOLD_ERROR) {
        puts("Warning: inverse transform not computed, as there was an error in a previous stage");
        return;
    }
    bw_priv* p = P(priv_);
    for (int l = winfos.nlevels; l >= 1; l--) {
        DTYPE* dst = l == 1 ? d_image : approx_of(*this, p, l - 1);
        DTYPE** b = d_coeffs + 3 * (l - 1) + 1;
        const int rc = SFX(pdwt_ext2d_inverse_level)(dst, approx_of(*this, p, l), b[0], b[1], b[2], p->nr[l - 1], p->nc[l - 1], &p->f);
        if (rc != PDWT_OK) {
            report("::inverse()", rc);
            state = W_INVERSE_ERROR;
            return;
        }
    }
    state = W_INVERSE;
}

int BoundaryWavelets::get_image(DTYPE* res)
{
    ON_MY_DEVICE_B();
    if (!d_image || !res || state == W_CREATION_ERROR) return 0;
    const size_t n = (size_t)winfos.Nr * winfos.Nc;
    if (pdwt_memcpy_d2h(res, d_image, n * sizeof(DTYPE)) != PDWT_OK) return 0;
    return (int)n;
}

void BoundaryWavelets::set_image(DTYPE* img, int mem_is_on_device)
{
    ON_MY_DEVICE_B();
    if (!d_image || !img || state == W_CREATION_ERROR) return;
    const size_t nb = (size_t)winfos.Nr * winfos.Nc * sizeof(DTYPE);
    const int rc = mem_is_on_device ? pdwt_memcpy_d2d_foreign(d_image, img, nb) : pdwt_memcpy_h2d(d_image, img, nb);
    if (rc != PDWT_OK) report("::set_image()", rc);
    state = W_INIT;
}

int BoundaryWavelets::num_bands() const { return state == W_CREATION_ERROR ? 0 : 3 * winfos.nlevels + 1; }

long long BoundaryWavelets::coeff_shape(int num, int* nr, int* nc) const
{
    if (state == W_CREATION_ERROR || num < 0 || num >= num_bands()) return 0;
    const bw_priv* p = P(priv_);
    const int l = band_level(winfos.nlevels, num);
    if (nr) *nr = p->nr[l];
    if (nc) *nc = p->nc[l];
    return (long long)p->nr[l] * p->nc[l];
}

int BoundaryWavelets::get_coeff(DTYPE* coeff, int num)
{
    ON_MY_DEVICE_B();
    if (state == W_INVERSE) {
        puts("Warning: get_coeff(): inverse() has been performed; run forward() first.");
        return 0;
    }
    const long long n = coeff_shape(num, NULL, NULL);
    if (n <= 0 || !coeff) return 0;
    if (pdwt_memcpy_d2h(coeff, d_coeffs[num], (size_t)n * sizeof(DTYPE)) != PDWT_OK) return 0;
    return (int)n;
}

void BoundaryWavelets::set_coeff(DTYPE* coeff, int num, int mem_is_on_device)
{
    ON_MY_DEVICE_B();
    const long long n = coeff_shape(num, NULL, NULL);
    if (n <= 0 || !coeff) {
        if (state != W_CREATION_ERROR) printf("ERROR: set_coeff(): invalid coefficient index %d\n", num);
        return;
    }
    const size_t nb = (size_t)n * sizeof(DTYPE);
    const int rc = mem_is_on_device ? pdwt_memcpy_d2d_foreign(d_coeffs[num], coeff, nb) : pdwt_memcpy_h2d(d_coeffs[num], coeff, nb);
    if (rc != PDWT_OK) report("::set_coeff()", rc);
}

intptr_t BoundaryWavelets::image_int_ptr() { return (intptr_t)d_image; }
intptr_t BoundaryWavelets::coeff_int_ptr(int num) { return coeff_shape(num, NULL, NULL) > 0 ? (intptr_t)d_coeffs[num] : 0; }

// ---- the band list (bandstats_host.hpp) ------------------------------------------------------------------------------------------
// pointer and size of every band; nb = 0 when the coefficients are not there to be read (need_forward: only those of a forward())
static pdwt_bl::BandList band_list(const BoundaryWavelets& W, bool need_forward)
{
    pdwt_bl::BandList bl;
    bl.nb = 0;
    if (W.state == W_CREATION_ERROR || W.state == W_INVERSE || !W.d_coeffs) return bl;
    if (need_forward && !(W.state == W_FORWARD || W.state == W_THRESHOLD)) return bl;
    const int nb = W.num_bands();
    for (int k = 0; k < nb; k++) {
        bl.ptr[k] = W.d_coeffs[k];
        bl.n[k] = (size_t)W.coeff_shape(k, NULL, NULL);
    }
    bl.nb = nb;
    bl.finest = 3;  // D1
    bl.samples = (double)W.winfos.Nr * W.winfos.Nc;
    return bl;
}

void BoundaryWavelets::threshold(int op, DTYPE beta, int do_thresh_appcoeffs)
{
    ON_MY_DEVICE_B();
    if (state == W_INVERSE) {
        puts("Warning: BoundaryWavelets(): cannot threshold coefficients after W.inverse() (run forward() first)");
        return;
    }
    const pdwt_bl::BandList bl = band_list(*this, false);
    if (!bl.nb) return;
    DTYPE betas[pdwt_bl::kMaxBands];
    for (int k = 0; k < bl.nb; k++) betas[k] = beta;
    if (!do_thresh_appcoeffs) betas[0] = (DTYPE)-1;  // (a negative beta leaves the band alone)
    const int rc = pdwt_bl::threshold(bl, betas, op);
    if (rc != PDWT_OK) {
        report(op ? "::hard_threshold()" : "::soft_threshold()", rc);
        state = W_THRESHOLD_ERROR;
    }
}
void BoundaryWavelets::soft_threshold(DTYPE beta, int do_thresh_appcoeffs) { threshold(0, beta, do_thresh_appcoeffs); }
void BoundaryWavelets::hard_threshold(DTYPE beta, int do_thresh_appcoeffs) { threshold(1, beta, do_thresh_appcoeffs); }

double BoundaryWavelets::norm1()
{
    ON_MY_DEVICE_B();
    const pdwt_bl::BandList bl = band_list(*this, false);
    if (!bl.nb) return -1.0;
    w_band_stats s[pdwt_bl::kMaxBands];
    const int rc = pdwt_bl::stats(bl, -1, s, 0);
    if (rc != PDWT_OK) {
        report("::norm1()", rc);
        return -1.0;
    }
    double sum = 0.0;
    for (int k = 0; k < bl.nb; k++) sum += s[k].sum_abs;
    return sum;
}

int BoundaryWavelets::band_stats(int num, w_band_stats* out, int with_median)
{
    ON_MY_DEVICE_B();
    const pdwt_bl::BandList bl = band_list(*this, true);
    if (!bl.nb || num < 0 || num >= bl.nb || !out) return PDWT_EINVAL;
    const int rc = pdwt_bl::stats(bl, num, out, with_median);
    if (rc != PDWT_OK) report("::band_stats()", rc);
    return rc;
}

int BoundaryWavelets::all_band_stats(w_band_stats* out, int with_median)
{
    ON_MY_DEVICE_B();
    const pdwt_bl::BandList bl = band_list(*this, true);
    if (!bl.nb || !out) return PDWT_EINVAL;
    const int rc = pdwt_bl::stats(bl, -1, out, with_median);
    if (rc != PDWT_OK) report("::all_band_stats()", rc);
    return rc;
}

double BoundaryWavelets::estimate_sigma()
{
    ON_MY_DEVICE_B();
    const pdwt_bl::BandList bl = band_list(*this, true);
    double sigma = -1.0;
    if (!bl.nb) return -1.0;
    const int rc = pdwt_bl::estimate_sigma(bl, &sigma);
    if (rc != PDWT_OK) {
        report("::estimate_sigma()", rc);
        return -1.0;
    }
    return sigma;
}

void BoundaryWavelets::threshold_bands(const DTYPE* betas, int kind)
{
    ON_MY_DEVICE_B();
    const pdwt_bl::BandList bl = band_list(*this, true);
    if (!bl.nb || !betas || (kind != 0 && kind != 1)) return;
    const int rc = pdwt_bl::threshold(bl, betas, kind);
    if (rc != PDWT_OK) {
        report("::threshold_bands()", rc);
        state = W_THRESHOLD_ERROR;
    }
}

double BoundaryWavelets::denoise(int method, double sigma, int kind, DTYPE* betas_out)
{
    ON_MY_DEVICE_B();
    const pdwt_bl::BandList bl = band_list(*this, true);
    if (!bl.nb || (method != 0 && method != 1) || (kind != 0 && kind != 1)) return -1.0;
    DTYPE betas[pdwt_bl::kMaxBands];
    const int rc = pdwt_bl::denoise(bl, method, kind, &sigma, betas);
    if (rc != PDWT_OK) {
        report("::denoise()", rc);
        state = W_THRESHOLD_ERROR;
        return -1.0;
    }
    if (betas_out) memcpy(betas_out, betas, (size_t)bl.nb * sizeof(DTYPE));
    return sigma;
}

// ---- flat C handle API (pdwt_amd/boundary.py) ---------------------------------------------------------------
#define BW(h) static_cast<BoundaryWavelets*>(h)
extern "C" {
void* pdwt_bw_new(DTYPE* img, int Nr, int Nc, const char* wname, int levels, int mode, int memisonhost)
{
    return new (std::nothrow) BoundaryWavelets(img, Nr, Nc, wname, levels, mode, memisonhost);
}
void pdwt_bw_delete(void* h) { delete BW(h); }
void pdwt_bw_forward(void* h) { BW(h)->forward(); }
void pdwt_bw_inverse(void* h) { BW(h)->inverse(); }
int pdwt_bw_get_image(void* h, DTYPE* out) { return BW(h)->get_image(out); }
void pdwt_bw_set_image(void* h, DTYPE* img, int mem_is_on_device) { BW(h)->set_image(img, mem_is_on_device); }
int pdwt_bw_state(void* h) { return (int)BW(h)->state; }
void pdwt_bw_info(void* h, w_info_bw* out) { *out = BW(h)->winfos; }
int pdwt_bw_geometry(int Nr, int Nc, int hlen, int levels, int* nr, int* nc) { return BoundaryWavelets::geometry(Nr, Nc, hlen, levels, nr, nc); }
int pdwt_bw_mode_index(const char* name) { return BoundaryWavelets::mode_index(name); }
int pdwt_bw_num_bands(void* h) { return BW(h)->num_bands(); }
long long pdwt_bw_coeff_shape(void* h, int num, int* nr, int* nc) { return BW(h)->coeff_shape(num, nr, nc); }
int pdwt_bw_get_coeff(void* h, DTYPE* out, int num) { return BW(h)->get_coeff(out, num); }
void pdwt_bw_set_coeff(void* h, DTYPE* in, int num, int mem_is_on_device) { BW(h)->set_coeff(in, num, mem_is_on_device); }
intptr_t pdwt_bw_image_int_ptr(void* h) { return BW(h)->image_int_ptr(); }
intptr_t pdwt_bw_coeff_int_ptr(void* h, int num) { return BW(h)->coeff_int_ptr(num); }
void pdwt_bw_soft_threshold(void* h, DTYPE beta, int app) { BW(h)->soft_threshold(beta, app); }
void pdwt_bw_hard_threshold(void* h, DTYPE beta, int app) { BW(h)->hard_threshold(beta, app); }
double pdwt_bw_norm1(void* h) { return BW(h)->norm1(); }
int pdwt_bw_band_stats(void* h, int num, w_band_stats* out, int with_median) { return BW(h)->band_stats(num, out, with_median); }
int pdwt_bw_all_band_stats(void* h, w_band_stats* out, int with_median) { return BW(h)->all_band_stats(out, with_median); }
double pdwt_bw_estimate_sigma(void* h) { return BW(h)->estimate_sigma(); }
void pdwt_bw_threshold_bands(void* h, const DTYPE* betas, int kind) { BW(h)->threshold_bands(betas, kind); }
double pdwt_bw_denoise(void* h, int method, double sigma, int kind, DTYPE* betas_out) { return BW(h)->denoise(method, sigma, kind, betas_out); }
}
#undef BW

// =====================================================================================================================================
// BoundaryWavelets1D: the same along the last axis of an Nr x Nc batch of rows (include/pdwt_hip.h "Batched 1-D DWT with boundary
// modes").  The whole-transform entries choose between the one-launch kernels and the per-level loop; this class owns the band table and
// the scratch of the loop, and shares the band-list code above.
// =====================================================================================================================================
namespace {
struct bw1_priv {
    bw_filters_t f;
    int dev;        // the device current at construction; every method runs there
    int n[kL + 1];  // [0] the samples of a row, [l] the coefficients per row of level l
    int fused;      // the transforms of this instance are one launch each
    DTYPE* d_bands; // the one allocation behind d_coeffs
    DTYPE* d_tmp;   // the intermediate approximations of the per-level path; NULL when fused or for one level
};
static_assert(offsetof(bw1_priv, dev) == offsetof(bw_priv, dev), "DevScopeB reads the device of either class");
inline bw1_priv* P1(void* p) { return (bw1_priv*)p; }
void report1(const char* where, int rc) { printf("ERROR: BoundaryWavelets1D%s failed (code %d): %s\n", where, rc, pdwt_last_error_string()); }
}  // namespace

int BoundaryWavelets1D::geometry(int Nc, int hlen, int levels, int* n)
{
    if (Nc < 1 || hlen < 2 || hlen > PDWT_MAX_FILTER_WIDTH || (hlen & 1)) return 0;
    if (levels < 1) levels = 1;
    int wmaxlev = w_ilog2(Nc / (hlen - 1));  // the batched-1-D rule of Wavelets = PyWavelets' dwt_max_level
    if (wmaxlev > kL) wmaxlev = kL;
    if (levels > wmaxlev) levels = wmaxlev;
    for (int l = 0; l <= levels; l++) {
        if (n) n[l] = Nc;
        Nc = (Nc + hlen - 1) >> 1;
    }
    return levels;
}

BoundaryWavelets1D::BoundaryWavelets1D(DTYPE* img, int Nr, int Nc, const char* wname_, int levels, int mode, int memisonhost)
    : d_image(NULL), d_coeffs(NULL), state(W_INIT), priv_(NULL)
{
    winfos.Nr = Nr, winfos.Nc = Nc, winfos.nlevels = levels, winfos.hlen = 0, winfos.mode = mode;
    strncpy(wname, wname_ ? wname_ : "", 127);
    wname[127] = 0;
    if (Nr < 1 || Nc < 1 || !wname_ || (unsigned long long)Nr * (unsigned long long)Nc >= (1ull << 31)) {
        puts("ERROR: BoundaryWavelets1D(): invalid batch size or wavelet name");
        state = W_CREATION_ERROR;
        return;
    }
    if (mode < 0 || mode >= BW_NUM_MODES) {
        printf("ERROR: BoundaryWavelets1D(): unknown boundary mode %d (0 zero, 1 constant, 2 symmetric, 3 reflect, 4 periodic)\n", mode);
        state = W_CREATION_ERROR;
        return;
    }
    if (levels < 1) {
        puts("Warning: cannot initialize wavelet coefficients with nlevels < 1. Forcing nlevels = 1");
        winfos.nlevels = 1;
    }
    bw1_priv* p = new (std::nothrow) bw1_priv();
    if (!p) {
        state = W_CREATION_ERROR;
        return;
    }
    priv_ = p;
    p->d_bands = p->d_tmp = NULL, p->fused = 0;
    p->dev = pdwt_get_device();
    const int hlen = SFX(pdwt_compute_filters_separable)(wname, 0, &p->f);
    if (hlen <= 0) {
        printf("ERROR: unknown wavelet name %s\n", wname);
        state = W_CREATION_ERROR;
        return;
    }
    p->f.hlen = hlen;
    winfos.hlen = hlen;
    const int wmaxlev = geometry(Nc, hlen, winfos.nlevels, p->n);
    if (winfos.nlevels > wmaxlev) {
        printf("Warning: required level (%d) is greater than the maximum possible level for %s (%d) on rows of %d samples.\n", winfos.nlevels, wname, wmaxlev, Nc);
        printf("Forcing nlevels = %d\n", wmaxlev);
        winfos.nlevels = wmaxlev;
    }
    if (winfos.nlevels < 1) {
        printf("ERROR: rows of %d samples are too short for one level of %s\n", Nc, wname);
        state = W_CREATION_ERROR;
        return;
    }
    const int L = winfos.nlevels, nb = L + 1;
    size_t off[kL + 1], total = 0;
    for (int k = 0; k < nb; k++) {
        off[k] = total;
        total += ((size_t)Nr * p->n[k == 0 ? L : k] * sizeof(DTYPE) + 255) & ~(size_t)255;
    }
    const size_t n = (size_t)Nr * Nc;
    const long long ntmp = pdwt_ext1d_tmp_elems(Nr, Nc, hlen, L, (int)sizeof(DTYPE));
    p->fused = pdwt_ext1d_fused(Nc, hlen, L, (int)sizeof(DTYPE)) == 1;
    d_image = (DTYPE*)pdwt_malloc(n * sizeof(DTYPE));
    p->d_bands = (DTYPE*)pdwt_malloc(total);
    d_coeffs = (DTYPE**)calloc((size_t)nb, sizeof(DTYPE*));
    int rc = (d_image && p->d_bands && d_coeffs && ntmp >= 0) ? PDWT_OK : PDWT_ENOMEM;
    if (rc == PDWT_OK && ntmp > 0) {
        p->d_tmp = (DTYPE*)pdwt_malloc((size_t)ntmp * sizeof(DTYPE));
        if (!p->d_tmp) rc = PDWT_ENOMEM;
    }
    if (rc == PDWT_OK) {
        for (int k = 0; k < nb; k++) d_coeffs[k] = (DTYPE*)((char*)p->d_bands + off[k]);
        rc = pdwt_memset(p->d_bands, 0, total);
    }
    if (rc == PDWT_OK) {
        if (!img) rc = pdwt_memset(d_image, 0, n * sizeof(DTYPE));
        else if (memisonhost) rc = pdwt_memcpy_h2d(d_image, img, n * sizeof(DTYPE));
        else rc = pdwt_memcpy_d2d_foreign(d_image, img, n * sizeof(DTYPE));
    }
    if (rc != PDWT_OK) {
        report1("(): allocation or upload", rc);
        state = W_CREATION_ERROR;
    }
}

BoundaryWavelets1D::~BoundaryWavelets1D()
{
    ON_MY_DEVICE_B();
    if (d_image) pdwt_free(d_image);
    free(d_coeffs);
    if (priv_) {
        bw1_priv* p = P1(priv_);
        if (p->d_bands) pdwt_free(p->d_bands);
        if (p->d_tmp) pdwt_free(p->d_tmp);
        delete p;
    }
}

void BoundaryWavelets1D::forward()
{
    ON_MY_DEVICE_B();
    if (state == W_CREATION_ERROR) {
        puts("Warning: forward transform not computed, as there was an error when creating the wavelets");
        return;
    }
    bw1_priv* p = P1(priv_);
    const int rc = SFX(pdwt_ext1d_forward)(d_image, d_coeffs, winfos.Nr, winfos.Nc, winfos.nlevels, winfos.mode, &p->f, p->d_tmp);
    if (rc < 0) {
        report1("::forward()", rc);
        state = W_FORWARD_ERROR;
        return;
    }
    state = W_FORWARD;
}

void BoundaryWavelets1D::inverse()
{
    ON_MY_DEVICE_B();
    if (state == W_INVERSE) {
        puts("Warning: W.inverse() has already been run. Inverse is available in W.get_image()");
        return;
    }
    if (state == W_CREATION_ERROR || state == W_FORWARD_ERROR || state == W_THRESHOLD_ERROR) {
        puts("Warning: inverse transform not computed, as there was an error in a previous stage");
        return;
    }
    bw1_priv* p = P1(priv_);
    const int rc = SFX(pdwt_ext1d_inverse)(d_image, d_coeffs, winfos.Nr, winfos.Nc, winfos.nlevels, &p->f, p->d_tmp);
    if (rc < 0) {
        report1("::inverse()", rc);
        state = W_INVERSE_ERROR;
        return;
    }
    state = W_INVERSE;
}

int BoundaryWavelets1D::get_image(DTYPE* res)
{
    ON_MY_DEVICE_B();
    if (!d_image || !res || state == W_CREATION_ERROR) return 0;
    const size_t n = (size_t)winfos.Nr * winfos.Nc;
    if (pdwt_memcpy_d2h(res, d_image, n * sizeof(DTYPE)) != PDWT_OK) return 0;
    return (int)n;
}

void BoundaryWavelets1D::set_image(DTYPE* img, int mem_is_on_device)
{
    ON_MY_DEVICE_B();
    if (!d_image || !img || state == W_CREATION_ERROR) return;
    const size_t nb = (size_t)winfos.Nr * winfos.Nc * sizeof(DTYPE);
    const int rc = mem_is_on_device ? pdwt_memcpy_d2d_foreign(d_image, img, nb) : pdwt_memcpy_h2d(d_image, img, nb);
    if (rc != PDWT_OK) report1("::set_image()", rc);
    state = W_INIT;
}

int BoundaryWavelets1D::num_bands() const { return state == W_CREATION_ERROR ? 0 : winfos.nlevels + 1; }
int BoundaryWavelets1D::fused() const { return state == W_CREATION_ERROR || !priv_ ? 0 : P1(priv_)->fused; }

long long BoundaryWavelets1D::coeff_shape(int num, int* nr, int* nc) const
{
    if (state == W_CREATION_ERROR || num < 0 || num >= num_bands()) return 0;
    const int len = P1(priv_)->n[num == 0 ? winfos.nlevels : num];
    if (nr) *nr = winfos.Nr;
    if (nc) *nc = len;
    return (long long)winfos.Nr * len;
}

int BoundaryWavelets1D::get_coeff(DTYPE* coeff, int num)
{
    ON_MY_DEVICE_B();
    if (state == W_INVERSE) {
        puts("Warning: get_coeff(): inverse() has been performed; run forward() first.");
        return 0;
    }
    const long long n = coeff_shape(num, NULL, NULL);
    if (n <= 0 || !coeff) return 0;
    if (pdwt_memcpy_d2h(coeff, d_coeffs[num], (size_t)n * sizeof(DTYPE)) != PDWT_OK) return 0;
    return (int)n;
}

void BoundaryWavelets1D::set_coeff(DTYPE* coeff, int num, int mem_is_on_device)
{
    ON_MY_DEVICE_B();
    const long long n = coeff_shape(num, NULL, NULL);
    if (n <= 0 || !coeff) {
        if (state != W_CREATION_ERROR) printf("ERROR: set_coeff(): invalid coefficient index %d\n", num);
        return;
    }
    const size_t nb = (size_t)n * sizeof(DTYPE);
    const int rc = mem_is_on_device ? pdwt_memcpy_d2d_foreign(d_coeffs[num], coeff, nb) : pdwt_memcpy_h2d(d_coeffs[num], coeff, nb);
    if (rc != PDWT_OK) report1("::set_coeff()", rc);
}

intptr_t BoundaryWavelets1D::image_int_ptr() { return (intptr_t)d_image; }
intptr_t BoundaryWavelets1D::coeff_int_ptr(int num) { return coeff_shape(num, NULL, NULL) > 0 ? (intptr_t)d_coeffs[num] : 0; }

static pdwt_bl::BandList band_list(const BoundaryWavelets1D& W, bool need_forward)
{
    pdwt_bl::BandList bl;
    bl.nb = 0;
    if (W.state == W_CREATION_ERROR || W.state == W_INVERSE || !W.d_coeffs) return bl;
    if (need_forward && !(W.state == W_FORWARD || W.state == W_THRESHOLD)) return bl;
    const int nb = W.num_bands();
    for (int k = 0; k < nb; k++) {
        bl.ptr[k] = W.d_coeffs[k];
        bl.n[k] = (size_t)W.coeff_shape(k, NULL, NULL);
    }
    bl.nb = nb;
    bl.finest = 1;  // D1, all rows together
    bl.samples = (double)W.winfos.Nc;  // the batched-1-D rule of wt.h: N of the universal threshold is the length of a signal
    return bl;
}

void BoundaryWavelets1D::threshold(int op, DTYPE beta, int do_thresh_appcoeffs)
{
    ON_MY_DEVICE_B();
    if (state == W_INVERSE) {
        puts("Warning: BoundaryWavelets1D(): cannot threshold coefficients after W.inverse() (run forward() first)");
        return;
    }
    const pdwt_bl::BandList bl = band_list(*this, false);
    if (!bl.nb) return;
    DTYPE betas[pdwt_bl::kMaxBands];
    for (int k = 0; k < bl.nb; k++) betas[k] = beta;
    if (!do_thresh_appcoeffs) betas[0] = (DTYPE)-1;
    const int rc = pdwt_bl::threshold(bl, betas, op);
    if (rc != PDWT_OK) {
        report1(op ? "::hard_threshold()" : "::soft_threshold()", rc);
        state = W_THRESHOLD_ERROR;
    }
}
void BoundaryWavelets1D::soft_threshold(DTYPE beta, int do_thresh_appcoeffs) { threshold(0, beta, do_thresh_appcoeffs); }
void BoundaryWavelets1D::hard_threshold(DTYPE beta, int do_thresh_appcoeffs) { threshold(1, beta, do_thresh_appcoeffs); }

double BoundaryWavelets1D::norm1()
{
    ON_MY_DEVICE_B();
    const pdwt_bl::BandList bl = band_list(*this, false);
    if (!bl.nb) return -1.0;
    w_band_stats s[pdwt_bl::kMaxBands];
    const int rc = pdwt_bl::stats(bl, -1, s, 0);
    if (rc != PDWT_OK) {
        report1("::norm1()", rc);
        return -1.0;
    }
    double sum = 0.0;
    for (int k = 0; k < bl.nb; k++) sum += s[k].sum_abs;
    return sum;
}

int BoundaryWavelets1D::band_stats(int num, w_band_stats* out, int with_median)
{
    ON_MY_DEVICE_B();
    const pdwt_bl::BandList bl = band_list(*this, true);
    if (!bl.nb || num < 0 || num >= bl.nb || !out) return PDWT_EINVAL;
    const int rc = pdwt_bl::stats(bl, num, out, with_median);
    if (rc != PDWT_OK) report1("::band_stats()", rc);
    return rc;
}

int BoundaryWavelets1D::all_band_stats(w_band_stats* out, int with_median)
{
    ON_MY_DEVICE_B();
    const pdwt_bl::BandList bl = band_list(*this, true);
    if (!bl.nb || !out) return PDWT_EINVAL;
    const int rc = pdwt_bl::stats(bl, -1, out, with_median);
    if (rc != PDWT_OK) report1("::all_band_stats()", rc);
    return rc;
}

double BoundaryWavelets1D::estimate_sigma()
{
    ON_MY_DEVICE_B();
    const pdwt_bl::BandList bl = band_list(*this, true);
    double sigma = -1.0;
    if (!bl.nb) return -1.0;
    const int rc = pdwt_bl::estimate_sigma(bl, &sigma);
    if (rc != PDWT_OK) {
        report1("::estimate_sigma()", rc);
        return -1.0;
    }
    return sigma;
}

void BoundaryWavelets1D::threshold_bands(const DTYPE* betas, int kind)
{
    ON_MY_DEVICE_B();
    const pdwt_bl::BandList bl = band_list(*this, true);
    if (!bl.nb || !betas || (kind != 0 && kind != 1)) return;
    const int rc = pdwt_bl::threshold(bl, betas, kind);
    if (rc != PDWT_OK) {
        report1("::threshold_bands()", rc);
        state = W_THRESHOLD_ERROR;
    }
}

double BoundaryWavelets1D::denoise(int method, double sigma, int kind, DTYPE* betas_out)
{
    ON_MY_DEVICE_B();
    const pdwt_bl::BandList bl = band_list(*this, true);
    if (!bl.nb || (method != 0 && method != 1) || (kind != 0 && kind != 1)) return -1.0;
    DTYPE betas[pdwt_bl::kMaxBands];
    const int rc = pdwt_bl::denoise(bl, method, kind, &sigma, betas);
    if (rc != PDWT_OK) {
        report1("::denoise()", rc);
        state = W_THRESHOLD_ERROR;
        return -1.0;
    }
    if (betas_out) memcpy(betas_out, betas, (size_t)bl.nb * sizeof(DTYPE));
    return sigma;
}

// ---- flat C handle API (pdwt_amd/boundary.py), name for name with pdwt_bw_* --------------------------------------
#define BW1(h) static_cast<BoundaryWavelets1D*>(h)
extern "C" {
void* pdwt_bw1_new(DTYPE* img, int Nr, int Nc, const char* wname, int levels, int mode, int memisonhost)
{
    return new (std::nothrow) BoundaryWavelets1D(img, Nr, Nc, wname, levels, mode, memisonhost);
}
void pdwt_bw1_delete(void* h) { delete BW1(h); }
void pdwt_bw1_forward(void* h) { BW1(h)->forward(); }
void pdwt_bw1_inverse(void* h) { BW1(h)->inverse(); }
int pdwt_bw1_get_image(void* h, DTYPE* out) { return BW1(h)->get_image(out); }
void pdwt_bw1_set_image(void* h, DTYPE* img, int mem_is_on_device) { BW1(h)->set_image(img, mem_is_on_device); }
int pdwt_bw1_state(void* h) { return (int)BW1(h)->state; }
void pdwt_bw1_info(void* h, w_info_bw* out) { *out = BW1(h)->winfos; }
int pdwt_bw1_geometry(int Nc, int hlen, int levels, int* n) { return BoundaryWavelets1D::geometry(Nc, hlen, levels, n); }
int pdwt_bw1_mode_index(const char* name) { return BoundaryWavelets::mode_index(name); }
int pdwt_bw1_fused(void* h) { return BW1(h)->fused(); }
int pdwt_bw1_num_bands(void* h) { return BW1(h)->num_bands(); }
long long pdwt_bw1_coeff_shape(void* h, int num, int* nr, int* nc) { return BW1(h)->coeff_shape(num, nr, nc); }
int pdwt_bw1_get_coeff(void* h, DTYPE* out, int num) { return BW1(h)->get_coeff(out, num); }
void pdwt_bw1_set_coeff(void* h, DTYPE* in, int num, int mem_is_on_device) { BW1(h)->set_coeff(in, num, mem_is_on_device); }
intptr_t pdwt_bw1_image_int_ptr(void* h) { return BW1(h)->image_int_ptr(); }
intptr_t pdwt_bw1_coeff_int_ptr(void* h, int num) { return BW1(h)->coeff_int_ptr(num); }
void pdwt_bw1_soft_threshold(void* h, DTYPE beta, int app) { BW1(h)->soft_threshold(beta, app); }
void pdwt_bw1_hard_threshold(void* h, DTYPE beta, int app) { BW1(h)->hard_threshold(beta, app); }
double pdwt_bw1_norm1(void* h) { return BW1(h)->norm1(); }
int pdwt_bw1_band_stats(void* h, int num, w_band_stats* out, int with_median) { return BW1(h)->band_stats(num, out, with_median); }
int pdwt_bw1_all_band_stats(void* h, w_band_stats* out, int with_median) { return BW1(h)->all_band_stats(out, with_median); }
double pdwt_bw1_estimate_sigma(void* h) { return BW1(h)->estimate_sigma(); }
void pdwt_bw1_threshold_bands(void* h, const DTYPE* betas, int kind) { BW1(h)->threshold_bands(betas, kind); }
double pdwt_bw1_denoise(void* h, int method, double sigma, int kind, DTYPE* betas_out) { return BW1(h)->denoise(method, sigma, kind, betas_out); }
}
#undef BW1
