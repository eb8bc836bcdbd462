// swt3d.cpp -- host side of `StationaryWavelets3D` (include/swt3d.h) above the 3-D stationary entry points of
// include/pdwt_hip.h, and its flat C handle API (pdwt_swt3d_*).  The logic of wt3d.cpp (Wavelets3D) with the SWT entry points;
// built into libpdwt.so (float) and libpdwtd.so (-DDOUBLEPRECISION).  The state machine is the one of Wavelets / Wavelets3D.
#include <limits.h>
#include <new>
#include <string.h>

#include "../../include/pdwt_hip.h"
#include "../../include/swt3d.h"
#include "bandstats_host.hpp"


#ifndef DOUBLEPRECISION
#define SFX(name) name##_f32
typedef pdwt_filters_f32 filters3_t;
#else
#define SFX(name) name##_f64
typedef pdwt_filters_f64 filters3_t;
#endif

namespace {
struct state3_t {
    filters3_t f;
    int dev;  // the device current at construction; every method runs there
};
inline state3_t* S(void* p) { return (state3_t*)p; }
inline pdwt_info3d to_pdwt3(const w_info3d& w)
{
    pdwt_info3d p;
    memcpy(&p, &w, sizeof(p));
    return p;
}
struct DevScope3 {
    int prev, mine;
    explicit DevScope3(const void* st) : prev(-1), mine(st ? ((const state3_t*)st)->dev : -1)
    {
        if (mine < 0) return;
        prev = pdwt_get_device();
        if (prev != mine) pdwt_set_device(mine);
    }
    ~DevScope3()
    {
        if (mine >= 0 && prev >= 0 && prev != mine) pdwt_set_device(prev);
    }
};
void report3(const char* where, int rc) { printf("ERROR: %s failed (code %d): %s\n", where, rc, pdwt_last_error_string()); }
}  // namespace
#define ON_MY_DEVICE3() DevScope3 dev_scope_(filters_)

StationaryWavelets3D::StationaryWavelets3D(DTYPE* vol, int Nz, int Nr, int Nc, const char* wname_, int levels, int memisonhost)
    : d_image(NULL), d_coeffs(NULL), d_tmp(NULL), state(W_INIT), filters_(NULL)
{
    winfos.Nz = Nz;
    winfos.Nr = Nr;
    winfos.Nc = Nc;
    winfos.nlevels = levels;
    winfos.hlen = 0;
    strncpy(wname, wname_ ? wname_ : "", 127);
    wname[127] = 0;
    if (Nz < 1 || Nr < 1 || Nc < 1 || !wname_) {
        puts("ERROR: StationaryWavelets3D(): invalid volume size or wavelet name");
        state = W_CREATION_ERROR;
        return;
    }
    if (levels < 1) {
        puts("Warning: cannot initialize wavelet coefficients with nlevels < 1. Forcing nlevels = 1");
        winfos.nlevels = 1;
    }
    filters_ = calloc(1, sizeof(state3_t));
    if (!filters_) {
        state = W_CREATION_ERROR;
        return;
    }
    S(filters_)->dev = pdwt_get_device();
    const int hlen = SFX(pdwt_compute_filters_separable)(wname, 0, &S(filters_)->f);
    if (hlen <= 0) {
        printf("ERROR: unknown wavelet name %s\n", wname);
        state = W_CREATION_ERROR;
        return;
    }
    winfos.hlen = hlen;
    // the 2-D rule (src/wt.cu:155-165) with the third axis added
    int N = Nz < Nr ? Nz : Nr;
    if (Nc < N) N = Nc;
    const int wmaxlev = w_ilog2(N / (hlen - 1));
    if (winfos.nlevels > wmaxlev) {
        printf("Warning: required level (%d) is greater than the maximum possible level for %s (%d) on a %dx%dx%d volume.\n",
               winfos.nlevels, wname, wmaxlev, Nz, Nr, Nc);
        printf("Forcing nlevels = %d\n", wmaxlev);
        winfos.nlevels = wmaxlev;
    }
    if (winfos.nlevels < 1) {
        printf("ERROR: a %dx%dx%d volume is too small for one level of %s\n", Nz, Nr, Nc, wname);
        state = W_CREATION_ERROR;
        return;
    }
    const pdwt_info3d w = to_pdwt3(winfos);
    const size_t n = (size_t)Nz * Nr * Nc, ntmp = pdwt_tmp_elems_swt3d(w);
    if (ntmp == 0) {
        puts("ERROR: StationaryWavelets3D(): unsupported volume size (Nz <= 65535 and Nr * Nc < 2^31 are required)");
        state = W_CREATION_ERROR;
        return;
    }
    d_image = (DTYPE*)pdwt_malloc(n * sizeof(DTYPE));
    d_tmp = (DTYPE*)pdwt_malloc(ntmp * sizeof(DTYPE));
    d_coeffs = SFX(pdwt_create_coeffs_buffer_swt3d)(w);
    if (!d_image || !d_tmp || !d_coeffs) {
        printf("ERROR: StationaryWavelets3D(): device allocation failed: %s\n", pdwt_last_error_string());
        state = W_CREATION_ERROR;
        return;
    }
    int rc;
    if (!vol) rc = pdwt_memset(d_image, 0, n * sizeof(DTYPE));
    else if (memisonhost) rc = pdwt_memcpy_h2d(d_image, vol, n * sizeof(DTYPE));
    else rc = pdwt_memcpy_d2d_foreign(d_image, vol, n * sizeof(DTYPE));
    if (rc != PDWT_OK) {
        report3("StationaryWavelets3D(): volume upload", rc);
        state = W_CREATION_ERROR;
    }
}

StationaryWavelets3D::~StationaryWavelets3D()
{
    ON_MY_DEVICE3();
    if (d_image) pdwt_free(d_image);
    if (d_coeffs) SFX(pdwt_free_coeffs_buffer_swt3d)(d_coeffs, to_pdwt3(winfos));
    if (d_tmp) pdwt_free(d_tmp);
    free(filters_);
}

void StationaryWavelets3D::forward()
{
    ON_MY_DEVICE3();
    if (state == W_CREATION_ERROR) {
        puts("Warning: forward transform not computed, as there was an error when creating the wavelets");
        return;
    }
    const int rc = SFX(pdwt_forward3d_swt)(d_image, d_coeffs, d_tmp, to_pdwt3(winfos), &S(filters_)->f);
    if (rc != PDWT_OK) {
        report3("StationaryWavelets3D::forward()", rc);
        state = W_FORWARD_ERROR;
        return;
    }
    state = W_FORWARD;
}

void StationaryWavelets3D::inverse()
{
    ON_MY_DEVICE3();
    if (state == W_INVERSE) {
        puts("Warning: W.inverse() has already been run. Inverse is available in W.get_image()");
        return;
    }
    if (state == W_CREATION_ERROR || state == W_FORWARD_ERROR || state == W_THRESHOLD_ERROR) {
        puts("Warning: inverse transform not computed, as there was an error in a previous stage");
        return;
    }
    const int rc = SFX(pdwt_inverse3d_swt)(d_image, d_coeffs, d_tmp, to_pdwt3(winfos), &S(filters_)->f);
    if (rc != PDWT_OK) {
        report3("StationaryWavelets3D::inverse()", rc);
        state = W_INVERSE_ERROR;
        return;
    }
    state = W_INVERSE;
}

void StationaryWavelets3D::soft_threshold(DTYPE beta, int do_thresh_appcoeffs, int normalize)
{
    ON_MY_DEVICE3();
    if (state == W_INVERSE) {
        puts("Warning: StationaryWavelets3D(): cannot threshold coefficients after W.inverse() (run forward() first)");
        return;
    }
    if (state == W_CREATION_ERROR) return;
    const int rc = SFX(pdwt_soft_thresh_swt3d)(d_coeffs, beta, to_pdwt3(winfos), do_thresh_appcoeffs, normalize);
    if (rc != PDWT_OK) {
        report3("StationaryWavelets3D::soft_threshold()", rc);
        state = W_THRESHOLD_ERROR;
    }
}

void StationaryWavelets3D::hard_threshold(DTYPE beta, int do_thresh_appcoeffs, int normalize)
{
    ON_MY_DEVICE3();
    if (state == W_INVERSE) {
        puts("Warning: StationaryWavelets3D(): cannot threshold coefficients after W.inverse() (run forward() first)");
        return;
    }
    if (state == W_CREATION_ERROR) return;
    const int rc = SFX(pdwt_hard_thresh_swt3d)(d_coeffs, beta, to_pdwt3(winfos), do_thresh_appcoeffs, normalize);
    if (rc != PDWT_OK) {
        report3("StationaryWavelets3D::hard_threshold()", rc);
        state = W_THRESHOLD_ERROR;
    }
}

double StationaryWavelets3D::norm1_double()
{
    ON_MY_DEVICE3();
    if (state == W_CREATION_ERROR) return 0;
    double d = 0;
    const int rc = SFX(pdwt_norm1_swt3d)(d_coeffs, to_pdwt3(winfos), &d);
    if (rc != PDWT_OK) report3("StationaryWavelets3D::norm1()", rc);
    return d;
}
DTYPE StationaryWavelets3D::norm1() { return (DTYPE)norm1_double(); }

int StationaryWavelets3D::get_image(DTYPE* res)
{
    ON_MY_DEVICE3();
    if (!d_image || !res) return 0;
    const size_t n = (size_t)winfos.Nz * winfos.Nr * winfos.Nc;
    if (pdwt_memcpy_d2h(res, d_image, n * sizeof(DTYPE)) != PDWT_OK) return 0;
    return n > (size_t)INT_MAX ? INT_MAX : (int)n;
}

void StationaryWavelets3D::set_image(DTYPE* vol, int mem_is_on_device)
{
    ON_MY_DEVICE3();
    if (!d_image || !vol) return;
    const size_t nb = (size_t)winfos.Nz * winfos.Nr * winfos.Nc * sizeof(DTYPE);
    const int rc = mem_is_on_device ? pdwt_memcpy_d2d_foreign(d_image, vol, nb) : pdwt_memcpy_h2d(d_image, vol, nb);
    if (rc != PDWT_OK) report3("StationaryWavelets3D::set_image()", rc);
    if (state != W_CREATION_ERROR) state = W_INIT;
}

int StationaryWavelets3D::num_bands() const { return state == W_CREATION_ERROR ? 0 : pdwt_num_bands_swt3d(to_pdwt3(winfos)); }

long long StationaryWavelets3D::band_shape(int num, int* bz, int* by, int* bx) const
{
    if (state == W_CREATION_ERROR) return 0;
    const long long n = pdwt_band_size_swt3d(to_pdwt3(winfos), num, bz, by, bx);
    return n > 0 ? n : 0;
}

int StationaryWavelets3D::get_coeff(DTYPE* coeff, int num)
{
    ON_MY_DEVICE3();
    if (state == W_INVERSE) {
        puts("Warning: get_coeff(): inverse() has been performed; run forward() first.");
        return 0;
    }
    if (!d_coeffs || !coeff) return 0;
    const long long n = band_shape(num, NULL, NULL, NULL);
    if (n <= 0) {
        printf("ERROR: get_coeff(): invalid coefficient index %d\n", num);
        return 0;
    }
    if (pdwt_memcpy_d2h(coeff, d_coeffs[num], (size_t)n * sizeof(DTYPE)) != PDWT_OK) return 0;
    return n > (long long)INT_MAX ? INT_MAX : (int)n;
}

void StationaryWavelets3D::set_coeff(DTYPE* coeff, int num, int mem_is_on_device)
{
    ON_MY_DEVICE3();
    if (!d_coeffs || !coeff) return;
    const long long n = band_shape(num, NULL, NULL, NULL);
    if (n <= 0) {
        printf("ERROR: set_coeff(): invalid coefficient index %d\n", num);
        return;
    }
    const size_t nb = (size_t)n * sizeof(DTYPE);
    const int rc = mem_is_on_device ? pdwt_memcpy_d2d_foreign(d_coeffs[num], coeff, nb) : pdwt_memcpy_h2d(d_coeffs[num], coeff, nb);
    if (rc != PDWT_OK) report3("StationaryWavelets3D::set_coeff()", rc);
}

intptr_t StationaryWavelets3D::image_int_ptr(void) { return (intptr_t)d_image; }
intptr_t StationaryWavelets3D::coeff_int_ptr(int num) { return (d_coeffs && band_shape(num, NULL, NULL, NULL) > 0) ? (intptr_t)d_coeffs[num] : 0; }

// ---- band statistics and noise-adaptive thresholds (include/swt3d.h; the shared host half: bandstats_host.hpp) ----
// pointer and size of every band; nb = 0 unless the coefficients are valid
static pdwt_bl::BandList band_list(const StationaryWavelets3D& W)
{
    pdwt_bl::BandList bl;
    bl.nb = 0;
    if (!(W.state == W_FORWARD || W.state == W_THRESHOLD) || !W.d_coeffs) return bl;
    const int nb = W.num_bands();
    if (nb < 2 || nb > pdwt_bl::kMaxBands) return bl;
    for (int k = 0; k < nb; k++) {
        const long long n = W.band_shape(k, NULL, NULL, NULL);
        if (n <= 0 || !W.d_coeffs[k]) return bl;
        bl.ptr[k] = W.d_coeffs[k];
        bl.n[k] = (size_t)n;
    }
    bl.nb = nb;
    bl.finest = 7 * W.winfos.nlevels;  // ddd of level 1
    bl.samples = (double)W.winfos.Nz * W.winfos.Nr * W.winfos.Nc;
    return bl;
}

int StationaryWavelets3D::band_stats(int num, w_band_stats* out, int with_median)
{
    ON_MY_DEVICE3();
    const pdwt_bl::BandList bl = band_list(*this);
    if (!bl.nb || num < 0 || num >= bl.nb || !out) return PDWT_EINVAL;
    const int rc = pdwt_bl::stats(bl, num, out, with_median);
    if (rc != PDWT_OK) report3("StationaryWavelets3D::band_stats()", rc);
    return rc;
}

int StationaryWavelets3D::all_band_stats(w_band_stats* out, int with_median)
{
    ON_MY_DEVICE3();
    const pdwt_bl::BandList bl = band_list(*this);
    if (!bl.nb || !out) return PDWT_EINVAL;
    const int rc = pdwt_bl::stats(bl, -1, out, with_median);
    if (rc != PDWT_OK) report3("StationaryWavelets3D::all_band_stats()", rc);
    return rc;
}

double StationaryWavelets3D::estimate_sigma()
{
    ON_MY_DEVICE3();
    const pdwt_bl::BandList bl = band_list(*this);
    double sigma = -1.0;
    if (!bl.nb) return -1.0;
    const int rc = pdwt_bl::estimate_sigma(bl, &sigma);
    if (rc != PDWT_OK) {
        report3("StationaryWavelets3D::estimate_sigma()", rc);
        return -1.0;
    }
    return sigma;
}

void StationaryWavelets3D::threshold_bands(const DTYPE* betas, int kind)
{
    ON_MY_DEVICE3();
    const pdwt_bl::BandList bl = band_list(*this);
    if (!bl.nb || !betas || (kind != 0 && kind != 1)) return;
    const int rc = pdwt_bl::threshold(bl, betas, kind);
    if (rc != PDWT_OK) {
        report3("StationaryWavelets3D::threshold_bands()", rc);
        state = W_THRESHOLD_ERROR;
    }
}

double StationaryWavelets3D::denoise(int method, double sigma, int kind, DTYPE* betas_out)
{
    ON_MY_DEVICE3();
    const pdwt_bl::BandList bl = band_list(*this);
    if (!bl.nb || (method != 0 && method != 1) || (kind != 0 && kind != 1)) return -1.0;
    DTYPE betas[pdwt_bl::kMaxBands];
    const int rc = pdwt_bl::denoise(bl, method, kind, &sigma, betas);
    if (rc != PDWT_OK) {
        report3("StationaryWavelets3D::denoise()", rc);
        state = W_THRESHOLD_ERROR;
        return -1.0;
    }
    if (betas_out) memcpy(betas_out, betas, (size_t)bl.nb * sizeof(DTYPE));
    return sigma;
}

// ---- flat C handle API (pdwt_amd/swt3d.py) -------------------------------------------------------
#define SW3(h) (static_cast<StationaryWavelets3D*>(h))
extern "C" {
void* pdwt_swt3d_new(DTYPE* vol, int Nz, int Nr, int Nc, const char* wname, int levels, int memisonhost)
{
    return new (std::nothrow) StationaryWavelets3D(vol, Nz, Nr, Nc, wname, levels, memisonhost);
}
void pdwt_swt3d_delete(void* h) { delete SW3(h); }
void pdwt_swt3d_forward(void* h) { SW3(h)->forward(); }
void pdwt_swt3d_inverse(void* h) { SW3(h)->inverse(); }
void pdwt_swt3d_soft_threshold(void* h, DTYPE beta, int app, int normalize) { SW3(h)->soft_threshold(beta, app, normalize); }
void pdwt_swt3d_hard_threshold(void* h, DTYPE beta, int app, int normalize) { SW3(h)->hard_threshold(beta, app, normalize); }
DTYPE pdwt_swt3d_norm1(void* h) { return SW3(h)->norm1(); }
double pdwt_swt3d_norm1_f64(void* h) { return SW3(h)->norm1_double(); }
int pdwt_swt3d_get_image(void* h, DTYPE* out) { return SW3(h)->get_image(out); }
void pdwt_swt3d_set_image(void* h, DTYPE* vol, int mem_is_on_device) { SW3(h)->set_image(vol, mem_is_on_device); }
int pdwt_swt3d_num_bands(void* h) { return SW3(h)->num_bands(); }
long long pdwt_swt3d_band_shape(void* h, int num, int* bz, int* by, int* bx) { return SW3(h)->band_shape(num, bz, by, bx); }
int pdwt_swt3d_get_coeff(void* h, DTYPE* out, int num) { return SW3(h)->get_coeff(out, num); }
void pdwt_swt3d_set_coeff(void* h, DTYPE* in, int num, int mem_is_on_device) { SW3(h)->set_coeff(in, num, mem_is_on_device); }
int pdwt_swt3d_state(void* h) { return (int)SW3(h)->state; }
void pdwt_swt3d_info(void* h, w_info3d* out) { *out = SW3(h)->winfos; }
intptr_t pdwt_swt3d_image_int_ptr(void* h) { return SW3(h)->image_int_ptr(); }
intptr_t pdwt_swt3d_coeff_int_ptr(void* h, int num) { return SW3(h)->coeff_int_ptr(num); }
int pdwt_swt3d_band_stats(void* h, int num, w_band_stats* out, int with_median) { return SW3(h)->band_stats(num, out, with_median); }
int pdwt_swt3d_all_band_stats(void* h, w_band_stats* out, int with_median) { return SW3(h)->all_band_stats(out, with_median); }
double pdwt_swt3d_estimate_sigma(void* h) { return SW3(h)->estimate_sigma(); }
void pdwt_swt3d_threshold_bands(void* h, const DTYPE* betas, int kind) { SW3(h)->threshold_bands(betas, kind); }
double pdwt_swt3d_denoise(void* h, int method, double sigma, int kind, DTYPE* betas_out) { return SW3(h)->denoise(method, sigma, kind, betas_out); }
}
