// wt3d.cpp -- host side of `Wavelets3D` (include/wt3d.h) above the 3-D entry points of include/pdwt_hip.h, and its flat C
// handle API (pdwt_wavelets3d_*, the shape of wt_capi.cpp).  Plain host C++ like wt.cpp, built into libpdwt.so (float) and
// libpdwtd.so (-DDOUBLEPRECISION).  The state machine is the one of Wavelets (wt.cpp, reference src/wt.cu).
#include <limits.h>
#include <new>
#include <string.h>

#include "../../include/pdwt_hip.h"
#include "../../include/wt3d.h"
#include "bandstats_host.hpp"

static_assert(sizeof(w_info3d) == sizeof(pdwt_info3d), "w_info3d must mirror pdwt_info3d");

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

Wavelets3D::Wavelets3D(DTYPE* vol, int Nz, int Nr, int Nc, const char* wname_, int levels, int memisonhost)
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
        puts("ERROR: Wavelets3D(): invalid volume size or wavelet name");
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
    const size_t n = (size_t)Nz * Nr * Nc, ntmp = pdwt_tmp_elems3d(w);
    if (ntmp == 0) {
        puts("ERROR: Wavelets3D(): unsupported volume size (Nz <= 65535 and Nr * Nc < 2^31 are required)");
        state = W_CREATION_ERROR;
        return;
    }
    d_image = (DTYPE*)pdwt_malloc(n * sizeof(DTYPE));
    d_tmp = (DTYPE*)pdwt_malloc(ntmp * sizeof(DTYPE));
    d_coeffs = SFX(pdwt_create_coeffs_buffer3d)(w);
    if (!d_image || !d_tmp || !d_coeffs) {
        printf("ERROR: Wavelets3D(): device allocation failed: %s\n", pdwt_last_error_string());
        state = W_CREATION_ERROR;
        return;
    }
    int rc;
    if (!vol) rc = pdwt_memset(d_image, 0, n * sizeof(DTYPE));
    else if (memisonhost) rc = pdwt_memcpy_h2d(d_image, vol, n * sizeof(DTYPE));
    else rc = pdwt_memcpy_d2d_foreign(d_image, vol, n * sizeof(DTYPE));
    if (rc != PDWT_OK) {
        report3("Wavelets3D(): volume upload", rc);
        state = W_CREATION_ERROR;
    }
}

Wavelets3D::~Wavelets3D()
{
    ON_MY_DEVICE3();
    if (d_image) pdwt_free(d_image);
    if (d_coeffs) SFX(pdwt_free_coeffs_buffer3d)(d_coeffs, to_pdwt3(winfos));
    if (d_tmp) pdwt_free(d_tmp);
    free(filters_);
}

void Wavelets3D::forward()
{
    ON_MY_DEVICE3();
    if (state == W_CREATION_ERROR) {
        puts("Warning: forward transform not computed, as there was an error when creating the wavelets");
        return;
    }
    const int rc = SFX(pdwt_forward3d_separable)(d_image, d_coeffs, d_tmp, to_pdwt3(winfos), &S(filters_)->f);
    if (rc != PDWT_OK) {
        report3("Wavelets3D::forward()", rc);
        state = W_FORWARD_ERROR;
        return;
    }
    state = W_FORWARD;
}

void Wavelets3D::inverse()
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
    const int rc = SFX(pdwt_inverse3d_separable)(d_image, d_coeffs, d_tmp, to_pdwt3(winfos), &S(filters_)->f);
    if (rc != PDWT_OK) {
        report3("Wavelets3D::inverse()", rc);
        state = W_INVERSE_ERROR;
        return;
    }
    state = W_INVERSE;
}

void Wavelets3D::soft_threshold(DTYPE beta, int do_thresh_appcoeffs, int normalize)
{
    ON_MY_DEVICE3();
    if (state == W_INVERSE) {
        puts("Warning: Wavelets3D(): cannot threshold coefficients, as they were modified by W.inverse()");
        return;
    }
    if (state == W_CREATION_ERROR) return;
    const int rc = SFX(pdwt_soft_thresh3d)(d_coeffs, beta, to_pdwt3(winfos), do_thresh_appcoeffs, normalize);
    if (rc != PDWT_OK) {
        report3("Wavelets3D::soft_threshold()", rc);
        state = W_THRESHOLD_ERROR;
    }
}

void Wavelets3D::hard_threshold(DTYPE beta, int do_thresh_appcoeffs, int normalize)
{
    ON_MY_DEVICE3();
    if (state == W_INVERSE) {
        puts("Warning: Wavelets3D(): cannot threshold coefficients, as they were modified by W.inverse()");
        return;
    }
    if (state == W_CREATION_ERROR) return;
    const int rc = SFX(pdwt_hard_thresh3d)(d_coeffs, beta, to_pdwt3(winfos), do_thresh_appcoeffs, normalize);
    if (rc != PDWT_OK) {
        report3("Wavelets3D::hard_threshold()", rc);
        state = W_THRESHOLD_ERROR;
    }
}

double Wavelets3D::norm1_double()
{
    ON_MY_DEVICE3();
    if (state == W_CREATION_ERROR) return 0;
    double d = 0;
    const int rc = SFX(pdwt_norm1_3d)(d_coeffs, to_pdwt3(winfos), &d);
    if (rc != PDWT_OK) report3("Wavelets3D::norm1()", rc);
    return d;
}
DTYPE Wavelets3D::norm1() { return (DTYPE)norm1_double(); }

int Wavelets3D::get_image(DTYPE* res)
{
    ON_MY_DEVICE3();
    if (!d_image || !res) return 0;
    const size_t n = (size_t)winfos.Nz * winfos.Nr * winfos.Nc;
    if (pdwt_memcpy_d2h(res, d_image, n * sizeof(DTYPE)) != PDWT_OK) return 0;
    return n > (size_t)INT_MAX ? INT_MAX : (int)n;
}

void Wavelets3D::set_image(DTYPE* vol, int mem_is_on_device)
{
    ON_MY_DEVICE3();
    if (!d_image || !vol) return;
    const size_t nb = (size_t)winfos.Nz * winfos.Nr * winfos.Nc * sizeof(DTYPE);
    const int rc = mem_is_on_device ? pdwt_memcpy_d2d_foreign(d_image, vol, nb) : pdwt_memcpy_h2d(d_image, vol, nb);
    if (rc != PDWT_OK) report3("Wavelets3D::set_image()", rc);
    if (state != W_CREATION_ERROR) state = W_INIT;
}

int Wavelets3D::num_bands() const { return state == W_CREATION_ERROR ? 0 : pdwt_num_bands3d(to_pdwt3(winfos)); }

long long Wavelets3D::band_shape(int num, int* bz, int* by, int* bx) const
{
    if (state == W_CREATION_ERROR) return 0;
    const long long n = pdwt_band_size3d(to_pdwt3(winfos), num, bz, by, bx);
    return n > 0 ? n : 0;
}

int Wavelets3D::get_coeff(DTYPE* coeff, int num)
{
    ON_MY_DEVICE3();
    if (state == W_INVERSE) {
        puts("Warning: get_coeff(): inverse() has been performed, the coefficients has been modified and do not make sense anymore.");
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

void Wavelets3D::set_coeff(DTYPE* coeff, int num, int mem_is_on_device)
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
    if (rc != PDWT_OK) report3("Wavelets3D::set_coeff()", rc);
}

intptr_t Wavelets3D::image_int_ptr(void) { return (intptr_t)d_image; }
intptr_t Wavelets3D::coeff_int_ptr(int num) { return (d_coeffs && band_shape(num, NULL, NULL, NULL) > 0) ? (intptr_t)d_coeffs[num] : 0; }

// ---- band statistics and noise-adaptive thresholds (include/wt3d.h; the shared host half: bandstats_host.hpp) ----
// pointer and size of every band; nb = 0 unless the coefficients are valid
static pdwt_bl::BandList band_list(const Wavelets3D& W)
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

int Wavelets3D::band_stats(int num, w_band_stats* out, int with_median)
{
    ON_MY_DEVICE3();
    const pdwt_bl::BandList bl = band_list(*this);
    if (!bl.nb || num < 0 || num >= bl.nb || !out) return PDWT_EINVAL;
    const int rc = pdwt_bl::stats(bl, num, out, with_median);
    if (rc != PDWT_OK) report3("Wavelets3D::band_stats()", rc);
    return rc;
}

int Wavelets3D::all_band_stats(w_band_stats* out, int with_median)
{
    ON_MY_DEVICE3();
    const pdwt_bl::BandList bl = band_list(*this);
    if (!bl.nb || !out) return PDWT_EINVAL;
    const int rc = pdwt_bl::stats(bl, -1, out, with_median);
    if (rc != PDWT_OK) report3("Wavelets3D::all_band_stats()", rc);
    return rc;
}

double Wavelets3D::estimate_sigma()
{
    ON_MY_DEVICE3();
    const pdwt_bl::BandList bl = band_list(*this);
    double sigma = -1.0;
    if (!bl.nb) return -1.0;
    const int rc = pdwt_bl::estimate_sigma(bl, &sigma);
    if (rc != PDWT_OK) {
        report3("Wavelets3D::estimate_sigma()", rc);
        return -1.0;
    }
    return sigma;
}

void Wavelets3D::threshold_bands(const DTYPE* betas, int kind)
{
    ON_MY_DEVICE3();
    const pdwt_bl::BandList bl = band_list(*this);
    if (!bl.nb || !betas || (kind != 0 && kind != 1)) return;
    const int rc = pdwt_bl::threshold(bl, betas, kind);
    if (rc != PDWT_OK) {
        report3("Wavelets3D::threshold_bands()", rc);
        state = W_THRESHOLD_ERROR;
    }
}

double Wavelets3D::denoise(int method, double sigma, int kind, DTYPE* betas_out)
{
    ON_MY_DEVICE3();
    const pdwt_bl::BandList bl = band_list(*this);
    if (!bl.nb || (method != 0 && method != 1) || (kind != 0 && kind != 1)) return -1.0;
    DTYPE betas[pdwt_bl::kMaxBands];
    const int rc = pdwt_bl::denoise(bl, method, kind, &sigma, betas);
    if (rc != PDWT_OK) {
        report3("Wavelets3D::denoise()", rc);
        state = W_THRESHOLD_ERROR;
        return -1.0;
    }
    if (betas_out) memcpy(betas_out, betas, (size_t)bl.nb * sizeof(DTYPE));
    return sigma;
}

// ---- flat C handle API (pdwt_amd/wavelets3d.py) -------------------------------------------------------
#define W3(h) (static_cast<Wavelets3D*>(h))
extern "C" {
void* pdwt_wavelets3d_new(DTYPE* vol, int Nz, int Nr, int Nc, const char* wname, int levels, int memisonhost)
{
    return new (std::nothrow) Wavelets3D(vol, Nz, Nr, Nc, wname, levels, memisonhost);
}
void pdwt_wavelets3d_delete(void* h) { delete W3(h); }
void pdwt_wavelets3d_forward(void* h) { W3(h)->forward(); }
void pdwt_wavelets3d_inverse(void* h) { W3(h)->inverse(); }
void pdwt_wavelets3d_soft_threshold(void* h, DTYPE beta, int app, int normalize) { W3(h)->soft_threshold(beta, app, normalize); }
void pdwt_wavelets3d_hard_threshold(void* h, DTYPE beta, int app, int normalize) { W3(h)->hard_threshold(beta, app, normalize); }
DTYPE pdwt_wavelets3d_norm1(void* h) { return W3(h)->norm1(); }
double pdwt_wavelets3d_norm1_f64(void* h) { return W3(h)->norm1_double(); }
int pdwt_wavelets3d_get_image(void* h, DTYPE* out) { return W3(h)->get_image(out); }
void pdwt_wavelets3d_set_image(void* h, DTYPE* vol, int mem_is_on_device) { W3(h)->set_image(vol, mem_is_on_device); }
int pdwt_wavelets3d_num_bands(void* h) { return W3(h)->num_bands(); }
long long pdwt_wavelets3d_band_shape(void* h, int num, int* bz, int* by, int* bx) { return W3(h)->band_shape(num, bz, by, bx); }
int pdwt_wavelets3d_get_coeff(void* h, DTYPE* out, int num) { return W3(h)->get_coeff(out, num); }
void pdwt_wavelets3d_set_coeff(void* h, DTYPE* in, int num, int mem_is_on_device) { W3(h)->set_coeff(in, num, mem_is_on_device); }
int pdwt_wavelets3d_state(void* h) { return (int)W3(h)->state; }
void pdwt_wavelets3d_info(void* h, w_info3d* out) { *out = W3(h)->winfos; }
intptr_t pdwt_wavelets3d_image_int_ptr(void* h) { return W3(h)->image_int_ptr(); }
intptr_t pdwt_wavelets3d_coeff_int_ptr(void* h, int num) { return W3(h)->coeff_int_ptr(num); }
int pdwt_wavelets3d_band_stats(void* h, int num, w_band_stats* out, int with_median) { return W3(h)->band_stats(num, out, with_median); }
int pdwt_wavelets3d_all_band_stats(void* h, w_band_stats* out, int with_median) { return W3(h)->all_band_stats(out, with_median); }
double pdwt_wavelets3d_estimate_sigma(void* h) { return W3(h)->estimate_sigma(); }
void pdwt_wavelets3d_threshold_bands(void* h, const DTYPE* betas, int kind) { W3(h)->threshold_bands(betas, kind); }
double pdwt_wavelets3d_denoise(void* h, int method, double sigma, int kind, DTYPE* betas_out) { return W3(h)->denoise(method, sigma, kind, betas_out); }
}
