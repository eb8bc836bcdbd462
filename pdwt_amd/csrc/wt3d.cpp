// wt3d.cpp -- host side of the two volume classes, `Wavelets3D` (include/wt3d.h) and `StationaryWavelets3D` (include/swt3d.h), above
// the 3-D entry points of include/pdwt_hip.h, and their flat C handle APIs (pdwt_wavelets3d_*, pdwt_swt3d_*, the shape of
// wt_capi.cpp).  Every method is written once, on their base `Transform3D`; what differs between the transforms is one `w_ops3d` table
// each.  Plain host C++ like wt.cpp, built into libpdwt.so (float) and libpdwtd.so (-DDOUBLEPRECISION).  The state machine is the one
// of Wavelets (wt.cpp, reference src/wt.cu).
#include <limits.h>
#include <new>
#include <string.h>

#include "../../include/swt3d.h"
#include "bandstats_host.hpp"
#include "host_common.hpp"

static_assert(sizeof(w_info3d) == sizeof(pdwt_info3d), "w_info3d must mirror pdwt_info3d");

// What one transform contributes to the shared class: its name in messages, its entry points of include/pdwt_hip.h in this build's
// precision, and the two texts that differ.  The only place that knows which transform an instance runs.
struct w_ops3d {
    const char* name;
    size_t (*tmp_elems)(pdwt_info3d);
    DTYPE** (*create_coeffs_buffer)(pdwt_info3d);
    int (*free_coeffs_buffer)(DTYPE**, pdwt_info3d);
    int (*forward)(DTYPE*, DTYPE**, DTYPE*, pdwt_info3d, const filters_t*);
    int (*inverse)(DTYPE*, DTYPE**, DTYPE*, pdwt_info3d, const filters_t*);
    int (*soft_thresh)(DTYPE**, DTYPE, pdwt_info3d, int, int);
    int (*hard_thresh)(DTYPE**, DTYPE, pdwt_info3d, int, int);
    int (*norm1)(DTYPE**, pdwt_info3d, double*);
    int (*num_bands)(pdwt_info3d);
    long long (*band_size)(pdwt_info3d, int, int*, int*, int*);
    const char* thresh_after_inverse;     // after the name: the threshold refused in state W_INVERSE
    const char* get_coeff_after_inverse;  // get_coeff() refused in state W_INVERSE
};
static const w_ops3d kDwtOps = {
    "Wavelets3D", pdwt_tmp_elems3d, SFX(pdwt_create_coeffs_buffer3d), SFX(pdwt_free_coeffs_buffer3d), SFX(pdwt_forward3d_separable),
    SFX(pdwt_inverse3d_separable), SFX(pdwt_soft_thresh3d), SFX(pdwt_hard_thresh3d), SFX(pdwt_norm1_3d), pdwt_num_bands3d, pdwt_band_size3d,
    "cannot threshold coefficients, as they were modified by W.inverse()",
    "inverse() has been performed, the coefficients has been modified and do not make sense anymore."};
static const w_ops3d kSwtOps = {
    "StationaryWavelets3D", pdwt_tmp_elems_swt3d, SFX(pdwt_create_coeffs_buffer_swt3d), SFX(pdwt_free_coeffs_buffer_swt3d), SFX(pdwt_forward3d_swt),
    SFX(pdwt_inverse3d_swt), SFX(pdwt_soft_thresh_swt3d), SFX(pdwt_hard_thresh_swt3d), SFX(pdwt_norm1_swt3d), pdwt_num_bands_swt3d, pdwt_band_size_swt3d,
    "cannot threshold coefficients after W.inverse() (run forward() first)", "inverse() has been performed; run forward() first."};

namespace {
struct state3_t {
    filters_t f;
    int dev;  // the device current at construction; every method runs there
};
inline state3_t* S(void* p) { return (state3_t*)p; }
inline pdwt_info3d to_pdwt3(const w_info3d& w)
{
    pdwt_info3d p;
    memcpy(&p, &w, sizeof(p));
    return p;
}
}  // namespace
#define ON_MY_DEVICE3() DevScope dev_scope_(filters_ ? ((const state3_t*)filters_)->dev : -1)

Transform3D::Transform3D(const w_ops3d& ops, DTYPE* vol, int Nz, int Nr, int Nc, const char* wname_, int levels, int memisonhost)
    : d_image(NULL), d_coeffs(NULL), d_tmp(NULL), state(W_INIT), ops_(&ops), filters_(NULL)
{
    winfos.Nz = Nz;
    winfos.Nr = Nr;
    winfos.Nc = Nc;
    winfos.nlevels = levels;
    winfos.hlen = 0;
    strncpy(wname, wname_ ? wname_ : "", 127);
    wname[127] = 0;
    if (Nz < 1 || Nr < 1 || Nc < 1 || !wname_) {
        printf("ERROR: %s(): invalid volume size or wavelet name\n", ops_->name);
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
    const size_t n = (size_t)Nz * Nr * Nc, ntmp = ops_->tmp_elems(w);
    if (ntmp == 0) {
        printf("ERROR: %s(): unsupported volume size (Nz <= 65535 and Nr * Nc < 2^31 are required)\n", ops_->name);
        state = W_CREATION_ERROR;
        return;
    }
    d_image = (DTYPE*)pdwt_malloc(n * sizeof(DTYPE));
    d_tmp = (DTYPE*)pdwt_malloc(ntmp * sizeof(DTYPE));
    d_coeffs = ops_->create_coeffs_buffer(w);
    if (!d_image || !d_tmp || !d_coeffs) {
        printf("ERROR: %s(): device allocation failed: %s\n", ops_->name, pdwt_last_error_string());
        state = W_CREATION_ERROR;
        return;
    }
    int rc;
    if (!vol) rc = pdwt_memset(d_image, 0, n * sizeof(DTYPE));
    else if (memisonhost) rc = pdwt_memcpy_h2d(d_image, vol, n * sizeof(DTYPE));
    else rc = pdwt_memcpy_d2d_foreign(d_image, vol, n * sizeof(DTYPE));
    if (rc != PDWT_OK) {
        report(ops_->name, "(): volume upload", rc);
        state = W_CREATION_ERROR;
    }
}

Transform3D::~Transform3D()
{
    ON_MY_DEVICE3();
    if (d_image) pdwt_free(d_image);
    if (d_coeffs) ops_->free_coeffs_buffer(d_coeffs, to_pdwt3(winfos));
    if (d_tmp) pdwt_free(d_tmp);
    free(filters_);
}

void Transform3D::forward()
{
    ON_MY_DEVICE3();
    if (state == W_CREATION_ERROR) {
        puts("Warning: forward transform not computed, as there was an error when creating the wavelets");
        return;
    }
    const int rc = ops_->forward(d_image, d_coeffs, d_tmp, to_pdwt3(winfos), &S(filters_)->f);
    if (rc != PDWT_OK) {
        report(ops_->name, "::forward()", rc);
        state = W_FORWARD_ERROR;
        return;
    }
    state = W_FORWARD;
}

void Transform3D::inverse()
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
    const int rc = ops_->inverse(d_image, d_coeffs, d_tmp, to_pdwt3(winfos), &S(filters_)->f);
    if (rc != PDWT_OK) {
        report(ops_->name, "::inverse()", rc);
        state = W_INVERSE_ERROR;
        return;
    }
    state = W_INVERSE;
}

void Transform3D::soft_threshold(DTYPE beta, int do_thresh_appcoeffs, int normalize)
{
    ON_MY_DEVICE3();
    if (state == W_INVERSE) {
        printf("Warning: %s(): %s\n", ops_->name, ops_->thresh_after_inverse);
        return;
    }
    if (state == W_CREATION_ERROR) return;
    const int rc = ops_->soft_thresh(d_coeffs, beta, to_pdwt3(winfos), do_thresh_appcoeffs, normalize);
    if (rc != PDWT_OK) {
        report(ops_->name, "::soft_threshold()", rc);
        state = W_THRESHOLD_ERROR;
    }
}

void Transform3D::hard_threshold(DTYPE beta, int do_thresh_appcoeffs, int normalize)
{
    ON_MY_DEVICE3();
    if (state == W_INVERSE) {
        printf("Warning: %s(): %s\n", ops_->name, ops_->thresh_after_inverse);
        return;
    }
    if (state == W_CREATION_ERROR) return;
    const int rc = ops_->hard_thresh(d_coeffs, beta, to_pdwt3(winfos), do_thresh_appcoeffs, normalize);
    if (rc != PDWT_OK) {
        report(ops_->name, "::hard_threshold()", rc);
        state = W_THRESHOLD_ERROR;
    }
}

double Transform3D::norm1_double()
{
    ON_MY_DEVICE3();
    if (state == W_CREATION_ERROR) return 0;
    double d = 0;
    const int rc = ops_->norm1(d_coeffs, to_pdwt3(winfos), &d);
    if (rc != PDWT_OK) report(ops_->name, "::norm1()", rc);
    return d;
}
DTYPE Transform3D::norm1() { return (DTYPE)norm1_double(); }

int Transform3D::get_image(DTYPE* res)
{
    ON_MY_DEVICE3();
    if (!d_image || !res) return 0;
    const size_t n = (size_t)winfos.Nz * winfos.Nr * winfos.Nc;
    if (pdwt_memcpy_d2h(res, d_image, n * sizeof(DTYPE)) != PDWT_OK) return 0;
    return n > (size_t)INT_MAX ? INT_MAX : (int)n;
}

void Transform3D::set_image(DTYPE* vol, int mem_is_on_device)
{
    ON_MY_DEVICE3();
    if (!d_image || !vol) return;
    const size_t nb = (size_t)winfos.Nz * winfos.Nr * winfos.Nc * sizeof(DTYPE);
    const int rc = mem_is_on_device ? pdwt_memcpy_d2d_foreign(d_image, vol, nb) : pdwt_memcpy_h2d(d_image, vol, nb);
    if (rc != PDWT_OK) report(ops_->name, "::set_image()", rc);
    if (state != W_CREATION_ERROR) state = W_INIT;
}

int Transform3D::num_bands() const { return state == W_CREATION_ERROR ? 0 : ops_->num_bands(to_pdwt3(winfos)); }

long long Transform3D::band_shape(int num, int* bz, int* by, int* bx) const
{
    if (state == W_CREATION_ERROR) return 0;
    const long long n = ops_->band_size(to_pdwt3(winfos), num, bz, by, bx);
    return n > 0 ? n : 0;
}

int Transform3D::get_coeff(DTYPE* coeff, int num)
{
    ON_MY_DEVICE3();
    if (state == W_INVERSE) {
        printf("Warning: get_coeff(): %s\n", ops_->get_coeff_after_inverse);
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

void Transform3D::set_coeff(DTYPE* coeff, int num, int mem_is_on_device)
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
    if (rc != PDWT_OK) report(ops_->name, "::set_coeff()", rc);
}

intptr_t Transform3D::image_int_ptr(void) { return (intptr_t)d_image; }
intptr_t Transform3D::coeff_int_ptr(int num) { return (d_coeffs && band_shape(num, NULL, NULL, NULL) > 0) ? (intptr_t)d_coeffs[num] : 0; }

// ---- band statistics and noise-adaptive thresholds (include/wt3d.h; the host half shared with Wavelets: bandstats_host.hpp) ----
// pointer and size of every band; nb = 0 unless the coefficients are valid
static pdwt_bl::BandList band_list(const Transform3D& W)
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

int Transform3D::band_stats(int num, w_band_stats* out, int with_median)
{
    ON_MY_DEVICE3();
    const pdwt_bl::BandList bl = band_list(*this);
    if (!bl.nb || num < 0 || num >= bl.nb || !out) return PDWT_EINVAL;
    const int rc = pdwt_bl::stats(bl, num, out, with_median);
    if (rc != PDWT_OK) report(ops_->name, "::band_stats()", rc);
    return rc;
}

int Transform3D::all_band_stats(w_band_stats* out, int with_median)
{
    ON_MY_DEVICE3();
    const pdwt_bl::BandList bl = band_list(*this);
    if (!bl.nb || !out) return PDWT_EINVAL;
    const int rc = pdwt_bl::stats(bl, -1, out, with_median);
    if (rc != PDWT_OK) report(ops_->name, "::all_band_stats()", rc);
    return rc;
}

double Transform3D::estimate_sigma()
{
    ON_MY_DEVICE3();
    const pdwt_bl::BandList bl = band_list(*this);
    double sigma = -1.0;
    if (!bl.nb) return -1.0;
    const int rc = pdwt_bl::estimate_sigma(bl, &sigma);
    if (rc != PDWT_OK) {
        report(ops_->name, "::estimate_sigma()", rc);
        return -1.0;
    }
    return sigma;
}

void Transform3D::threshold_bands(const DTYPE* betas, int kind)
{
    ON_MY_DEVICE3();
    const pdwt_bl::BandList bl = band_list(*this);
    if (!bl.nb || !betas || (kind != 0 && kind != 1)) return;
    const int rc = pdwt_bl::threshold(bl, betas, kind);
    if (rc != PDWT_OK) {
        report(ops_->name, "::threshold_bands()", rc);
        state = W_THRESHOLD_ERROR;
    }
}

double Transform3D::denoise(int method, double sigma, int kind, DTYPE* betas_out)
{
    ON_MY_DEVICE3();
    const pdwt_bl::BandList bl = band_list(*this);
    if (!bl.nb || (method != 0 && method != 1) || (kind != 0 && kind != 1)) return -1.0;
    DTYPE betas[pdwt_bl::kMaxBands];
    const int rc = pdwt_bl::denoise(bl, method, kind, &sigma, betas);
    if (rc != PDWT_OK) {
        report(ops_->name, "::denoise()", rc);
        state = W_THRESHOLD_ERROR;
        return -1.0;
    }
    if (betas_out) memcpy(betas_out, betas, (size_t)bl.nb * sizeof(DTYPE));
    return sigma;
}

// ---- the two classes: a constructor each, which names the table ----------------------------------------
Wavelets3D::Wavelets3D(DTYPE* vol, int Nz, int Nr, int Nc, const char* wname_, int levels, int memisonhost)
    : Transform3D(kDwtOps, vol, Nz, Nr, Nc, wname_, levels, memisonhost)
{
}
StationaryWavelets3D::StationaryWavelets3D(DTYPE* vol, int Nz, int Nr, int Nc, const char* wname_, int levels, int memisonhost)
    : Transform3D(kSwtOps, vol, Nz, Nr, Nc, wname_, levels, memisonhost)
{
}

// ---- flat C handle APIs (pdwt_amd/wavelets3d.py, pdwt_amd/swt3d.py): one list, stamped out per class -------------------
// new and delete go through the concrete class (the destructor of Transform3D is not virtual)
#define PDWT_HANDLE_API3(P, CLS) \
    void* P##new(DTYPE* vol, int Nz, int Nr, int Nc, const char* wname, int levels, int memisonhost) { return new (std::nothrow) CLS(vol, Nz, Nr, Nc, wname, levels, memisonhost); } \
    void P##delete(void* h) { delete static_cast<CLS*>(h); } \
    void P##forward(void* h) { static_cast<CLS*>(h)->forward(); } \
    void P##inverse(void* h) { static_cast<CLS*>(h)->inverse(); } \
    void P##soft_threshold(void* h, DTYPE beta, int app, int normalize) { static_cast<CLS*>(h)->soft_threshold(beta, app, normalize); } \
    void P##hard_threshold(void* h, DTYPE beta, int app, int normalize) { static_cast<CLS*>(h)->hard_threshold(beta, app, normalize); } \
    DTYPE P##norm1(void* h) { return static_cast<CLS*>(h)->norm1(); } \
    double P##norm1_f64(void* h) { return static_cast<CLS*>(h)->norm1_double(); } \
    int P##get_image(void* h, DTYPE* out) { return static_cast<CLS*>(h)->get_image(out); } \
    void P##set_image(void* h, DTYPE* vol, int mem_is_on_device) { static_cast<CLS*>(h)->set_image(vol, mem_is_on_device); } \
    int P##num_bands(void* h) { return static_cast<CLS*>(h)->num_bands(); } \
    long long P##band_shape(void* h, int num, int* bz, int* by, int* bx) { return static_cast<CLS*>(h)->band_shape(num, bz, by, bx); } \
    int P##get_coeff(void* h, DTYPE* out, int num) { return static_cast<CLS*>(h)->get_coeff(out, num); } \
    void P##set_coeff(void* h, DTYPE* in, int num, int mem_is_on_device) { static_cast<CLS*>(h)->set_coeff(in, num, mem_is_on_device); } \
    int P##state(void* h) { return (int)static_cast<CLS*>(h)->state; } \
    void P##info(void* h, w_info3d* out) { *out = static_cast<CLS*>(h)->winfos; } \
    intptr_t P##image_int_ptr(void* h) { return static_cast<CLS*>(h)->image_int_ptr(); } \
    intptr_t P##coeff_int_ptr(void* h, int num) { return static_cast<CLS*>(h)->coeff_int_ptr(num); } \
    int P##band_stats(void* h, int num, w_band_stats* out, int with_median) { return static_cast<CLS*>(h)->band_stats(num, out, with_median); } \
    int P##all_band_stats(void* h, w_band_stats* out, int with_median) { return static_cast<CLS*>(h)->all_band_stats(out, with_median); } \
    double P##estimate_sigma(void* h) { return static_cast<CLS*>(h)->estimate_sigma(); } \
    void P##threshold_bands(void* h, const DTYPE* betas, int kind) { static_cast<CLS*>(h)->threshold_bands(betas, kind); } \
    double P##denoise(void* h, int method, double sigma, int kind, DTYPE* betas_out) { return static_cast<CLS*>(h)->denoise(method, sigma, kind, betas_out); }
extern "C" {
PDWT_HANDLE_API3(pdwt_wavelets3d_, Wavelets3D)
PDWT_HANDLE_API3(pdwt_swt3d_, StationaryWavelets3D)
}
#undef PDWT_HANDLE_API3
