// bandstats_host.hpp -- the host half of band_stats / all_band_stats / estimate_sigma / threshold_bands / denoise, shared by
// Wavelets and WaveletsImages (wt.cpp), Wavelets3D (wt3d.cpp) and StationaryWavelets3D (swt3d.cpp): each class checks its state and builds its
// band list (pointer and logical size per band, the finest diagonal band, the samples of one signal); everything else is here.
// Plain host C++ above the C-ABI (include/pdwt_hip.h: the bandlist stats / thresh entries), DTYPE as in wt.h.
#pragma once
#include <math.h>
#include <stddef.h>

#include "../../include/pdwt_hip.h"
#include "../../include/wt.h"

static_assert(sizeof(w_band_stats) == sizeof(pdwt_band_stats), "w_band_stats must mirror pdwt_band_stats");

namespace pdwt_bl {

#ifndef DOUBLEPRECISION
#define PDWT_BL_SFX(name) name##_f32
#else
#define PDWT_BL_SFX(name) name##_f64
#endif

constexpr int kMaxBands = 3 * 32 + 1;
// median |N(0, 1)|: sigma = median |finest diagonal band| / kMadScale
constexpr double kMadScale = 0.6744897501960817;

struct BandList {
    DTYPE* ptr[kMaxBands];
    size_t n[kMaxBands];
    int nb;          // 0: the list could not be built
    int finest;      // the finest diagonal band (D1 / ddd of level 1)
    double samples;  // N of the universal threshold: samples of one transformed signal
};

// statistics of band `num`, or of every band (num < 0: out has nb entries); 0 on success
inline int stats(const BandList& bl, int num, w_band_stats* out, int with_median)
{
    if (!out || bl.nb < 1 || num >= bl.nb) return PDWT_EINVAL;
    unsigned char want[kMaxBands];
    for (int k = 0; k < bl.nb; k++) want[k] = with_median ? 1 : 0;
    pdwt_band_stats* o = reinterpret_cast<pdwt_band_stats*>(out);
    if (num >= 0) return PDWT_BL_SFX(pdwt_bandlist_stats)(bl.ptr + num, bl.n + num, 1, want, o);
    return PDWT_BL_SFX(pdwt_bandlist_stats)(bl.ptr, bl.n, bl.nb, want, o);
}

inline int estimate_sigma(const BandList& bl, double* sigma)
{
    // the select passes alone (want_median = 2): the moments of the band are not needed
    const unsigned char want = 2;
    pdwt_band_stats s;
    const int rc = PDWT_BL_SFX(pdwt_bandlist_stats)(bl.ptr + bl.finest, bl.n + bl.finest, 1, &want, &s);
    if (rc == PDWT_OK) *sigma = s.median_abs / kMadScale;
    return rc;
}

// kind: 0 soft, 1 hard; betas[k] < 0 leaves band k alone
inline int threshold(const BandList& bl, const DTYPE* betas, int kind)
{
    if (!betas || bl.nb < 1) return PDWT_EINVAL;
    return PDWT_BL_SFX(pdwt_bandlist_thresh)(kind, bl.ptr, bl.n, betas, bl.nb);
}

// The beta of every band in double (band 0 = -1: never touched) from sigma and, for BayesShrink, the statistics of the bands: THE rule
// of denoise(), single image and batch.  method 0 VisuShrink: sigma * sqrt(2 ln samples) on every detail band (s is not read);
// method 1 BayesShrink: sigma^2 / sqrt(ms_b - sigma^2), ms_b = sum c^2 / n, or max |c| when ms_b <= sigma^2.
inline void band_betas(int method, double sigma, double samples, const pdwt_band_stats* s, int nb, double* beta)
{
    beta[0] = -1.0;
    if (method == 0) {
        const double t = sigma * sqrt(2.0 * log(samples));
        for (int k = 1; k < nb; k++) beta[k] = t;
    } else {
        const double s2 = sigma * sigma;
        for (int k = 1; k < nb; k++) {
            const double ms = s[k].n > 0 ? s[k].sum_sq / s[k].n : 0.0;
            beta[k] = ms > s2 ? s2 / sqrt(ms - s2) : s[k].max_abs;  // no signal above the noise: the band goes to zero
        }
    }
}

// method 0 VisuShrink, 1 BayesShrink (include/wt.h); *sigma < 0 on entry: estimated.  The betas (one rounding to DTYPE) go to `betas`
// (nb entries, band 0 = -1) and are applied.
inline int denoise(const BandList& bl, int method, int kind, double* sigma, DTYPE* betas)
{
    if (bl.nb < 2 || (method != 0 && method != 1) || (kind != 0 && kind != 1)) return PDWT_EINVAL;
    const bool estimate = *sigma < 0;
    double beta[kMaxBands];
    pdwt_band_stats s[kMaxBands];
    if (method == 0) {
        if (estimate) {
            if (const int rc = estimate_sigma(bl, sigma); rc != PDWT_OK) return rc;
        }
    } else {
        // one moments launch over all bands; the median of the finest diagonal band rides along when sigma is to be estimated
        unsigned char want[kMaxBands] = {};
        want[bl.finest] = estimate ? 1 : 0;
        if (const int rc = PDWT_BL_SFX(pdwt_bandlist_stats)(bl.ptr, bl.n, bl.nb, want, s); rc != PDWT_OK) return rc;
        if (estimate) *sigma = s[bl.finest].median_abs / kMadScale;
    }
    band_betas(method, *sigma, bl.samples, s, bl.nb, beta);
    for (int k = 0; k < bl.nb; k++) betas[k] = (DTYPE)beta[k];
    return threshold(bl, betas, kind);
}

// ---- a regular batch (WaveletsImages, include/wt_batch.h): B images with the band geometry of `g` (its ptr[] is not used), the
// B * nb band pointers in a table in device memory (band k of image b at d_tab[b * nb + k]); kernels: bandbatch.hip.  Every
// call is a fixed number of launches and one copy to the host, whatever B (pdwt_bandbatch_*, include/pdwt_hip.h).
inline int batch_stats(const BandList& g, DTYPE* const* d_tab, int B, w_band_stats* out, int with_median)
{
    if (!out || !d_tab || g.nb < 1 || B < 1) return PDWT_EINVAL;
    unsigned char want[kMaxBands];
    for (int k = 0; k < g.nb; k++) want[k] = with_median ? 1 : 0;
    return PDWT_BL_SFX(pdwt_bandbatch_stats)(d_tab, g.n, B, g.nb, want, reinterpret_cast<pdwt_band_stats*>(out));
}

// s: B * nb entries of scratch for the caller's statistics
inline int batch_estimate_sigma(const BandList& g, DTYPE* const* d_tab, int B, pdwt_band_stats* s, double* sigma)
{
    if (!sigma || !s || !d_tab || g.nb < 1 || B < 1) return PDWT_EINVAL;
    // the selection alone, on the finest diagonal band of every image: the other bands ask for nothing
    unsigned char want[kMaxBands] = {};
    size_t n[kMaxBands] = {};
    n[g.finest] = g.n[g.finest];  // (a band of 0 elements is left out of every launch)
    want[g.finest] = 2;
    const int rc = PDWT_BL_SFX(pdwt_bandbatch_stats)(d_tab, n, B, g.nb, want, s);
    if (rc != PDWT_OK) return rc;
    for (int b = 0; b < B; b++) sigma[b] = s[(size_t)b * g.nb + g.finest].median_abs / kMadScale;
    return PDWT_OK;
}

// betas: B * nb; beta < 0 leaves that band of that image alone
inline int batch_threshold(const BandList& g, DTYPE* const* d_tab, int B, const DTYPE* betas, int kind)
{
    if (!betas || !d_tab || g.nb < 1 || B < 1) return PDWT_EINVAL;
    return PDWT_BL_SFX(pdwt_bandbatch_thresh)(kind, d_tab, g.n, betas, B, g.nb);
}

// denoise() of every image with ITS OWN sigma: sigma_in NULL or sigma_in[b] < 0 = estimated from image b.  sigma_out: B values;
// betas: B * nb (one rounding to DTYPE, band 0 = -1), applied.  s: B * nb entries of scratch.
inline int batch_denoise(const BandList& g, DTYPE* const* d_tab, int B, int method, int kind, const double* sigma_in, pdwt_band_stats* s,
                         double* sigma_out, DTYPE* betas)
{
    if (g.nb < 2 || B < 1 || !d_tab || !s || !sigma_out || !betas || (method != 0 && method != 1) || (kind != 0 && kind != 1)) return PDWT_EINVAL;
    bool estimate = !sigma_in;
    for (int b = 0; b < B && !estimate; b++) estimate = sigma_in[b] < 0;
    if (method == 0) {
        if (estimate) {
            if (const int rc = batch_estimate_sigma(g, d_tab, B, s, sigma_out); rc != PDWT_OK) return rc;
        }
    } else {
        // one moments launch over all bands of all images; the medians of the finest diagonal bands ride along when a sigma is to be estimated
        unsigned char want[kMaxBands] = {};
        want[g.finest] = estimate ? 1 : 0;
        if (const int rc = PDWT_BL_SFX(pdwt_bandbatch_stats)(d_tab, g.n, B, g.nb, want, s); rc != PDWT_OK) return rc;
        if (estimate)
            for (int b = 0; b < B; b++) sigma_out[b] = s[(size_t)b * g.nb + g.finest].median_abs / kMadScale;
    }
    double beta[kMaxBands];
    for (int b = 0; b < B; b++) {
        if (sigma_in && !(sigma_in[b] < 0)) sigma_out[b] = sigma_in[b];
        band_betas(method, sigma_out[b], g.samples, s + (size_t)b * g.nb, g.nb, beta);
        for (int k = 0; k < g.nb; k++) betas[(size_t)b * g.nb + k] = (DTYPE)beta[k];
    }
    return batch_threshold(g, d_tab, B, betas, kind);
}

}  // namespace pdwt_bl
