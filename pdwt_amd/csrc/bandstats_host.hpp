// bandstats_host.hpp -- the host half of band_stats / all_band_stats / estimate_sigma / threshold_bands / denoise, shared by
// Wavelets (wt.cpp), Wavelets3D (wt3d.cpp) and StationaryWavelets3D (swt3d.cpp): each class checks its state and builds its
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

// method 0 VisuShrink, 1 BayesShrink (include/wt.h); *sigma < 0 on entry: estimated.  The betas (one rounding to DTYPE) go to `betas`
// (nb entries, band 0 = -1) and are applied.
inline int denoise(const BandList& bl, int method, int kind, double* sigma, DTYPE* betas)
{
    if (bl.nb < 2 || (method != 0 && method != 1) || (kind != 0 && kind != 1)) return PDWT_EINVAL;
    const bool estimate = *sigma < 0;
    double beta[kMaxBands];
    beta[0] = -1.0;
    if (method == 0) {
        if (estimate) {
            if (const int rc = estimate_sigma(bl, sigma); rc != PDWT_OK) return rc;
        }
        const double t = *sigma * sqrt(2.0 * log(bl.samples));
        for (int k = 1; k < bl.nb; k++) beta[k] = t;
    } else {
        // one moments launch over all bands; the median of the finest diagonal band rides along when sigma is to be estimated
        unsigned char want[kMaxBands] = {};
        want[bl.finest] = estimate ? 1 : 0;
        pdwt_band_stats s[kMaxBands];
        if (const int rc = PDWT_BL_SFX(pdwt_bandlist_stats)(bl.ptr, bl.n, bl.nb, want, s); rc != PDWT_OK) return rc;
        if (estimate) *sigma = s[bl.finest].median_abs / kMadScale;
        const double s2 = *sigma * *sigma;
        for (int k = 1; k < bl.nb; k++) {
            const double ms = s[k].n > 0 ? s[k].sum_sq / s[k].n : 0.0;
            beta[k] = ms > s2 ? s2 / sqrt(ms - s2) : s[k].max_abs;  // no signal above the noise: the band goes to zero
        }
    }
    for (int k = 0; k < bl.nb; k++) betas[k] = (DTYPE)beta[k];
    return threshold(bl, betas, kind);
}

}  // namespace pdwt_bl
