/*
 * swt3d.h -- `StationaryWavelets3D`: the separable, stationary (undecimated, a-trous) 3-D transform of a volume -- the
 * reference's do_swt with a third axis.  Same build as wt3d.h: plain host C++, DTYPE = float (libpdwt.so) or double
 * (-DDOUBLEPRECISION, libpdwtd.so), every device action a C-ABI call into libpdwt_hip.so (include/pdwt_hip.h).
 *
 * Volume: row-major Nz x Nr x Nc.  Level j = the 1-D a-trous level of Wavelets(..., do_swt=1, ndim=1) at tap spacing 2^(j-1)
 * along x, then y, then z; its input is the aaa band of level j-1.  No decimation: any size, odd sizes included.
 * Levels are clamped to ilog2(min(Nz, Nr, Nc) / (hlen - 1)); a clamp to 0 levels is W_CREATION_ERROR.
 * Sizes: Nz <= 65535 and Nr * Nc < 2^31 (the volume itself may be larger); otherwise W_CREATION_ERROR.
 * Device memory of an instance: the volume, 7L+1 full-size bands and a 4-volume scratch: (7L + 6) x the volume.
 * Bands: the indexing of Wavelets3D -- 0 = A_L, then for levels L .. 1 the details aad, ada, add, daa, dad, dda, ddd (first
 * letter = z axis) -- every band Nz x Nr x Nc.  inverse() leaves every band intact.
 * State machine: the one of Wavelets / Wavelets3D.  Not available: non-separable and custom banks, cycle spinning,
 * group_soft_threshold, shrink, proj_linf.
 */
#ifndef SWT3D_H
#define SWT3D_H

#include "wt3d.h"

class StationaryWavelets3D {
  public:
    DTYPE* d_image;   /* device: volume / reconstruction */
    DTYPE** d_coeffs; /* host array of 7L+1 device pointers (one allocation) */
    DTYPE* d_tmp;     /* device scratch */
    char wname[128];
    w_info3d winfos;
    w_state state;

    StationaryWavelets3D(DTYPE* vol, int Nz, int Nr, int Nc, const char* wname, int levels, int memisonhost = 1);
    ~StationaryWavelets3D();

    void forward();
    void inverse();
    void soft_threshold(DTYPE beta, int do_thresh_appcoeffs = 0, int normalize = 0);
    void hard_threshold(DTYPE beta, int do_thresh_appcoeffs = 0, int normalize = 0);
    DTYPE norm1();
    double norm1_double(); /* norm1() before its rounding to DTYPE */
    int get_image(DTYPE* vol);
    void set_image(DTYPE* vol, int mem_is_on_device = 0);
    int num_bands() const;
    /* elements of band num (and its shape), 0 for a bad index */
    long long band_shape(int num, int* bNz, int* bNr, int* bNc) const;
    int get_coeff(DTYPE* coeff, int num);
    void set_coeff(DTYPE* coeff, int num, int mem_is_on_device = 0);
    intptr_t image_int_ptr(void);
    intptr_t coeff_int_ptr(int num);
    /* ADDITIONS: band statistics and noise-adaptive thresholds, computed on the device (pdwt_amd/csrc/bandstats.hip).  All five need
     * valid coefficients (after forward(), before inverse(); the rules of Wavelets, wt.h); otherwise band_stats / all_band_stats return a negative value,
     * estimate_sigma / denoise return -1, threshold_bands does nothing, and nothing is launched.
     *   band_stats       n, sum |c|, sum c^2, max |c| (accumulated in double) and, with_median, the exact median of |c| of band num
     *   all_band_stats   the same for every band (out: 7L+1 entries) in ONE moments launch
     *   estimate_sigma   median |finest diagonal band| / 0.6744897501960817  (band 7L = ddd of level 1)
     *   threshold_bands  one beta per band (7L+1 betas); beta < 0 leaves the band alone; kind 0 soft, 1 hard
     *   denoise          method 0 VisuShrink: every detail band gets sigma * sqrt(2 ln N), N = Nz*Nr*Nc;
     *                    method 1 BayesShrink: detail band b gets sigma^2 / sqrt(ms_b - sigma^2), ms_b = sum c^2 / n, or max |c| (the band
     *                    goes to zero) when ms_b <= sigma^2.  sigma < 0: estimate_sigma().  Band 0 is never touched (beta -1).  Host
     *                    arithmetic in double, betas rounded to DTYPE once and returned in betas_out (7L+1 entries) when given.
     *                    Returns the sigma it used.  The rules assume an orthonormal bank; bior / rbio banks get them as they are. */
    int band_stats(int num, w_band_stats* out, int with_median = 1);
    int all_band_stats(w_band_stats* out, int with_median = 0);
    double estimate_sigma();
    void threshold_bands(const DTYPE* betas, int kind = 0);
    double denoise(int method, double sigma = -1.0, int kind = 0, DTYPE* betas_out = NULL);

  private:
    void* filters_; /* per-instance bank + device */
    StationaryWavelets3D(const StationaryWavelets3D&);
    StationaryWavelets3D& operator=(const StationaryWavelets3D&);
};

#endif
