/*
 * wt3d.h -- `Wavelets3D` (and `Transform3D`, the base it shares with `StationaryWavelets3D` of swt3d.h): the separable, decimated, periodised 3-D DWT of a volume (no reference counterpart: the
 * reference's Wavelets refuses ndims == 3).  Same build as wt.h: plain host C++, DTYPE = float (libpdwt.so) or double
 * (-DDOUBLEPRECISION, libpdwtd.so), every device action a C-ABI call into libpdwt_hip.so (include/pdwt_hip.h).
 *
 * Volume: row-major Nz x Nr x Nc.  One level = the 1-D level of Wavelets(..., ndim=1) along x, then y, then z.
 * Levels are clamped to ilog2(min(Nz, Nr, Nc) / (hlen - 1)); a clamp to 0 levels is W_CREATION_ERROR.
 * Sizes: Nz <= 65535 and Nr * Nc < 2^31 (the volume itself may be larger, e.g. 2048^3); otherwise W_CREATION_ERROR.
 * Device memory of an instance: the volume, the bands (about 1.0x the volume) and the scratch d_tmp (about 1.13x): ~3.1x the volume.
 * Bands (get_coeff / set_coeff / coeff_int_ptr): 0 = A_L, then for levels L .. 1 the 7 detail bands of the level in the key
 * order of PyWavelets' dwtn -- aad, ada, add, daa, dad, dda, ddd (first letter = z axis) -- so band 1 + 7*(L - lev) + k is
 * detail k of level lev (1 = finest).  A level-lev band has div2^lev(Nz) x div2^lev(Nr) x div2^lev(Nc) elements.
 * State machine: the w_state rules of Wavelets (threshold / get_coeff after inverse() are refused, inverse() twice is
 * refused).  Not available in 3-D: SWT, non-separable and custom banks, cycle spinning, group_soft_threshold, shrink, proj_linf.
 */
#ifndef WT3D_H
#define WT3D_H

#include "wt.h"

struct w_info3d {
    int Nz;      /* planes */
    int Nr;      /* rows per plane */
    int Nc;      /* columns per row */
    int nlevels; /* decomposition levels, after clamping */
    int hlen;    /* filter length */
};

struct w_ops3d; /* what one transform contributes: its name, entry points and the two texts that differ (pdwt_amd/csrc/wt3d.cpp) */

/* Everything `Wavelets3D` and `StationaryWavelets3D` (swt3d.h) share, which is all but their constructors: one implementation in
 * pdwt_amd/csrc/wt3d.cpp, the transform chosen by the table the derived constructor passes in.  Not instantiable, not copyable. */
class Transform3D {
  public:
    DTYPE* d_image;   /* device: volume / reconstruction */
    DTYPE** d_coeffs; /* host array of 7L+1 device pointers (one allocation) */
    DTYPE* d_tmp;     /* device scratch */
    char wname[128];
    w_info3d winfos;
    w_state state;

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

  protected:
    Transform3D(const w_ops3d& ops, DTYPE* vol, int Nz, int Nr, int Nc, const char* wname, int levels, int memisonhost);
    ~Transform3D(); /* not virtual: destroy an instance through its concrete class */

  private:
    const w_ops3d* ops_; /* set first: valid after every W_CREATION_ERROR return */
    void* filters_;      /* per-instance bank + device */
    Transform3D(const Transform3D&);
    Transform3D& operator=(const Transform3D&);
};

class Wavelets3D : public Transform3D {
  public:
    Wavelets3D(DTYPE* vol, int Nz, int Nr, int Nc, const char* wname, int levels, int memisonhost = 1);
};

#endif
