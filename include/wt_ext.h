/*
 * wt_ext.h -- `BoundaryWavelets`: the multi-level 2-D DWT with signal-extension boundary modes (no reference counterpart: the reference
 * and every other class here periodise).  Same build as wt.h: plain host C++, DTYPE = float (libpdwt.so) or double (-DDOUBLEPRECISION,
 * libpdwtd.so), every device action a C-ABI call into libpdwt_hip.so (include/pdwt_hip.h "2-D DWT with boundary modes"; kernels:
 * pdwt_amd/csrc/dwt_ext.hip).
 * `BoundaryWavelets1D`, further down, is the same transform along the last axis of a batch of rows; `BoundaryWavelets3D`, below
 * it, along the three axes of a volume; `BoundaryWaveletsImages`, at the end, the 2-D transform of every image of a batch.
 *
 * Modes (PyWavelets' names and semantics): 0 zero, 1 constant, 2 symmetric (PyWavelets' default), 3 reflect, 4 periodic.  The
 * transform is pywt.wavedec2 of those modes: a level takes an nr x nc approximation to four bands of ((nr + hlen - 1) / 2) x
 * ((nc + hlen - 1) / 2), so the bands of L levels hold MORE samples than the image.  inverse() needs no mode and trims like
 * pywt.waverec2.  Haar runs the bank's own taps (1/sqrt 2), not the 0.5 butterfly of the periodised Haar levels.
 * Bands.  [A_L, H1, V1, D1, ..., H_L, V_L, D_L], level 1 the finest, the orientation of Wavelets (H = row low / column high).
 * Levels are clamped as in Wavelets to ilog2(min(Nr, Nc) / (hlen - 1)) (PyWavelets' dwt_max_level) and to 32 (97 bands, the limit of
 * the band-list kernels); a clamp to 0 levels is W_CREATION_ERROR.  Nr * Nc < 2^31.
 * Storage.  All bands in ONE device allocation at 256-byte offsets, and two buffers of the size of a level-1 band for the
 * intermediate approximations: forward() leaves the image intact, inverse() leaves the bands intact.  Device memory of an instance:
 * about 2.5 images plus the halo growth of the bands.
 * State machine: the w_state rules of Wavelets.  After inverse() reading a band, the thresholds, norm1 and the statistics are refused
 * until the next forward(); set_image gives W_INIT; set_coeff is allowed in every state but W_CREATION_ERROR and leaves it alone
 * (coefficients written from outside may be inverted without a forward()).  The statistics, threshold_bands and denoise need the
 * coefficients of a forward() (W_FORWARD / W_THRESHOLD).
 */
#ifndef WT_EXT_H
#define WT_EXT_H

#include "wt.h"

#define BW_MAX_LEVELS 32
#define BW_NUM_MODES 5

struct w_info_bw {
    int Nr, Nc;
    int nlevels; /* after clamping */
    int hlen;
    int mode;
};

/* What the four classes of this header share: every member but `winfos`, and every method whose signature does not name the number of
 * axes.  Written once in pdwt_amd/csrc/wt_ext.cpp; what differs between the classes is one `bw_ops` table each.  Not for direct use. */
struct bw_ops;
class BoundaryTransform {
  public:
    DTYPE* d_image;   /* device: the input / its reconstruction */
    DTYPE** d_coeffs; /* HOST table of num_bands() device pointers into one allocation */
    char wname[128];
    w_state state;

    void forward();
    void inverse();
    int get_image(DTYPE* img);
    void set_image(DTYPE* img, int mem_is_on_device = 0);

    int num_bands() const;                /* 3L+1 (2-D), L+1 (1-D), 7L+1 (3-D); 0 after W_CREATION_ERROR */
    int get_coeff(DTYPE* coeff, int num); /* elements copied, 0 when refused */
    void set_coeff(DTYPE* coeff, int num, int mem_is_on_device = 0);
    intptr_t image_int_ptr();
    intptr_t coeff_int_ptr(int num);

    /* every detail band; the approximation only when do_thresh_appcoeffs.  One launch. */
    void soft_threshold(DTYPE beta, int do_thresh_appcoeffs = 0);
    void hard_threshold(DTYPE beta, int do_thresh_appcoeffs = 0);
    double norm1(); /* sum |c| over all bands, in double; -1 when refused */

    /* the additions of wt.h on these bands (the finest diagonal band and N of the universal threshold: see each class), same meaning */
    int band_stats(int num, w_band_stats* out, int with_median = 1);
    int all_band_stats(w_band_stats* out, int with_median = 0);
    double estimate_sigma();
    void threshold_bands(const DTYPE* betas, int kind = 0);
    double denoise(int method, double sigma = -1.0, int kind = 0, DTYPE* betas_out = NULL);

  protected:
    BoundaryTransform();
    ~BoundaryTransform();
    /* the constructor of all four: dims = {Nz, Nr, Nc} (1 for an axis the class does not have; the images of a batch are Nz); *nlevels holds the levels asked for and
     * gets the clamped ones, *hlen the length of the bank, as far as the construction came */
    void create(const bw_ops& ops, DTYPE* src, const int* dims, const char* wname, int mode, int memisonhost, int* nlevels, int* hlen);
    long long band_shape(int num, int* shape) const; /* elements of band num and its {nz, nr, nc}; 0 for a bad index */
    const bw_ops* ops_;                              /* which of the four transforms this is */
    void* priv_;                                     /* bank, device, geometry, the band allocation, the scratch */

  private:
    void threshold(int op, DTYPE beta, int do_thresh_appcoeffs);
    BoundaryTransform(const BoundaryTransform&);
    BoundaryTransform& operator=(const BoundaryTransform&);
};

class BoundaryWavelets : public BoundaryTransform {
  public:
    w_info_bw winfos;

    BoundaryWavelets(DTYPE* img, int Nr, int Nc, const char* wname, int levels, int mode, int memisonhost = 1);

    /* the levels an instance of this size gets (levels < 1 asks for 1; clamped to ilog2(min(Nr, Nc) / (hlen - 1)) and BW_MAX_LEVELS;
     * 0 = too small or a bad size / bank length) and, in nr / nc when given, the shape of the approximation of level 0 (the image) ..
     * that level: the bands of level l are nr[l] x nc[l].  Needs no device.  What the constructor uses. */
    static int geometry(int Nr, int Nc, int hlen, int levels, int* nr, int* nc);
    /* the mode number of a PyWavelets mode name, -1 for any other */
    static int mode_index(const char* name);

    /* elements of band num, 0 for a bad index.  The finest diagonal band is D1 (band 3), N of the universal threshold Nr * Nc. */
    long long coeff_shape(int num, int* nr, int* nc) const;
};

/*
 * `BoundaryWavelets1D`: the same along the LAST axis only, for a batch of Nr independent rows of Nc samples -- pywt.wavedec(x, wname,
 * mode, levels, axis=-1) (include/pdwt_hip.h "Batched 1-D DWT with boundary modes"; kernels: pdwt_amd/csrc/dwt_ext1d.hip).  Member for
 * member the class above, with these differences:
 * Bands.  [A_L, D_1, ..., D_L], level 1 the finest, band l row-major Nr x N_l, N_l = (N_{l-1} + hlen - 1) / 2: the order of Wavelets
 * with ndim = 1.  Levels are clamped to ilog2(Nc / (hlen - 1)) and to 32; a clamp to 0 levels is W_CREATION_ERROR.  Nr * Nc < 2^31.
 * One launch.  When a row fits the LDS of a workgroup (fused() == 1) forward() and inverse() are ONE kernel launch each, whatever the
 * number of levels: the batch is read once and every band written once.  Longer rows run one launch per level through a scratch
 * buffer of two level-1 approximations, which only such an instance allocates.  Both paths give the same bits.
 * Statistics.  The finest detail band is band 1 (all rows together); N of the universal threshold is Nc, the batched-1-D rule of wt.h.
 */
class BoundaryWavelets1D : public BoundaryTransform {
  public:
    w_info_bw winfos;

    BoundaryWavelets1D(DTYPE* img, int Nr, int Nc, const char* wname, int levels, int mode, int memisonhost = 1);

    /* the levels a row of Nc samples gets (levels < 1 asks for 1; clamped to ilog2(Nc / (hlen - 1)) and BW_MAX_LEVELS; 0 = too short or
     * a bad size / bank length) and, in n when given, the samples per row of level 0 (the batch) .. that level.  Needs no device. */
    static int geometry(int Nc, int hlen, int levels, int* n);

    long long coeff_shape(int num, int* nr, int* nc) const; /* elements of band num (Nr x N_l), 0 for a bad index */
    int fused() const; /* 1: forward() and inverse() of this instance are one launch each; 0 after W_CREATION_ERROR */
};

/*
 * `BoundaryWavelets3D`: the same along all three axes of an Nz x Nr x Nc volume -- pywt.wavedecn(vol, wname, mode, levels)
 * (include/pdwt_hip.h "3-D DWT with boundary modes"; kernels: pdwt_amd/csrc/dwt_ext3d.hip).  One level applies the one-axis formula
 * along x (the last axis), then y, then z, and takes an nz x nr x nc approximation to eight bands of ((nz + hlen - 1) / 2) x
 * ((nr + hlen - 1) / 2) x ((nc + hlen - 1) / 2).  Member for member the first class above, with these differences:
 * Bands.  The order of Wavelets3D (include/wt3d.h) and of pywt.wavedecn: [A_L, the 7 details of level L, ..., those of level 1];
 * detail k of level lev (1 = finest) is band 1 + 7 * (L - lev) + k, k in the order aad, ada, add, daa, dad, dda, ddd (first letter =
 * z axis).  Levels are clamped to ilog2(min(Nz, Nr, Nc) / (hlen - 1)) and to 13 (92 bands); a clamp to 0 levels is W_CREATION_ERROR.
 * Nz <= 65535 and Nr * Nc < 2^31.
 * Storage.  All bands in ONE zero-filled device allocation at 256-byte offsets, and one scratch buffer of four level-1 quadrants
 * (Nz x N_r1 x N_c1 each) plus one level-1 approximation, through which the approximation of every level but the last goes: forward()
 * leaves the volume intact, inverse() leaves the bands intact.  Two launches per level and direction.
 * Statistics.  The finest diagonal band is ddd of level 1 (band 7L); N of the universal threshold is Nz * Nr * Nc.
 */
#define BW3_MAX_LEVELS 13

struct w_info_bw3 {
    int Nz, Nr, Nc;
    int nlevels; /* after clamping */
    int hlen;
    int mode;
};

class BoundaryWavelets3D : public BoundaryTransform {
  public:
    w_info_bw3 winfos;

    BoundaryWavelets3D(DTYPE* vol, int Nz, int Nr, int Nc, const char* wname, int levels, int mode, int memisonhost = 1);

    /* the levels a volume of this size gets (levels < 1 asks for 1; clamped to ilog2(min(Nz, Nr, Nc) / (hlen - 1)) and
     * BW3_MAX_LEVELS; 0 = too small or a bad size / bank length) and, in nz / nr / nc when given, the shape of the approximation of
     * level 0 (the volume) .. that level: the bands of level l are nz[l] x nr[l] x nc[l].  Needs no device. */
    static int geometry(int Nz, int Nr, int Nc, int hlen, int levels, int* nz, int* nr, int* nc);

    long long coeff_shape(int num, int* nz, int* nr, int* nc) const; /* elements of band num, 0 for a bad index */
};

/*
 * `BoundaryWaveletsImages`: the 2-D transform of the first class on every image of a B x Nr x Nc batch -- pywt.wavedec2(x, wname, mode,
 * levels, axes=(-2, -1)) (include/pdwt_hip.h "Batched 2-D DWT with boundary modes"; kernels: pdwt_amd/csrc/dwt_ext2db.hip).  Definitions,
 * band order, orientation and level clamp are those of BoundaryWavelets; member for member that class, with these differences:
 * Bands.  Band num is ONE contiguous B x nr_l x nc_l stack, image-major: band num of image b is d_coeffs[num] + b * nr_l * nc_l.
 * get_coeff / set_coeff move a whole stack, get_image / set_image the whole batch.  1 <= B <= 65535, Nr * Nc < 2^31.
 * One launch.  When the pyramid of one image fits the LDS of a workgroup (fused() == 1: float32 up to about 140 x 140) forward() and
 * inverse() are ONE kernel launch each, whatever the number of levels and images: one workgroup per image, the batch read once, every
 * band written once.  Larger images run one launch per level through two scratch stacks of level-1 size, which only such an
 * instance allocates.  Both paths, and a loop over B BoundaryWavelets instances, give the same bits.
 * Statistics, two sets.
 *   POOLED (the inherited methods: band_stats, all_band_stats, estimate_sigma, threshold_bands, denoise, norm1, soft_threshold,
 *   hard_threshold): a band is the whole stack, as BoundaryWavelets1D pools its rows.  The finest diagonal band is the D1 stack
 *   (band 3) of all images together; N of the universal threshold is Nr * Nc (one image).
 *   PER IMAGE (the images_* methods below, the semantics of WaveletsImages, include/wt_batch.h): arrays are image-major with
 *   B * num_bands() entries, entry [b * num_bands() + k] = band k of image b.  Every call is a fixed number of launches and one copy to
 *   the host whatever B (the pdwt_bandbatch_* entries over a device table of the B * num_bands() slice pointers, built on first use).
 *   They return PDWT_OK, PDWT_EINVAL when refused (the coefficients of a forward() are needed, as for the pooled set; images_norm1
 *   only needs them readable), or the code of the entry that failed.
 */
struct w_info_bwb {
    int B, Nr, Nc;
    int nlevels; /* after clamping */
    int hlen;
    int mode;
};

#define BWB_MAX_IMAGES 65535

class BoundaryWaveletsImages : public BoundaryTransform {
  public:
    w_info_bwb winfos;

    BoundaryWaveletsImages(DTYPE* imgs, int B, int Nr, int Nc, const char* wname, int levels, int mode, int memisonhost = 1);

    /* elements of band num (the whole stack) and its shape B x nr x nc, 0 for a bad index */
    long long coeff_shape(int num, int* b, int* nr, int* nc) const;
    int fused() const; /* 1: forward() and inverse() of this instance are one launch each; 0 after W_CREATION_ERROR */

    int images_all_band_stats(w_band_stats* out, int with_median = 0); /* out: B * num_bands() */
    int images_estimate_sigma(double* sigma_out);                      /* B sigmas, each from its own D1 */
    int images_threshold_bands(const DTYPE* betas, int kind = 0);      /* betas: B * num_bands(); a negative beta leaves that band alone */
    /* sigma_in NULL or sigma_in[b] < 0: estimated from image b.  method 0 VisuShrink, 1 BayesShrink (the rule of wt.h, per image);
     * sigma_out: B; betas_out (may be NULL): B * num_bands(), band 0 of every image -1 */
    int images_denoise(int method, const double* sigma_in, int kind, double* sigma_out, DTYPE* betas_out = NULL);
    int images_norm1(double* out); /* B sums |c| over the bands of each image, in double */
};

#endif
