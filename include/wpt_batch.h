/*
 * wpt_batch.h -- `WaveletPacketsImages`: the 2-D wavelet packet transform of `WaveletPackets` (wpt.h) on every image of a B x Nr x Nc
 * stack -- texture patches, tiles, detector frames -- with ONE best basis for the batch.  Same build as wt.h: plain host C++, DTYPE = float
 * (libpdwt.so) or double (-DDOUBLEPRECISION, libpdwtd.so), every device action a C-ABI call into libpdwt_hip.so (include/pdwt_hip.h
 * "Batched 2-D wavelet packets"; kernels: pdwt_amd/csrc/wpt2db.hip).
 *
 * Per image the tree is exactly that of WaveletPackets: the periodised one-level [A, H, V, D] split of every node (Haar: the clamped
 * 2x2 butterfly), ceil-half node shapes, natural order with the path digits a h v d, the level clamp ilog2(min(Nr, Nc) / (hlen - 1))
 * and WPT_MAX_LEVELS; a clamp to 0 levels is W_CREATION_ERROR.  The results are the bits a WaveletPackets instance gives on that image.
 * Limits: 1 <= B <= 65535, Nr * Nc < 2^31, B * 4^L <= 2^22.
 * Storage.  One device allocation per depth 1 .. L laid out (B, 4^l, nr_l, nc_l), image-major: image b's depth-l line is one contiguous
 * run; node i of a depth is a (B, nr_l, nc_l) stack with a pitch of 4^l nr_l nc_l elements.  forward() fills every depth and leaves the
 * images intact.  Device memory of an instance: about (L + 1) batches.
 * Forms.  fused(): the whole tree of an image runs in the LDS of one workgroup, one launch per direction (pdwt_wptb_fused says when;
 * allow_fused = 0 turns it off); otherwise the level entries of WaveletPackets run over the forest of all images, depth by depth.  Both
 * give the same bits.  After a fused inverse() only the images are rewritten; the per-depth form also rewrites the parents above the
 * basis.  The basis nodes themselves are never modified by inverse().
 * Basis.  ONE basis serves every image (the default: all 4^L nodes of depth L); best_basis() chooses it from the costs summed over the
 * images, in image order.  State machine, refusals and messages: those of WaveletPackets.
 */
#ifndef WPT_BATCH_H
#define WPT_BATCH_H

#include "wpt.h"

struct w_info_wptb {
    int B, Nr, Nc;
    int nlevels; /* after clamping */
    int hlen;
};

class WaveletPacketsImages {
  public:
    DTYPE* d_image;                      /* device: the B images / reconstructions = the nodes of depth 0 */
    DTYPE* d_nodes[WPT_MAX_LEVELS + 1];  /* device: the allocation of each depth ([0] = d_image) */
    char wname[128];
    w_info_wptb winfos;
    w_state state;

    WaveletPacketsImages(DTYPE* imgs, int B, int Nr, int Nc, const char* wname, int levels, int memisonhost = 1, int allow_fused = 1);
    ~WaveletPacketsImages();

    void forward();
    void inverse();
    long long get_image(DTYPE* imgs);                         /* all B images; elements copied */
    void set_image(DTYPE* imgs, int mem_is_on_device = 0);    /* all B images */
    int fused() const;                                        /* 1: one launch per direction runs the whole tree of every image */

    /* geometry (valid unless W_CREATION_ERROR): nodes of a depth per image = 4^depth; elements of one node of one image, 0 for a bad depth */
    long long node_shape(int depth, int* nr, int* nc) const;
    static int geometry(int Nr, int Nc, int hlen, int levels, int* nr, int* nc); /* WaveletPackets::geometry */
    static int path_index(const char* path, int* depth);                         /* WaveletPackets::path_index */

    /* copy out / in: elements copied, 0 when refused.  A node is the (B, nr, nc) stack of that node across the images (a pitched copy);
     * get_level copies the whole depth (B, 4^depth, nr, nc).  set_node as WaveletPackets::set_node, with such a stack. */
    long long get_node(DTYPE* out, int depth, int idx);
    long long get_level(DTYPE* out, int depth);
    long long set_node(DTYPE* in, int depth, int idx, int mem_is_on_device = 0);
    intptr_t node_int_ptr(int depth, int idx, long long* pitch = NULL); /* image 0's node; *pitch = elements between images */

    /* additive costs of a depth (0 .. L): per_image (B * 4^depth entries, image-major) and / or summed over the images in image order
     * (4^depth entries); either may be NULL.  kind 0 "l1", 1 "shannon".  PDWT_OK or a negative code. */
    int node_costs(int depth, int kind, double* per_image, double* summed);
    int best_basis(int kind); /* over the summed costs; a parent is kept when its cost is <= its children's.  Returns the basis size */
    int set_basis(const int* depth, const int* idx, int n);
    int basis_size() const;
    int get_basis(int* depth, int* idx) const;

    /* on the nodes of the current basis in every image; the all-"a" node only when do_thresh_appcoeffs */
    void soft_threshold(DTYPE beta, int do_thresh_appcoeffs = 0);
    void hard_threshold(DTYPE beta, int do_thresh_appcoeffs = 0);
    double norm1();                    /* sum |c| over the basis and the images, in double; -1 when refused */
    int images_norm1(double* out);     /* the same per image (B entries) */
    int node_stats(int depth, w_band_stats* out); /* per (image, node): B * 4^depth entries, image-major (median_abs NaN) */
    double estimate_sigma();           /* pooled: median |node "d"| over all images / 0.6744897501960817; -1 when refused */
    int images_estimate_sigma(double* out); /* the same per image (B entries) */

  private:
    void* priv_;
    void threshold(int op, DTYPE beta, int do_thresh_appcoeffs);
    WaveletPacketsImages(const WaveletPacketsImages&);
    WaveletPacketsImages& operator=(const WaveletPacketsImages&);
};

#endif
