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

/* d_image, d_nodes (depths 0 .. WPT_MAX_LEVELS are used), wname and state are members of the base, with the methods that are not
 * declared here: forward, inverse, set_image (all B images), node_shape (of one node of one image), get_level (the whole depth
 * (B, 4^depth, nr, nc)), best_basis (over the costs summed over the images), set_basis, basis_size, get_basis, soft_threshold,
 * hard_threshold (in every image), node_stats (per (image, node): B * 4^depth entries, image-major; median_abs NaN), estimate_sigma
 * (pooled: median |node "d"| over all images / 0.6744897501960817) (include/wpt_tree.h; as WaveletPackets, include/wpt.h). */
class WaveletPacketsImages : public PacketTree {
  public:
    w_info_wptb winfos;

    WaveletPacketsImages(DTYPE* imgs, int B, int Nr, int Nc, const char* wname, int levels, int memisonhost = 1, int allow_fused = 1);

    long long get_image(DTYPE* imgs) { return tree_get_image(imgs); } /* all B images; elements copied */
    int fused() const { return tree_fused(); }                        /* 1: one launch per direction runs the whole tree of every image */

    static int geometry(int Nr, int Nc, int hlen, int levels, int* nr, int* nc); /* WaveletPackets::geometry */
    static int path_index(const char* path, int* depth);                         /* WaveletPackets::path_index */

    /* copy out / in: elements copied, 0 when refused.  A node is the (B, nr, nc) stack of that node across the images (a pitched copy).
     * set_node as WaveletPackets::set_node, with such a stack. */
    long long get_node(DTYPE* out, int depth, int idx) { return tree_get_node(out, depth, idx); }
    long long set_node(DTYPE* in, int depth, int idx, int mem_is_on_device = 0) { return tree_set_node(in, depth, idx, mem_is_on_device); }
    /* image 0's node; *pitch = elements between images */
    intptr_t node_int_ptr(int depth, int idx, long long* pitch = NULL) { return tree_node_ptr(depth, idx, pitch); }

    /* additive costs of a depth (0 .. L): per_image (B * 4^depth entries, image-major) and / or summed over the images in image order
     * (4^depth entries); either may be NULL.  kind 0 "l1", 1 "shannon".  PDWT_OK or a negative code. */
    int node_costs(int depth, int kind, double* per_image, double* summed);

    double norm1();                         /* sum |c| over the basis and the images, in double (the images_norm1 entries in image order); -1 when refused */
    int images_norm1(double* out);          /* the same per image (B entries) */
    int images_estimate_sigma(double* out); /* estimate_sigma per image (B entries), each from its own node "d" */
};

#endif
