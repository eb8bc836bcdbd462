/*
 * wpt.h -- `WaveletPackets`: the 2-D wavelet packet transform (the full quad-tree, every band decomposed again) with
 * Coifman-Wickerhauser best-basis selection (no reference counterpart: the reference decomposes the approximation band only).
 * Same build as wt.h: plain host C++, DTYPE = float (libpdwt.so) or double (-DDOUBLEPRECISION, libpdwtd.so), every device action a
 * C-ABI call into libpdwt_hip.so (include/pdwt_hip.h "2-D wavelet packets"; kernels: pdwt_amd/csrc/wpt2d.hip).
 *
 * Nodes.  Depth 0 is the image (Nr x Nc).  A node of depth l has div2^l(Nr) x div2^l(Nc) elements (ceil-half); its four children
 * are the [A, H, V, D] bands of the one-level 2-D transform of Wavelets applied to it (periodised; Haar: the clamped 2x2 butterfly).
 * Index.  A path has one digit per depth, a=0 h=1 v=2 d=3, the first level the most significant: node i of depth l has the
 * children 4i .. 4i+3 of depth l+1; "ahd" is node 0*16 + 1*4 + 3 = 7 of depth 3.  (Natural order, not frequency order.)
 * Levels are clamped to ilog2(min(Nr, Nc) / (hlen - 1)) as in Wavelets, and to 7 (depth 7 has 16384 nodes, and the node count is
 * a grid dimension); a clamp to 0 levels is W_CREATION_ERROR.  Nr * Nc < 2^31.
 * Storage.  One device allocation per depth 1 .. L, its 4^l nodes contiguous (node stride = nr_l * nc_l elements); forward() fills
 * every depth and leaves the image intact.  Device memory of an instance: about (L + 1) images.
 * Basis.  A set of nodes that every root-to-leaf path meets exactly once; the default is all 4^L nodes of depth L.  inverse()
 * reconstructs the image from the nodes of the current basis: it climbs one depth at a time, synthesises only the parents that lie
 * above basis nodes, each into its own storage (depth 0: the image), and leaves the basis nodes themselves unmodified.
 * State machine: the w_state rules of Wavelets.  After inverse() the coefficients are invalid: reading a node, the thresholds, the
 * costs and statistics, best_basis and a second inverse() are refused.  A threshold or set_node gives W_THRESHOLD (set_node itself
 * needs the tree of a forward() and is refused in every other state); best_basis and
 * set_basis are refused in that state (the tree is no longer one transform).  forward() keeps the current basis.
 */
#ifndef WPT_H
#define WPT_H

#include "wpt_tree.h"

#define WPT_MAX_LEVELS 7

struct w_info_wpt {
    int Nr, Nc;
    int nlevels; /* after clamping */
    int hlen;
};

/* d_image, d_nodes (depths 0 .. WPT_MAX_LEVELS are used), wname and state are members of the base, with the methods that are not
 * declared here: forward, inverse, set_image, node_shape, get_level, best_basis, set_basis, basis_size, get_basis, soft_threshold,
 * hard_threshold, node_stats, estimate_sigma (include/wpt_tree.h).
 * node_shape(depth, &nr, &nc) (valid unless W_CREATION_ERROR): nodes of a depth = 4^depth; elements of one node, 0 for a bad depth. */
class WaveletPackets : public PacketTree {
  public:
    w_info_wpt winfos;

    WaveletPackets(DTYPE* img, int Nr, int Nc, const char* wname, int levels, int memisonhost = 1);

    int get_image(DTYPE* img) { return (int)tree_get_image(img); }

    /* the depth an instance of this size gets (levels < 1 asks for 1; clamped to ilog2(min(Nr, Nc) / (hlen - 1)) and WPT_MAX_LEVELS;
     * 0 = too small or a bad size) and, in nr / nc when given, the node shape of depth 0 .. that depth.  What the constructor uses. */
    static int geometry(int Nr, int Nc, int hlen, int levels, int* nr, int* nc);
    /* index of the node a path names ("" = the image), its depth in *depth; -1 for a bad letter or a path deeper than L */
    static int path_index(const char* path, int* depth);

    /* copy out / in: elements copied, 0 when refused.  get_level copies all 4^depth nodes of a depth.  set_node needs the tree
     * of a forward() (W_FORWARD / W_THRESHOLD; refused otherwise, also after inverse()) and gives W_THRESHOLD. */
    int get_node(DTYPE* out, int depth, int idx) { return (int)tree_get_node(out, depth, idx); }
    int set_node(DTYPE* in, int depth, int idx, int mem_is_on_device = 0) { return (int)tree_set_node(in, depth, idx, mem_is_on_device); }
    intptr_t node_int_ptr(int depth, int idx) { return tree_node_ptr(depth, idx, NULL); }

    /* additive costs of all 4^depth nodes of a depth (0 .. L; depth 0 = the image) in one launch, in double on the host:
     * kind 0 "l1" = sum |c|, kind 1 "shannon" = -sum c^2 ln c^2 (zero terms skipped).  PDWT_OK or a negative code. */
    int node_costs(int depth, int kind, double* out);
    /* best_basis(kind): bottom-up best basis on the host: a parent is kept when its cost is <= the sum of its children's best costs.
     * Installs the basis; returns the number of its nodes (see get_basis), or a negative code when refused.
     * set_basis(depth, idx, n): install a basis given as n (depth, idx) pairs; PDWT_EINVAL unless they partition the tree (overlap, gap,
     * bad index).  get_basis(depth, idx): sorted by (depth, idx); returns the count.
     * soft_threshold / hard_threshold(beta, do_thresh_appcoeffs = 0): on the nodes of the current basis; the all-"a" node only when
     * do_thresh_appcoeffs; one launch per depth that holds basis nodes.
     * node_stats(depth, out): n, sum |c|, sum c^2, max |c| of every node of a depth (out: 4^depth entries; median_abs NaN).
     * estimate_sigma(): median |node "d"| / 0.6744897501960817; -1 when refused. */
    double norm1() { return tree_norm1(); } /* sum |c| over the basis, in double; -1 when refused */
};

#endif
