/*
 * wpt1d.h -- `WaveletPackets1D`: the batched 1-D wavelet packet transform (the full binary tree of every row of an Nr x Nc batch,
 * pywt.WaveletPacket(mode='periodization'); no reference counterpart) with one Coifman-Wickerhauser best basis for the whole batch.
 * Same build as wt.h and wpt.h: plain host C++, DTYPE = float (libpdwt.so) or double (-DDOUBLEPRECISION, libpdwtd.so), every device
 * action a C-ABI call into libpdwt_hip.so (include/pdwt_hip.h "Batched 1-D wavelet packets"; kernels: pdwt_amd/csrc/wpt1d.hip).
 *
 * Nodes.  Depth 0 is the batch: Nr independent rows of n_0 = Nc samples, as Wavelets with ndim = 1.  Depth l has 2^l nodes per row of
 * n_l = div2(n_{l-1}) samples (ceil-half); node i has the children 2i (a) and 2i + 1 (d) of depth l + 1, the [A, D] bands of ONE level
 * of the periodised batched 1-D transform of Wavelets applied to it (Haar: the reference's 1-D Haar level).  A path has one letter
 * per depth, a=0 d=1, the first level the most significant ("ad" is node 1 of depth 2): natural (Paley) order; frequency_order gives
 * the Gray-code permutation.  Node 0 of depth l is A_l of Wavelets(ndim = 1), node 1 is D_l.
 * Levels are clamped to ilog2(Nc / (hlen - 1)) -- the rows do not count -- and to 12 (4096 nodes per row enter grid and table
 * sizes); a clamp to 0 levels is W_CREATION_ERROR.  Nr * Nc < 2^31.
 * Storage.  One device allocation per depth 1 .. L, laid out (Nr, 2^l, n_l) row-major: a row's depth-l line is one contiguous run,
 * so every store of every depth is coalesced however small n_l gets, get_level is a plain copy, and a node is a strided (Nr, n_l)
 * view with a pitch of 2^l * n_l elements (node-major, as WaveletPackets has it, would scatter 32-byte pieces at depth 9 of a
 * 4096-sample row).  forward() fills every depth and leaves the batch intact.  Device memory of an instance: about (L + 1) batches.
 * Paths.  When a row's two LDS lines fit a workgroup (fused(): float32 rows up to about 20 000 samples) forward() is ONE launch and
 * inverse() is ONE launch that writes the rows only; longer rows run one launch per depth and inverse() writes each synthesised
 * parent to its own storage, as WaveletPackets does.  Both paths give the same bits.  The nodes of the basis are never modified.
 * Basis.  A set of nodes that every root-to-leaf path meets exactly once, ONE for the whole batch; the default is all 2^L nodes of
 * depth L.  best_basis works on costs summed over the rows (in row order); node_costs also returns the per-row costs.
 * State machine: that of WaveletPackets (include/wpt.h), refusals included, on both paths.
 */
#ifndef WPT1D_H
#define WPT1D_H

#include "wpt_tree.h"

#define WPT1D_MAX_LEVELS 12

struct w_info_wpt1 {
    int Nr, Nc;
    int nlevels; /* after clamping */
    int hlen;
};

/* d_image, d_nodes, wname and state are members of the base, with the methods that are not declared here: forward, inverse, set_image,
 * node_shape, get_level, best_basis, set_basis, basis_size, get_basis, soft_threshold, hard_threshold, node_stats, estimate_sigma
 * (include/wpt_tree.h); they mean what they mean in WaveletPackets (include/wpt.h), with these differences:
 * node_shape(depth, &nr, &n): elements of one node (Nr * n_l) with its shape, 0 for a bad depth.  get_level copies the (Nr, 2^l, n_l)
 * allocation.  node_stats: of every node of a depth over all rows (out: 2^depth entries; median_abs NaN). */
class WaveletPackets1D : public PacketTree {
  public:
    w_info_wpt1 winfos;

    WaveletPackets1D(DTYPE* rows, int Nr, int Nc, const char* wname, int levels, int memisonhost = 1);

    int get_image(DTYPE* rows) { return (int)tree_get_image(rows); }
    int fused() const { return tree_fused(); } /* 1: the whole tree of a row is one launch; 0: one launch per depth */

    /* the depth an instance gets (levels < 1 asks for 1; 0 = too small or a bad size) and, in n when given, n_0 .. n_L */
    static int geometry(int Nc, int hlen, int levels, int* n);
    /* index of the node a path over "ad" names ("" = the batch), its depth in *depth; -1 for a bad letter or a path deeper than 12 */
    static int path_index(const char* path, int* depth);
    /* out[r] = r ^ (r >> 1): the natural index of the node of frequency rank r; the count 2^depth, or 0 for a bad depth */
    static int frequency_order(int depth, int* out);

    /* copy out / in (a node is Nr x n_l, dense on the host): elements copied, 0 when refused.  set_node needs the tree of a forward()
     * (W_FORWARD / W_THRESHOLD) and gives W_THRESHOLD. */
    int get_node(DTYPE* out, int depth, int idx) { return (int)tree_get_node(out, depth, idx); }
    int set_node(DTYPE* in, int depth, int idx, int mem_is_on_device = 0) { return (int)tree_set_node(in, depth, idx, mem_is_on_device); }
    /* device address of row 0 of a node; consecutive rows are *pitch ELEMENTS apart (2^depth * n_depth) */
    intptr_t node_int_ptr(int depth, int idx, long long* pitch) { return tree_node_ptr(depth, idx, pitch); }

    /* additive costs of all 2^depth nodes of a depth (0 .. L) in one launch, in double on the host, summed over the rows in row
     * order: kind 0 "l1" = sum |c|, kind 1 "shannon" = -sum c^2 ln c^2 (zero terms skipped).  per_row, when given, receives the
     * Nr * 2^depth costs of every (row, node).  PDWT_OK or a negative code. */
    int node_costs(int depth, int kind, double* out, double* per_row = 0);
    double norm1() { return tree_norm1(); } /* sum |c| over the basis, in double; -1 when refused */
};

#endif
