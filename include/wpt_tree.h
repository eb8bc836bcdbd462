/*
 * wpt_tree.h -- `PacketTree`: what the three wavelet packet classes share, `WaveletPackets` (wpt.h), `WaveletPackets1D` (wpt1d.h) and
 * `WaveletPacketsImages` (wpt_batch.h): every member but `winfos`, and every method whose signature is the same in the three.  A tree
 * of arity 4 or 2 with one device allocation per depth, in 1, Nr or B copies (the image; the rows; the images of a stack) that share ONE
 * basis.  Written once in pdwt_amd/csrc/wpt.cpp; what differs between the classes is one `wp_ops` table each.  Not for direct use: the
 * three headers document the methods.
 */
#ifndef WPT_TREE_H
#define WPT_TREE_H

#include "wt.h"

#define PACKET_TREE_MAX_LEVELS 12 /* the deepest of the three trees (WPT1D_MAX_LEVELS) */

struct wp_ops;
class PacketTree {
  public:
    DTYPE* d_image;                               /* device: the input / its reconstruction = depth 0 */
    DTYPE* d_nodes[PACKET_TREE_MAX_LEVELS + 1];   /* device: the allocation of each depth ([0] = d_image); NULL beyond the depth of the class */
    char wname[128];
    w_state state;

    void forward();
    void inverse();
    void set_image(DTYPE* img, int mem_is_on_device = 0);
    long long node_shape(int depth, int* nr, int* nc) const;
    long long get_level(DTYPE* out, int depth);

    int best_basis(int kind);
    int set_basis(const int* depth, const int* idx, int n);
    int basis_size() const;
    int get_basis(int* depth, int* idx) const;

    void soft_threshold(DTYPE beta, int do_thresh_appcoeffs = 0);
    void hard_threshold(DTYPE beta, int do_thresh_appcoeffs = 0);
    int node_stats(int depth, w_band_stats* out);
    double estimate_sigma();

  protected:
    PacketTree();
    ~PacketTree();
    /* the constructor of all three: dims = {copies that are no rows of the node, Nr, Nc} (the images of a stack; 1 otherwise); *nlevels
     * holds the levels asked for and gets the clamped ones, *hlen the length of the bank, as far as the construction came */
    void create(const wp_ops& ops, DTYPE* src, const int* dims, const char* wname, int memisonhost, int allow_fused, int* nlevels, int* hlen);
    /* what the classes declare under their own signatures (int or long long counts, an optional pitch) */
    long long tree_get_image(DTYPE* out);
    long long tree_get_node(DTYPE* out, int depth, int idx);
    long long tree_set_node(DTYPE* in, int depth, int idx, int mem_is_on_device);
    intptr_t tree_node_ptr(int depth, int idx, long long* pitch);
    int tree_fused() const;
    double tree_norm1(); /* over the basis, from the costs of each depth summed over the copies */
    const wp_ops* ops_;  /* which of the three trees this is */
    void* priv_;         /* bank, device, geometry, basis, device tables */

  private:
    void threshold(int op, DTYPE beta, int do_thresh_appcoeffs);
    PacketTree(const PacketTree&);
    PacketTree& operator=(const PacketTree&);
};

#endif
