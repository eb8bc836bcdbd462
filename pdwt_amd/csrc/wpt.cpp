// wpt.cpp -- host side of the three wavelet packet classes, `WaveletPackets` (include/wpt.h: the quad-tree of one image),
// `WaveletPackets1D` (include/wpt1d.h: the binary tree of every row of a batch) and `WaveletPacketsImages` (include/wpt_batch.h: the
// quad-tree of every image of a stack), above the packet entry points of include/pdwt_hip.h, and their flat C handle APIs (pdwt_wpt_*,
// pdwt_wp1h_*, pdwt_wpbh_*: pdwt_amd/wpt.py).  Every method the three have in common is written once, on their base `PacketTree`
// (include/wpt_tree.h): a tree of arity 4 or 2, one allocation per depth, in 1, Nr or B copies that share one basis.  What differs
// between the classes is one `wp_ops` table each: names and nouns, the geometry, and the functions that reach the device -- the
// transforms, the costs, the statistics and the threshold of one depth go through three different families of entry points.  Plain host
// C++ like wt.cpp, built into libpdwt.so (float) and libpdwtd.so (-DDOUBLEPRECISION).  The tree geometry, the basis (the node-state
// table: 1 = a node of the basis, 2 = above it, 0 = below it) and the best-basis search live here.
#include <limits.h>
#include <math.h>
#include <new>
#include <string.h>
#include <vector>

#include "../../include/wpt1d.h"
#include "../../include/wpt_batch.h"
#include "host_common.hpp"

static_assert(sizeof(w_band_stats) == sizeof(pdwt_band_stats), "w_band_stats must mirror pdwt_band_stats");
static_assert(WPT1D_MAX_LEVELS == PACKET_TREE_MAX_LEVELS && WPT_MAX_LEVELS <= PACKET_TREE_MAX_LEVELS, "d_nodes of the base holds the deepest tree");

namespace {
constexpr int kL = PACKET_TREE_MAX_LEVELS;
constexpr int kCostChunk = 65535;  // nodes per pdwt_wpt2d_node_cost call

struct wp_priv {
    filters_t f;
    int dev;             // the device current when the first allocation was made; every method runs there.  -1: a failed instance
    int arity, L;        // children per node; winfos.nlevels after clamping
    int copies;          // trees that share the basis: 1, Nr rows, B images
    int Nr, Nc;          // of one image; 1-D: the batch
    int allow_fused, fused;
    int nr[kL + 1], nc[kL + 1];                   // node_shape of each depth (1-D: nr = Nr, the rows of the batch)
    size_t elems[kL + 1];                         // elements of one node of one copy
    std::vector<unsigned char> in_basis[kL + 1];  // per depth: 1 = the node belongs to the basis
    std::vector<unsigned char> state;             // the node-state table of the basis (pdwt_wp1_state_table / pdwt_wptb_state_table)
    std::vector<int> parents[kL + 1];             // single image: per depth, the nodes above basis nodes (what inverse() synthesises)
    unsigned char* d_state;                       // device: the state table (1-D, batch)
    unsigned char* d_thr;                         // device, 1-D: 1 = a basis node other than the all-"a" node of its depth
    int* d_lists;       // device: single image: parents[l] at ptr_off[l]; batch: pdwt_wptb_chunk_lists of the table (per-depth form), or NULL
    DTYPE** d_ptr;      // device: the pointers of every (copy, node), depth l at ptr_off[l] (single image: built at construction; batch: on first use)
    size_t ptr_off[kL + 2];
};
inline wp_priv* P(void* p) { return (wp_priv*)p; }

inline int nnodes(const wp_priv* p, int depth) { return 1 << ((p->arity == 4 ? 2 : 1) * depth); }
inline int nnodes(int arity, int depth) { return 1 << ((arity == 4 ? 2 : 1) * depth); }
// where depth l starts in the node-state table: (arity^l - 1) / (arity - 1)
inline size_t toff(int arity, int depth) { return (size_t)(nnodes(arity, depth) - 1) / (size_t)(arity - 1); }
// bytes of the table of a tree of L depths (the binary one ends with a byte of padding: pdwt_wp1_state_table)
inline size_t state_bytes(int arity, int L) { return toff(arity, L + 1) + (arity == 2 ? 1 : 0); }
}  // namespace

// What one class contributes to the shared one.  The transforms, costs, statistics and thresholds stay three separate sets of functions:
// each class drives its own entry points of include/pdwt_hip.h with its own tables, and their results are compared bit for bit.
struct wp_ops {
    const char* name;
    int arity;              // children per node: 4 or 2 (the level clamp is the geometry function's)
    const char* noun;       // "invalid <noun> size or wavelet name"
    bool rows_are_copies;   // 1-D: the Nr rows are the copies, a node of one copy is n_l samples (else nr_l x nc_l)
    bool pitched;           // a node is a strided view of its depth: pitched copies, a gather before the median (single image: contiguous)
    int max_copies;         // batch: the largest B (with a message of its own); 0: no such check
    long long max_forest;   // batch: the most nodes of one depth over all images; 0: no such check
    const char* size_fmt;   // the transformed sizes in the clamp messages
    const char* too_small;  // "ERROR: <sizes> <too_small> for one level of <wname>"
    int (*geometry)(const int* dims, int hlen, int levels, int* nr, int* nc);
    int (*state_table)(int levels, const int* depth, const int* idx, int n, unsigned char* out);  // validates a basis given as pairs
    int (*alloc_tables)(PacketTree&, wp_priv*);                         // after the depths: the device tables of the class
    int (*install)(PacketTree&, wp_priv*, const unsigned char* state);  // a valid state table: what the device needs of it
    int (*forward)(PacketTree&, wp_priv*);                              // PDWT_OK or the code of the entry that failed
    int (*inverse)(PacketTree&, wp_priv*);
    int (*depth_costs)(PacketTree&, int depth, int kind, double* out);  // the costs of a depth summed over the copies (node_costs of the class)
    int (*depth_stats)(PacketTree&, wp_priv*, int depth, long long n, w_band_stats* out);
    int (*depth_thresh)(PacketTree&, wp_priv*, int depth, int op, DTYPE beta, int do_thresh_appcoeffs);
};

namespace {
// ---- what the classes with a table of node pointers share (single image: copies = 1) -------------------------------------------
// the device table of node pointers (copies * arity^l pointers per depth, forest order)
int need_ptr_table(wp_priv* p, DTYPE* const* d_nodes)
{
    if (p->d_ptr) return PDWT_OK;
    p->d_ptr = (DTYPE**)pdwt_malloc(p->ptr_off[p->L + 1] * sizeof(DTYPE*));
    if (!p->d_ptr) return PDWT_ENOMEM;
    std::vector<DTYPE*> tab(p->ptr_off[p->L + 1]);
    for (int l = 0; l <= p->L; l++) {
        const size_t n = (size_t)p->copies * nnodes(p, l);
        for (size_t g = 0; g < n; g++) tab[p->ptr_off[l] + g] = d_nodes[l] + g * p->elems[l];
    }
    const int rc = pdwt_memcpy_h2d(p->d_ptr, tab.data(), tab.size() * sizeof(DTYPE*));
    if (rc != PDWT_OK) {
        pdwt_free(p->d_ptr);
        p->d_ptr = NULL;
    }
    return rc;
}

void ptr_offsets(wp_priv* p)
{
    p->ptr_off[0] = 0;
    for (int l = 0; l <= p->L; l++) p->ptr_off[l + 1] = p->ptr_off[l] + (size_t)p->copies * nnodes(p, l);
}

int stats_ptrs(PacketTree& W, wp_priv* p, int depth, long long n, w_band_stats* out)
{
    const int rc = need_ptr_table(p, W.d_nodes);
    if (rc != PDWT_OK) return rc;
    const size_t ne = (size_t)n;
    return SFX(pdwt_bandbatch_stats)(p->d_ptr + p->ptr_off[depth], &ne, p->copies * nnodes(p, depth), 1, NULL, reinterpret_cast<pdwt_band_stats*>(out));
}

int thresh_ptrs(PacketTree& W, wp_priv* p, int l, int op, DTYPE beta, int do_thresh_appcoeffs)
{
    if (const int rc = need_ptr_table(p, W.d_nodes); rc != PDWT_OK) return rc;
    const int nn = nnodes(p, l);
    std::vector<DTYPE> betas((size_t)p->copies * nn, (DTYPE)-1);  // (a negative beta leaves the node alone)
    for (int i = (do_thresh_appcoeffs ? 0 : 1); i < nn; i++)
        if (p->in_basis[l][i])
            for (int b = 0; b < p->copies; b++) betas[(size_t)b * nn + i] = beta;
    return SFX(pdwt_bandbatch_thresh)(op, p->d_ptr + p->ptr_off[l], &p->elems[l], betas.data(), p->copies * nn, 1);
}

int geometry2(const int* dims, int hlen, int levels, int* nr, int* nc) { return WaveletPackets::geometry(dims[1], dims[2], hlen, levels, nr, nc); }

// ---- the single image: one launch per depth; the inverse synthesises the parents above the basis, by the lists of them ---------
int alloc_tables2(PacketTree& W, wp_priv* p)
{
    ptr_offsets(p);
    if (const int rc = need_ptr_table(p, W.d_nodes); rc != PDWT_OK) return rc;
    p->d_lists = (int*)pdwt_malloc(p->ptr_off[p->L + 1] * sizeof(int));
    return p->d_lists ? PDWT_OK : PDWT_ENOMEM;
}

int install2(PacketTree&, wp_priv* p, const unsigned char* st)
{
    for (int l = p->L; l >= 0; l--) {
        p->parents[l].clear();
        for (int i = 0; i < nnodes(p, l); i++)
            if (st[toff(4, l) + i] == 2) p->parents[l].push_back(i);
        if (!p->parents[l].empty()) {
            const int rc = pdwt_memcpy_h2d(p->d_lists + p->ptr_off[l], p->parents[l].data(), p->parents[l].size() * sizeof(int));
            if (rc != PDWT_OK) return rc;
        }
    }
    return PDWT_OK;
}

int forward2(PacketTree& W, wp_priv* p)
{
    for (int l = 0; l < p->L; l++) {
        const int rc = SFX(pdwt_wpt2d_forward_level)(W.d_nodes[l], W.d_nodes[l + 1], p->nr[l], p->nc[l], NULL, nnodes(p, l), &p->f);
        if (rc != PDWT_OK) return rc;
    }
    return PDWT_OK;
}

int inverse2(PacketTree& W, wp_priv* p)
{
    for (int l = p->L - 1; l >= 0; l--) {
        const int n = (int)p->parents[l].size();
        if (!n) continue;
        const int* list = (n == nnodes(p, l)) ? NULL : p->d_lists + p->ptr_off[l];
        const int rc = SFX(pdwt_wpt2d_inverse_level)(W.d_nodes[l], W.d_nodes[l + 1], p->nr[l], p->nc[l], list, n, &p->f);
        if (rc != PDWT_OK) return rc;
    }
    return PDWT_OK;
}

int depth_costs2(PacketTree& W, int depth, int kind, double* out) { return static_cast<WaveletPackets&>(W).node_costs(depth, kind, out); }

// ---- the rows of a batch: the whole-transform entries choose between one launch and one per depth and say which ran (a positive
// value): only a negative one is an error.  Costs and statistics come from the moments of every (row, node) -------------------------
int geometry1(const int* dims, int hlen, int levels, int* nr, int* nc)
{
    const int L = pdwt_wp1_geometry(dims[2], hlen, levels, nc);
    for (int l = 0; l <= L; l++) nr[l] = dims[1];
    return L;
}

int alloc_tables1(PacketTree&, wp_priv* p)
{
    p->fused = pdwt_wp1_fused(p->Nc, p->f.hlen, p->L, (int)sizeof(DTYPE)) == 1;
    p->d_state = (unsigned char*)pdwt_malloc(state_bytes(2, p->L));
    p->d_thr = (unsigned char*)pdwt_malloc(state_bytes(2, p->L));
    return p->d_state && p->d_thr ? PDWT_OK : PDWT_ENOMEM;
}

int install1(PacketTree&, wp_priv* p, const unsigned char* st)
{
    const size_t nb = state_bytes(2, p->L);
    std::vector<unsigned char> thr(nb, 0);
    for (int l = 0; l <= p->L; l++)
        for (int i = 1; i < nnodes(p, l); i++) thr[toff(2, l) + i] = st[toff(2, l) + i] == 1;
    if (const int rc = pdwt_memcpy_h2d(p->d_state, st, nb); rc != PDWT_OK) return rc;
    return pdwt_memcpy_h2d(p->d_thr, thr.data(), nb);
}

int forward1(PacketTree& W, wp_priv* p)
{
    const int rc = SFX(pdwt_wp1_forward)(W.d_image, W.d_nodes + 1, p->Nr, p->Nc, p->L, &p->f);
    return rc < 0 ? rc : PDWT_OK;
}

int inverse1(PacketTree& W, wp_priv* p)
{
    if (p->in_basis[0][0]) return PDWT_OK;  // (the batch itself as the basis: nothing to synthesise)
    const int rc = SFX(pdwt_wp1_inverse)(W.d_image, W.d_nodes + 1, p->Nr, p->Nc, p->L, p->d_state, &p->f);
    return rc < 0 ? rc : PDWT_OK;
}

// the four moments of every (row, node) of a depth: 4 * Nr * 2^depth doubles, segment = row * 2^depth + node
int depth_moments(PacketTree& W, wp_priv* p, int depth, std::vector<double>& m)
{
    const long long nseg = (long long)p->Nr * nnodes(p, depth);
    m.resize(4 * (size_t)nseg);
    return SFX(pdwt_wp1_moments)(W.d_nodes[depth], nseg, p->nc[depth], m.data());
}

int depth_costs1(PacketTree& W, int depth, int kind, double* out) { return static_cast<WaveletPackets1D&>(W).node_costs(depth, kind, out); }

int stats1(PacketTree& W, wp_priv* p, int depth, long long n, w_band_stats* out)
{
    std::vector<double> m;
    const int rc = depth_moments(W, p, depth, m);
    if (rc != PDWT_OK) return rc;
    const int nn = nnodes(p, depth);
    for (int i = 0; i < nn; i++) out[i].n = (double)n, out[i].sum_abs = 0.0, out[i].sum_sq = 0.0, out[i].max_abs = 0.0, out[i].median_abs = NAN;
    for (int r = 0; r < p->Nr; r++)
        for (int i = 0; i < nn; i++) {
            const double* s = &m[4 * ((size_t)r * nn + i)];
            out[i].sum_abs += s[0], out[i].sum_sq += s[1];
            if (s[2] > out[i].max_abs) out[i].max_abs = s[2];
        }
    return PDWT_OK;
}

int thresh1(PacketTree& W, wp_priv* p, int l, int op, DTYPE beta, int do_thresh_appcoeffs)
{
    const unsigned char* flags = (do_thresh_appcoeffs ? p->d_state : p->d_thr) + toff(2, l);
    return SFX(pdwt_wp1_thresh)(op, W.d_nodes[l], p->Nr, nnodes(p, l), p->nc[l], flags, beta);
}

// ---- the images of a stack: whole-transform entries as 1-D, over the state table and, in the per-depth form, its chunk lists ---
int alloc_tables_b(PacketTree&, wp_priv* p)
{
    p->fused = p->allow_fused && pdwt_wptb_fused(p->Nr, p->Nc, p->f.hlen, p->L, (int)sizeof(DTYPE)) == 1;
    ptr_offsets(p);
    p->d_state = (unsigned char*)pdwt_malloc(state_bytes(4, p->L));
    const long long nl = pdwt_wptb_tmp_elems(p->copies, p->Nr, p->Nc, p->f.hlen, p->L, (int)sizeof(DTYPE), p->allow_fused);
    if (nl > 0) p->d_lists = (int*)pdwt_malloc((size_t)nl * sizeof(int));
    if (!p->d_state || nl < 0 || (nl > 0 && !p->d_lists)) return nl < 0 ? PDWT_EINVAL : PDWT_ENOMEM;
    return PDWT_OK;
}

int install_b(PacketTree&, wp_priv* p, const unsigned char* st)
{
    int rc = pdwt_memcpy_h2d(p->d_state, st, state_bytes(4, p->L));
    if (rc != PDWT_OK) return rc;
    if (p->d_lists && st[0] == 2) {
        const long long n = pdwt_wptb_chunk_lists(p->copies, p->L, st, NULL);
        if (n < 0) return (int)n;
        std::vector<int> lists((size_t)n, 0);
        pdwt_wptb_chunk_lists(p->copies, p->L, st, lists.data());
        rc = pdwt_memcpy_h2d(p->d_lists, lists.data(), lists.size() * sizeof(int));
    }
    return rc;
}

int forward_b(PacketTree& W, wp_priv* p)
{
    const int rc = SFX(pdwt_wptb_forward)(W.d_image, W.d_nodes + 1, p->copies, p->Nr, p->Nc, p->L, &p->f, p->allow_fused);
    return rc < 0 ? rc : PDWT_OK;
}

int inverse_b(PacketTree& W, wp_priv* p)
{
    if (p->state[0] != 2) return PDWT_OK;  // (a basis of the root alone: the images are the coefficients)
    const int rc = SFX(pdwt_wptb_inverse)(W.d_image, W.d_nodes + 1, p->copies, p->Nr, p->Nc, p->L, p->state.data(), p->d_state, p->d_lists, &p->f, p->allow_fused);
    return rc < 0 ? rc : PDWT_OK;
}

int depth_costs_b(PacketTree& W, int depth, int kind, double* out) { return static_cast<WaveletPacketsImages&>(W).node_costs(depth, kind, NULL, out); }

const wp_ops kOps2 = {"WaveletPackets", 4, "image", false, false, 0, 0, "a %dx%d image", "is too small",
                      geometry2, pdwt_wptb_state_table, alloc_tables2, install2, forward2, inverse2, depth_costs2, stats_ptrs, thresh_ptrs};
const wp_ops kOps1 = {"WaveletPackets1D", 2, "batch", true, true, 0, 0, "rows of %d samples", "are too short",
                      geometry1, pdwt_wp1_state_table, alloc_tables1, install1, forward1, inverse1, depth_costs1, stats1, thresh1};
const wp_ops kOpsB = {"WaveletPacketsImages", 4, "image", false, true, 65535, 1ll << 22, "a %dx%d image", "is too small",
                      geometry2, pdwt_wptb_state_table, alloc_tables_b, install_b, forward_b, inverse_b, depth_costs_b, stats_ptrs, thresh_ptrs};

// install a valid state table: on the device, then the flags and the table on the host
int install_state(PacketTree& W, const wp_ops& o, wp_priv* p, std::vector<unsigned char>& st)
{
    if (const int rc = o.install(W, p, st.data()); rc != PDWT_OK) return rc;
    for (int l = 0; l <= p->L; l++) {
        p->in_basis[l].assign((size_t)nnodes(p, l), 0);
        for (int i = 0; i < nnodes(p, l); i++) p->in_basis[l][i] = st[toff(o.arity, l) + i] == 1;
    }
    p->state.swap(st);
    return PDWT_OK;
}

// install a basis given as pairs; PDWT_EINVAL unless they partition the tree
int install_pairs(PacketTree& W, const wp_ops& o, wp_priv* p, const int* depth, const int* idx, int n)
{
    std::vector<unsigned char> st(state_bytes(o.arity, p->L));
    if (o.state_table(p->L, depth, idx, n, st.data()) != PDWT_OK) return PDWT_EINVAL;
    return install_state(W, o, p, st);
}

// index of the node a path over `letters` (one per child, in child order) names, its depth in *depth; -1 for a bad letter or a path deeper than max_levels
int path_index_of(const char* letters, int max_levels, const char* path, int* depth)
{
    if (!path) return -1;
    const int arity = (int)strlen(letters);
    int i = 0, d = 0;
    for (; path[d]; d++) {
        const char* q = strchr(letters, path[d]);
        if (d >= max_levels || !q) return -1;
        i = arity * i + (int)(q - letters);
    }
    if (depth) *depth = d;
    return i;
}
}  // namespace
#define ON_MY_DEVICE_W() DevScope dev_scope_(priv_ ? ((const wp_priv*)priv_)->dev : -1)

// ---- the static functions of each class -------------------------------------------------------------------------------------------
int WaveletPackets::geometry(int Nr, int Nc, int hlen, int levels, int* nr, int* nc)
{
    if (Nr < 1 || Nc < 1 || hlen < 2 || (unsigned long long)Nr * (unsigned long long)Nc >= (1ull << 31)) return 0;
    if (levels < 1) levels = 1;
    int wmaxlev = w_ilog2((Nr < Nc ? Nr : Nc) / (hlen - 1));  // the rule of Wavelets (src/wt.cu:155-165)
    if (wmaxlev > WPT_MAX_LEVELS) wmaxlev = WPT_MAX_LEVELS;
    if (levels > wmaxlev) levels = wmaxlev;
    for (int l = 0; l <= levels; l++) {
        if (nr) nr[l] = Nr;
        if (nc) nc[l] = Nc;
        Nr = (Nr + 1) >> 1, Nc = (Nc + 1) >> 1;
    }
    return levels;
}
int WaveletPackets::path_index(const char* path, int* depth) { return path_index_of("ahvd", WPT_MAX_LEVELS, path, depth); }

int WaveletPackets1D::geometry(int Nc, int hlen, int levels, int* n) { return pdwt_wp1_geometry(Nc, hlen, levels, n); }
int WaveletPackets1D::path_index(const char* path, int* depth) { return path_index_of("ad", WPT1D_MAX_LEVELS, path, depth); }
int WaveletPackets1D::frequency_order(int depth, int* out) { return pdwt_wp1_frequency_order(depth, out) == PDWT_OK ? 1 << depth : 0; }

int WaveletPacketsImages::geometry(int Nr, int Nc, int hlen, int levels, int* nr, int* nc) { return WaveletPackets::geometry(Nr, Nc, hlen, levels, nr, nc); }
int WaveletPacketsImages::path_index(const char* path, int* depth) { return WaveletPackets::path_index(path, depth); }

// ---- construction ------------------------------------------------------------------------------------------------------------------
PacketTree::PacketTree() : d_image(NULL), state(W_INIT), ops_(NULL), priv_(NULL)
{
    for (int l = 0; l <= kL; l++) d_nodes[l] = NULL;
    wname[0] = 0;
}

void PacketTree::create(const wp_ops& o, DTYPE* src, const int* dims, const char* wname_, int memisonhost, int allow_fused, int* nlevels, int* hlen_out)
{
    ops_ = &o;
    const int B = dims[0], Nr = dims[1], Nc = dims[2];
    strncpy(wname, wname_ ? wname_ : "", 127);
    wname[127] = 0;
    state = W_CREATION_ERROR;  // until the last line
    if (Nr < 1 || Nc < 1 || !wname_ || (unsigned long long)Nr * (unsigned long long)Nc >= (1ull << 31)) {
        printf("ERROR: %s(): invalid %s size or wavelet name\n", o.name, o.noun);
        return;
    }
    if (o.max_copies && (B < 1 || B > o.max_copies)) {
        printf("ERROR: %s(): a batch holds 1 .. %d images (%d given)\n", o.name, o.max_copies, B);
        return;
    }
    if (*nlevels < 1) {
        puts("Warning: cannot initialize wavelet coefficients with nlevels < 1. Forcing nlevels = 1");
        *nlevels = 1;
    }
    wp_priv* p = new (std::nothrow) wp_priv();
    if (!p) return;
    priv_ = p;
    p->dev = -1;
    p->arity = o.arity, p->copies = o.rows_are_copies ? Nr : B, p->Nr = Nr, p->Nc = Nc, p->allow_fused = allow_fused ? 1 : 0;
    const int hlen = SFX(pdwt_compute_filters_separable)(wname, 0, &p->f);
    if (hlen <= 0) {
        printf("ERROR: unknown wavelet name %s\n", wname);
        return;
    }
    p->f.hlen = hlen;
    *hlen_out = hlen;
    const int wmaxlev = o.geometry(dims, hlen, *nlevels, p->nr, p->nc);
    char what[64];  // "a 24x26 image" / "rows of 48 samples" (a format with one %d leaves the second size alone)
    if (o.rows_are_copies) snprintf(what, sizeof(what), o.size_fmt, Nc);
    else snprintf(what, sizeof(what), o.size_fmt, Nr, Nc);
    if (*nlevels > wmaxlev) {
        printf("Warning: required level (%d) is greater than the maximum possible level for %s packets (%d) on %s.\n", *nlevels, wname, wmaxlev, what);
        printf("Forcing nlevels = %d\n", wmaxlev);
        *nlevels = wmaxlev;
    }
    if (*nlevels < 1) {
        printf("ERROR: %s %s for one level of %s\n", what, o.too_small, wname);
        return;
    }
    const int L = p->L = *nlevels;
    if (o.max_forest && (long long)B * nnodes(p, L) > o.max_forest) {
        printf("ERROR: %s(): %d images of %d nodes exceed 2^22 nodes per depth\n", o.name, B, nnodes(p, L));
        return;
    }
    for (int l = 0; l <= L; l++) p->elems[l] = o.rows_are_copies ? (size_t)p->nc[l] : (size_t)p->nr[l] * p->nc[l];
    // every argument is accepted: from here on the instance belongs to the current device (a failed one has none, and its methods touch none)
    p->dev = pdwt_get_device();
    int rc = PDWT_OK;
    for (int l = 0; l <= L && rc == PDWT_OK; l++) {
        const size_t nb = (size_t)p->copies * nnodes(p, l) * p->elems[l] * sizeof(DTYPE);
        d_nodes[l] = (DTYPE*)pdwt_malloc(nb);
        if (!d_nodes[l]) rc = PDWT_ENOMEM;
        else if (l > 0) rc = pdwt_memset(d_nodes[l], 0, nb);
    }
    d_image = d_nodes[0];
    if (rc == PDWT_OK) rc = o.alloc_tables(*this, p);
    if (rc == PDWT_OK) {  // the default basis: every node of depth L
        std::vector<int> d((size_t)nnodes(p, L), L), i((size_t)nnodes(p, L));
        for (int k = 0; k < nnodes(p, L); k++) i[k] = k;
        rc = install_pairs(*this, o, p, d.data(), i.data(), nnodes(p, L));
    }
    if (rc == PDWT_OK) {
        const size_t n = (size_t)p->copies * p->elems[0];
        if (!src) rc = pdwt_memset(d_image, 0, n * sizeof(DTYPE));
        else if (memisonhost) rc = pdwt_memcpy_h2d(d_image, src, n * sizeof(DTYPE));
        else rc = pdwt_memcpy_d2d_foreign(d_image, src, n * sizeof(DTYPE));
    }
    if (rc != PDWT_OK) {
        report(o.name, "(): allocation or upload", rc);
        return;
    }
    state = W_INIT;
}

PacketTree::~PacketTree()
{
    ON_MY_DEVICE_W();
    for (int l = 0; l <= kL; l++)
        if (d_nodes[l]) pdwt_free(d_nodes[l]);
    if (priv_) {
        wp_priv* p = P(priv_);
        if (p->d_ptr) pdwt_free(p->d_ptr);
        if (p->d_lists) pdwt_free(p->d_lists);
        if (p->d_state) pdwt_free(p->d_state);
        if (p->d_thr) pdwt_free(p->d_thr);
        delete p;
    }
}

WaveletPackets::WaveletPackets(DTYPE* img, int Nr, int Nc, const char* wname_, int levels, int memisonhost)
{
    const int dims[3] = {1, Nr, Nc};
    winfos.Nr = Nr, winfos.Nc = Nc, winfos.nlevels = levels, winfos.hlen = 0;
    create(kOps2, img, dims, wname_, memisonhost, 0, &winfos.nlevels, &winfos.hlen);
}

WaveletPackets1D::WaveletPackets1D(DTYPE* rows, int Nr, int Nc, const char* wname_, int levels, int memisonhost)
{
    const int dims[3] = {1, Nr, Nc};
    winfos.Nr = Nr, winfos.Nc = Nc, winfos.nlevels = levels, winfos.hlen = 0;
    create(kOps1, rows, dims, wname_, memisonhost, 1, &winfos.nlevels, &winfos.hlen);
}

WaveletPacketsImages::WaveletPacketsImages(DTYPE* imgs, int B, int Nr, int Nc, const char* wname_, int levels, int memisonhost, int allow_fused)
{
    const int dims[3] = {B, Nr, Nc};
    winfos.B = B, winfos.Nr = Nr, winfos.Nc = Nc, winfos.nlevels = levels, winfos.hlen = 0;
    create(kOpsB, imgs, dims, wname_, memisonhost, allow_fused, &winfos.nlevels, &winfos.hlen);
}

int PacketTree::tree_fused() const { return state != W_CREATION_ERROR && priv_ ? P(priv_)->fused : 0; }

// ---- transforms ----------------------------------------------------------------------------------------------------------------------
void PacketTree::forward()
{
    ON_MY_DEVICE_W();
    if (state == W_CREATION_ERROR) {
        puts("Warning: forward transform not computed, as there was an error when creating the wavelets");
        return;
    }
    const int rc = ops_->forward(*this, P(priv_));
    if (rc != PDWT_OK) {
        report(ops_->name, "::forward()", rc);
        state = W_FORWARD_ERROR;
        return;
    }
    state = W_FORWARD;
}

void PacketTree::inverse()
{
    ON_MY_DEVICE_W();
    if (state == W_INVERSE) {
        puts("Warning: W.inverse() has already been run. Inverse is available in W.get_image()");
        return;
    }
    if (state == W_CREATION_ERROR || state == W_FORWARD_ERROR || state == W_THRESHOLD_ERROR) {
        puts("Warning: inverse transform not computed, as there was an error in a previous stage");
        return;
    }
    const int rc = ops_->inverse(*this, P(priv_));
    if (rc != PDWT_OK) {
        report(ops_->name, "::inverse()", rc);
        state = W_INVERSE_ERROR;
        return;
    }
    state = W_INVERSE;
}

// ---- data in and out -----------------------------------------------------------------------------------------------------------------
long long PacketTree::tree_get_image(DTYPE* res)
{
    ON_MY_DEVICE_W();
    if (!d_image || !res || state == W_CREATION_ERROR) return 0;
    const wp_priv* p = P(priv_);
    const size_t n = (size_t)p->copies * p->elems[0];
    if (pdwt_memcpy_d2h(res, d_image, n * sizeof(DTYPE)) != PDWT_OK) return 0;
    return (long long)n;
}

void PacketTree::set_image(DTYPE* img, int mem_is_on_device)
{
    ON_MY_DEVICE_W();
    if (!d_image || !img || state == W_CREATION_ERROR) return;
    const wp_priv* p = P(priv_);
    const size_t nb = (size_t)p->copies * p->elems[0] * sizeof(DTYPE);
    const int rc = mem_is_on_device ? pdwt_memcpy_d2d_foreign(d_image, img, nb) : pdwt_memcpy_h2d(d_image, img, nb);
    if (rc != PDWT_OK) report(ops_->name, "::set_image()", rc);
    state = W_INIT;
}

long long PacketTree::node_shape(int depth, int* nr, int* nc) const
{
    if (state == W_CREATION_ERROR || depth < 0 || depth > P(priv_)->L) return 0;
    const wp_priv* p = P(priv_);
    if (nr) *nr = p->nr[depth];
    if (nc) *nc = p->nc[depth];
    return (long long)p->nr[depth] * p->nc[depth];
}

// device address of node idx of the first copy; the same node of consecutive copies is *pitch ELEMENTS apart
intptr_t PacketTree::tree_node_ptr(int depth, int idx, long long* pitch)
{
    if (node_shape(depth, NULL, NULL) <= 0 || idx < 0 || idx >= nnodes(P(priv_), depth)) return 0;
    const wp_priv* p = P(priv_);
    if (pitch) *pitch = (long long)nnodes(p, depth) * (long long)p->elems[depth];
    return (intptr_t)(d_nodes[depth] + (size_t)idx * p->elems[depth]);
}

// a node of every copy, dense on the host: one plain copy (single image) or a pitched one
long long PacketTree::tree_get_node(DTYPE* out, int depth, int idx)
{
    ON_MY_DEVICE_W();
    if (state == W_INVERSE) {
        puts("Warning: get_node(): inverse() has been performed, the coefficients has been modified and do not make sense anymore.");
        return 0;
    }
    long long pitch = 0;
    const intptr_t src = tree_node_ptr(depth, idx, &pitch);
    if (!src || !out) return 0;
    const wp_priv* p = P(priv_);
    const size_t w = p->elems[depth] * sizeof(DTYPE);
    const int rc = ops_->pitched ? pdwt_memcpy2d(out, w, (const void*)src, (size_t)pitch * sizeof(DTYPE), w, (size_t)p->copies, 1) : pdwt_memcpy_d2h(out, (const void*)src, w);
    if (rc != PDWT_OK) return 0;
    return (long long)p->copies * (long long)p->elems[depth];
}

long long PacketTree::get_level(DTYPE* out, int depth)
{
    ON_MY_DEVICE_W();
    if (state == W_INVERSE) {
        puts("Warning: get_level(): inverse() has been performed, the coefficients has been modified and do not make sense anymore.");
        return 0;
    }
    if (node_shape(depth, NULL, NULL) <= 0 || !out) return 0;
    const wp_priv* p = P(priv_);
    const long long n = (long long)p->copies * nnodes(p, depth) * (long long)p->elems[depth];
    if (pdwt_memcpy_d2h(out, d_nodes[depth], (size_t)n * sizeof(DTYPE)) != PDWT_OK) return 0;
    return n;
}

long long PacketTree::tree_set_node(DTYPE* in, int depth, int idx, int mem_is_on_device)
{
    ON_MY_DEVICE_W();
    if (!(state == W_FORWARD || state == W_THRESHOLD)) {
        puts("Warning: set_node(): refused, the tree does not hold the coefficients of a forward() (run forward() first)");
        return 0;
    }
    long long pitch = 0;
    const intptr_t dst = tree_node_ptr(depth, idx, &pitch);
    if (!dst || !in) return 0;
    const wp_priv* p = P(priv_);
    const size_t w = p->elems[depth] * sizeof(DTYPE);
    int rc;
    if (ops_->pitched) rc = pdwt_memcpy2d((void*)dst, (size_t)pitch * sizeof(DTYPE), in, w, w, (size_t)p->copies, mem_is_on_device ? 3 : 0);
    else rc = mem_is_on_device ? pdwt_memcpy_d2d_foreign((void*)dst, in, w) : pdwt_memcpy_h2d((void*)dst, in, w);
    if (rc != PDWT_OK) {
        report(ops_->name, "::set_node()", rc);
        return 0;
    }
    state = W_THRESHOLD;
    return (long long)p->copies * (long long)p->elems[depth];
}

// ---- costs ------------------------------------------------------------------------------------------------------------------------------
int WaveletPackets::node_costs(int depth, int kind, double* out)
{
    ON_MY_DEVICE_W();
    const long long n = node_shape(depth, NULL, NULL);
    if (!(state == W_FORWARD || state == W_THRESHOLD) || n <= 0 || !out) return PDWT_EINVAL;
    const int rc = SFX(pdwt_wpt2d_node_cost)(d_nodes[depth], (size_t)n, nnodes(4, depth), kind, out);
    if (rc != PDWT_OK) report("WaveletPackets", "::node_costs()", rc);
    return rc;
}

int WaveletPackets1D::node_costs(int depth, int kind, double* out, double* per_row)
{
    ON_MY_DEVICE_W();
    if (!(state == W_FORWARD || state == W_THRESHOLD) || node_shape(depth, NULL, NULL) <= 0 || !out || (kind != 0 && kind != 1)) return PDWT_EINVAL;
    std::vector<double> m;
    const int rc = depth_moments(*this, P(priv_), depth, m);
    if (rc != PDWT_OK) {
        report("WaveletPackets1D", "::node_costs()", rc);
        return rc;
    }
    const int nn = nnodes(2, depth), col = kind == 0 ? 0 : 3;
    for (int i = 0; i < nn; i++) out[i] = 0.0;
    for (int r = 0; r < winfos.Nr; r++)  // over the rows in row order
        for (int i = 0; i < nn; i++) {
            const double c = m[4 * ((size_t)r * nn + i) + col];
            out[i] += c;
            if (per_row) per_row[(size_t)r * nn + i] = c;
        }
    return PDWT_OK;
}

int WaveletPacketsImages::node_costs(int depth, int kind, double* per_image, double* summed)
{
    ON_MY_DEVICE_W();
    const long long n = node_shape(depth, NULL, NULL);
    if (!(state == W_FORWARD || state == W_THRESHOLD) || n <= 0 || (!per_image && !summed)) return PDWT_EINVAL;
    const int nn = nnodes(4, depth);
    const size_t total = (size_t)winfos.B * nn;
    std::vector<double> own;
    if (!per_image) own.resize(total), per_image = own.data();
    for (size_t g0 = 0; g0 < total; g0 += kCostChunk) {
        const int cnt = (int)(total - g0 < (size_t)kCostChunk ? total - g0 : (size_t)kCostChunk);
        const int rc = SFX(pdwt_wpt2d_node_cost)(d_nodes[depth] + g0 * (size_t)n, (size_t)n, cnt, kind, per_image + g0);
        if (rc != PDWT_OK) {
            report("WaveletPacketsImages", "::node_costs()", rc);
            return rc;
        }
    }
    if (summed)
        for (int i = 0; i < nn; i++) {
            double s = 0.0;
            for (int b = 0; b < winfos.B; b++) s += per_image[(size_t)b * nn + i];  // image order: two runs give the same bits
            summed[i] = s;
        }
    return PDWT_OK;
}

// ---- the basis ------------------------------------------------------------------------------------------------------------------------
// Coifman-Wickerhauser: bottom-up, a parent is kept when its cost is <= the sum of its children's best costs (summed left to right)
int PacketTree::best_basis(int kind)
{
    ON_MY_DEVICE_W();
    if (state != W_FORWARD || (kind != 0 && kind != 1)) return PDWT_EINVAL;
    wp_priv* p = P(priv_);
    const int L = p->L, a = p->arity;
    std::vector<double> best[kL + 1];
    std::vector<unsigned char> keep[kL + 1], flags[kL + 1];
    for (int l = 0; l <= L; l++) {
        best[l].resize((size_t)nnodes(p, l));
        if (const int rc = ops_->depth_costs(*this, l, kind, best[l].data()); rc != PDWT_OK) return rc;
        keep[l].assign((size_t)nnodes(p, l), 1);
        flags[l].assign((size_t)nnodes(p, l), 0);
    }
    for (int l = L - 1; l >= 0; l--)
        for (int i = 0; i < nnodes(p, l); i++) {
            const double* c = &best[l + 1][(size_t)a * i];
            double below = c[0];
            for (int q = 1; q < a; q++) below += c[q];
            if (!(best[l][i] <= below)) keep[l][i] = 0, best[l][i] = below;
        }
    flags[0][0] = 1;  // top-down: a node that is not kept hands over to its children
    std::vector<int> bd, bi;
    for (int l = 0; l <= L; l++)
        for (int i = 0; i < nnodes(p, l); i++) {
            if (!flags[l][i]) continue;
            if (keep[l][i]) bd.push_back(l), bi.push_back(i);  // (depth L keeps all)
            else
                for (int q = 0; q < a; q++) flags[l + 1][a * i + q] = 1;
        }
    if (const int rc = install_pairs(*this, *ops_, p, bd.data(), bi.data(), (int)bd.size()); rc != PDWT_OK) return rc;
    return basis_size();
}

int PacketTree::set_basis(const int* depth, const int* idx, int n)
{
    ON_MY_DEVICE_W();
    if (state == W_CREATION_ERROR || state == W_THRESHOLD || state == W_THRESHOLD_ERROR) return PDWT_EINVAL;
    return install_pairs(*this, *ops_, P(priv_), depth, idx, n);
}

int PacketTree::basis_size() const { return get_basis(NULL, NULL); }

int PacketTree::get_basis(int* depth, int* idx) const
{
    if (state == W_CREATION_ERROR) return 0;
    const wp_priv* p = P(priv_);
    int n = 0;
    for (int l = 0; l <= p->L; l++)
        for (int i = 0; i < nnodes(p, l); i++)
            if (p->in_basis[l][i]) {
                if (depth) depth[n] = l;
                if (idx) idx[n] = i;
                n++;
            }
    return n;
}

// ---- thresholds, norms, statistics over the basis ------------------------------------------------------------------------------------
void PacketTree::threshold(int op, DTYPE beta, int do_thresh_appcoeffs)
{
    ON_MY_DEVICE_W();
    if (state == W_INVERSE) {
        printf("Warning: %s(): cannot threshold coefficients, as they were modified by W.inverse()\n", ops_->name);
        return;
    }
    if (state == W_CREATION_ERROR) return;
    wp_priv* p = P(priv_);
    int rc = PDWT_OK;
    for (int l = 0; l <= p->L && rc == PDWT_OK; l++) {
        int any = 0;
        for (int i = (do_thresh_appcoeffs ? 0 : 1); i < nnodes(p, l) && !any; i++) any = p->in_basis[l][i];  // node 0 of every depth is the all-"a" path
        if (any) rc = ops_->depth_thresh(*this, p, l, op, beta, do_thresh_appcoeffs);
    }
    if (rc != PDWT_OK) {
        report(ops_->name, op ? "::hard_threshold()" : "::soft_threshold()", rc);
        state = W_THRESHOLD_ERROR;
        return;
    }
    state = W_THRESHOLD;
}
void PacketTree::soft_threshold(DTYPE beta, int do_thresh_appcoeffs) { threshold(0, beta, do_thresh_appcoeffs); }
void PacketTree::hard_threshold(DTYPE beta, int do_thresh_appcoeffs) { threshold(1, beta, do_thresh_appcoeffs); }

double PacketTree::tree_norm1()
{
    ON_MY_DEVICE_W();
    if (!(state == W_FORWARD || state == W_THRESHOLD)) return -1.0;
    wp_priv* p = P(priv_);
    std::vector<double> c;
    double sum = 0.0;
    for (int l = 0; l <= p->L; l++) {
        int any = 0;
        for (int i = 0; i < nnodes(p, l) && !any; i++) any = p->in_basis[l][i];
        if (!any) continue;
        c.resize((size_t)nnodes(p, l));
        if (ops_->depth_costs(*this, l, 0, c.data()) != PDWT_OK) return -1.0;
        for (int i = 0; i < nnodes(p, l); i++)
            if (p->in_basis[l][i]) sum += c[i];
    }
    return sum;
}

// per image over the depths and the nodes of the basis
int WaveletPacketsImages::images_norm1(double* out)
{
    ON_MY_DEVICE_W();
    if (!(state == W_FORWARD || state == W_THRESHOLD) || !out) return PDWT_EINVAL;
    wp_priv* p = P(priv_);
    std::vector<double> c;
    for (int b = 0; b < p->copies; b++) out[b] = 0.0;
    for (int l = 0; l <= p->L; l++) {
        const int nn = nnodes(p, l);
        int any = 0;
        for (int i = 0; i < nn && !any; i++) any = p->in_basis[l][i];
        if (!any) continue;
        c.resize((size_t)p->copies * nn);
        if (const int rc = node_costs(l, 0, c.data(), NULL); rc != PDWT_OK) return rc;
        for (int b = 0; b < p->copies; b++)
            for (int i = 0; i < nn; i++)
                if (p->in_basis[l][i]) out[b] += c[(size_t)b * nn + i];
    }
    return PDWT_OK;
}

// (not tree_norm1: the sum of the per-image sums, in image order)
double WaveletPacketsImages::norm1()
{
    if (!(state == W_FORWARD || state == W_THRESHOLD)) return -1.0;
    std::vector<double> per((size_t)winfos.B);
    if (images_norm1(per.data()) != PDWT_OK) return -1.0;
    double sum = 0.0;
    for (int b = 0; b < winfos.B; b++) sum += per[b];
    return sum;
}

int PacketTree::node_stats(int depth, w_band_stats* out)
{
    ON_MY_DEVICE_W();
    const long long n = node_shape(depth, NULL, NULL);
    if (!(state == W_FORWARD || state == W_THRESHOLD) || n <= 0 || !out) return PDWT_EINVAL;
    const int rc = ops_->depth_stats(*this, P(priv_), depth, n, out);
    if (rc != PDWT_OK) report(ops_->name, "::node_stats()", rc);
    return rc;
}

// the median of node "d" (the last node of depth 1) over all copies: contiguous in the single image, else gathered into one run by a
// pitched device-to-device copy
double PacketTree::estimate_sigma()
{
    ON_MY_DEVICE_W();
    if (!(state == W_FORWARD || state == W_THRESHOLD)) return -1.0;
    wp_priv* p = P(priv_);
    const size_t n = p->elems[1], w = n * sizeof(DTYPE), all = n * p->copies;
    const DTYPE* d = d_nodes[1] + (size_t)(p->arity - 1) * n;
    const unsigned char want = 2;  // the median alone
    pdwt_band_stats s;
    int rc, rf = PDWT_OK;
    if (!ops_->pitched) rc = SFX(pdwt_bandlist_stats)(&d, &n, 1, &want, &s);
    else {
        DTYPE* pool = (DTYPE*)pdwt_malloc(all * sizeof(DTYPE));
        if (!pool) return -1.0;
        rc = pdwt_memcpy2d(pool, w, d, p->arity * w, w, (size_t)p->copies, 2);
        const DTYPE* cp = pool;
        if (rc == PDWT_OK) rc = SFX(pdwt_bandlist_stats)(&cp, &all, 1, &want, &s);  // (synchronises)
        rf = pdwt_free(pool);
    }
    if (rc != PDWT_OK || rf != PDWT_OK) {
        report(ops_->name, "::estimate_sigma()", rc != PDWT_OK ? rc : rf);
        return -1.0;
    }
    return s.median_abs / 0.6744897501960817;
}

int WaveletPacketsImages::images_estimate_sigma(double* out)
{
    ON_MY_DEVICE_W();
    if (!(state == W_FORWARD || state == W_THRESHOLD) || !out) return PDWT_EINVAL;
    wp_priv* p = P(priv_);
    const size_t n = p->elems[1];
    std::vector<DTYPE*> tab((size_t)p->copies);
    for (int b = 0; b < p->copies; b++) tab[b] = d_nodes[1] + ((size_t)4 * b + 3) * n;  // node "d" of image b
    DTYPE** d_tab = (DTYPE**)pdwt_malloc(tab.size() * sizeof(DTYPE*));
    if (!d_tab) return PDWT_ENOMEM;
    std::vector<pdwt_band_stats> s((size_t)p->copies);
    const unsigned char want = 2;
    int rc = pdwt_memcpy_h2d(d_tab, tab.data(), tab.size() * sizeof(DTYPE*));
    if (rc == PDWT_OK) rc = SFX(pdwt_bandbatch_stats)(d_tab, &n, p->copies, 1, &want, s.data());  // (synchronises)
    const int rf = pdwt_free(d_tab);
    if (rc != PDWT_OK || rf != PDWT_OK) {
        report("WaveletPacketsImages", "::images_estimate_sigma()", rc != PDWT_OK ? rc : rf);
        return rc != PDWT_OK ? rc : rf;
    }
    for (int b = 0; b < p->copies; b++) out[b] = s[b].median_abs / 0.6744897501960817;
    return PDWT_OK;
}

// ---- flat C handle APIs (pdwt_amd/wpt.py): the same functions under three prefixes; the functions whose arguments or return types are
// those of their class are written out below --------------------------------------------------------------------------------------
#define WP_HANDLE_API(pfx, Cls)                                                                                                                \
    void pfx##delete(void* h) { delete static_cast<Cls*>(h); }                                                                                 \
    void pfx##forward(void* h) { static_cast<Cls*>(h)->forward(); }                                                                            \
    void pfx##inverse(void* h) { static_cast<Cls*>(h)->inverse(); }                                                                            \
    void pfx##set_image(void* h, DTYPE* img, int mem_is_on_device) { static_cast<Cls*>(h)->set_image(img, mem_is_on_device); }                 \
    int pfx##state(void* h) { return (int)static_cast<Cls*>(h)->state; }                                                                       \
    long long pfx##node_shape(void* h, int depth, int* nr, int* nc) { return static_cast<Cls*>(h)->node_shape(depth, nr, nc); }                \
    long long pfx##get_level(void* h, DTYPE* out, int depth) { return static_cast<Cls*>(h)->get_level(out, depth); }                           \
    int pfx##best_basis(void* h, int kind) { return static_cast<Cls*>(h)->best_basis(kind); }                                                  \
    int pfx##set_basis(void* h, const int* depth, const int* idx, int n) { return static_cast<Cls*>(h)->set_basis(depth, idx, n); }            \
    int pfx##basis_size(void* h) { return static_cast<Cls*>(h)->basis_size(); }                                                                \
    int pfx##get_basis(void* h, int* depth, int* idx) { return static_cast<Cls*>(h)->get_basis(depth, idx); }                                  \
    void pfx##soft_threshold(void* h, DTYPE beta, int app) { static_cast<Cls*>(h)->soft_threshold(beta, app); }                                \
    void pfx##hard_threshold(void* h, DTYPE beta, int app) { static_cast<Cls*>(h)->hard_threshold(beta, app); }                                \
    double pfx##norm1(void* h) { return static_cast<Cls*>(h)->norm1(); }                                                                       \
    int pfx##node_stats(void* h, int depth, w_band_stats* out) { return static_cast<Cls*>(h)->node_stats(depth, out); }                        \
    double pfx##estimate_sigma(void* h) { return static_cast<Cls*>(h)->estimate_sigma(); }

#define WP(h) static_cast<WaveletPackets*>(h)
#define W1(h) static_cast<WaveletPackets1D*>(h)
#define WB(h) static_cast<WaveletPacketsImages*>(h)
extern "C" {
WP_HANDLE_API(pdwt_wpt_, WaveletPackets)
WP_HANDLE_API(pdwt_wp1h_, WaveletPackets1D)
WP_HANDLE_API(pdwt_wpbh_, WaveletPacketsImages)

void* pdwt_wpt_new(DTYPE* img, int Nr, int Nc, const char* wname, int levels, int memisonhost) { return new (std::nothrow) WaveletPackets(img, Nr, Nc, wname, levels, memisonhost); }
void pdwt_wpt_info(void* h, w_info_wpt* out) { *out = WP(h)->winfos; }
int pdwt_wpt_geometry(int Nr, int Nc, int hlen, int levels, int* nr, int* nc) { return WaveletPackets::geometry(Nr, Nc, hlen, levels, nr, nc); }
int pdwt_wpt_path_index(const char* path, int* depth) { return WaveletPackets::path_index(path, depth); }
int pdwt_wpt_get_image(void* h, DTYPE* out) { return WP(h)->get_image(out); }
int pdwt_wpt_get_node(void* h, DTYPE* out, int depth, int idx) { return WP(h)->get_node(out, depth, idx); }
int pdwt_wpt_set_node(void* h, DTYPE* in, int depth, int idx, int mem_is_on_device) { return WP(h)->set_node(in, depth, idx, mem_is_on_device); }
intptr_t pdwt_wpt_node_int_ptr(void* h, int depth, int idx) { return WP(h)->node_int_ptr(depth, idx); }
int pdwt_wpt_node_costs(void* h, int depth, int kind, double* out) { return WP(h)->node_costs(depth, kind, out); }

void* pdwt_wp1h_new(DTYPE* rows, int Nr, int Nc, const char* wname, int levels, int memisonhost) { return new (std::nothrow) WaveletPackets1D(rows, Nr, Nc, wname, levels, memisonhost); }
void pdwt_wp1h_info(void* h, w_info_wpt1* out) { *out = W1(h)->winfos; }
int pdwt_wp1h_geometry(int Nc, int hlen, int levels, int* n) { return WaveletPackets1D::geometry(Nc, hlen, levels, n); }
int pdwt_wp1h_path_index(const char* path, int* depth) { return WaveletPackets1D::path_index(path, depth); }
int pdwt_wp1h_frequency_order(int depth, int* out) { return WaveletPackets1D::frequency_order(depth, out); }
int pdwt_wp1h_fused(void* h) { return W1(h)->fused(); }
int pdwt_wp1h_get_image(void* h, DTYPE* out) { return W1(h)->get_image(out); }
int pdwt_wp1h_get_node(void* h, DTYPE* out, int depth, int idx) { return W1(h)->get_node(out, depth, idx); }
int pdwt_wp1h_set_node(void* h, DTYPE* in, int depth, int idx, int mem_is_on_device) { return W1(h)->set_node(in, depth, idx, mem_is_on_device); }
intptr_t pdwt_wp1h_node_int_ptr(void* h, int depth, int idx, long long* pitch) { return W1(h)->node_int_ptr(depth, idx, pitch); }
int pdwt_wp1h_node_costs(void* h, int depth, int kind, double* out, double* per_row) { return W1(h)->node_costs(depth, kind, out, per_row); }

void* pdwt_wpbh_new(DTYPE* imgs, int B, int Nr, int Nc, const char* wname, int levels, int memisonhost, int allow_fused)
{
    return new (std::nothrow) WaveletPacketsImages(imgs, B, Nr, Nc, wname, levels, memisonhost, allow_fused);
}
void pdwt_wpbh_info(void* h, w_info_wptb* out) { *out = WB(h)->winfos; }
int pdwt_wpbh_geometry(int Nr, int Nc, int hlen, int levels, int* nr, int* nc) { return WaveletPacketsImages::geometry(Nr, Nc, hlen, levels, nr, nc); }
int pdwt_wpbh_path_index(const char* path, int* depth) { return WaveletPacketsImages::path_index(path, depth); }
int pdwt_wpbh_fused(void* h) { return WB(h)->fused(); }
long long pdwt_wpbh_get_image(void* h, DTYPE* out) { return WB(h)->get_image(out); }
long long pdwt_wpbh_get_node(void* h, DTYPE* out, int depth, int idx) { return WB(h)->get_node(out, depth, idx); }
long long pdwt_wpbh_set_node(void* h, DTYPE* in, int depth, int idx, int mem_is_on_device) { return WB(h)->set_node(in, depth, idx, mem_is_on_device); }
intptr_t pdwt_wpbh_node_int_ptr(void* h, int depth, int idx, long long* pitch) { return WB(h)->node_int_ptr(depth, idx, pitch); }
int pdwt_wpbh_node_costs(void* h, int depth, int kind, double* per_image, double* summed) { return WB(h)->node_costs(depth, kind, per_image, summed); }
int pdwt_wpbh_images_norm1(void* h, double* out) { return WB(h)->images_norm1(out); }
int pdwt_wpbh_images_estimate_sigma(void* h, double* out) { return WB(h)->images_estimate_sigma(out); }
}
#undef WP
#undef W1
#undef WB
