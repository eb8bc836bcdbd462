// wpt.cpp -- host side of `WaveletPackets` (include/wpt.h) above the packet entry points of include/pdwt_hip.h, and its flat C handle
// API (pdwt_wpt_*, the shape of wt3d.cpp).  Plain host C++ like wt.cpp, built into libpdwt.so (float) and libpdwtd.so
// (-DDOUBLEPRECISION).  The tree geometry, the basis (flags per depth, the lists of parents the inverse has to synthesise) and the
// best-basis search live here; the device only ever sees one depth step, a cost or a per-node threshold over one depth.
#include <limits.h>
#include <new>
#include <string.h>
#include <vector>

#include "../../include/wpt.h"
#include "host_common.hpp"

static_assert(sizeof(w_band_stats) == sizeof(pdwt_band_stats), "w_band_stats must mirror pdwt_band_stats");

namespace {
constexpr int kL = WPT_MAX_LEVELS;
inline int nnodes(int depth) { return 1 << (2 * depth); }

struct wpt_priv {
    filters_t f;
    int dev;  // the device current at construction; every method runs there
    int nr[kL + 1], nc[kL + 1];
    std::vector<unsigned char> in_basis[kL + 1];  // per depth: 1 = the node belongs to the basis
    std::vector<int> parents[kL + 1];             // per depth: the nodes that lie above basis nodes (what inverse() synthesises)
    DTYPE** d_ptr;                                // device: the node pointers of every depth, depth l at ptr_off[l] (B = 4^l, nb = 1 tables)
    int* d_lists;                                 // device: parents[l] at ptr_off[l]
    size_t ptr_off[kL + 2];
};
inline wpt_priv* P(void* p) { return (wpt_priv*)p; }

// flags per depth from a list of nodes; false unless the nodes partition the tree
bool flags_from_nodes(int L, const int* depth, const int* idx, int n, std::vector<unsigned char>* flags)
{
    if (!depth || !idx || n < 1) return false;
    std::vector<unsigned char> leaf((size_t)nnodes(L), 0);
    for (int l = 0; l <= L; l++) flags[l].assign((size_t)nnodes(l), 0);
    for (int k = 0; k < n; k++) {
        const int d = depth[k], i = idx[k];
        if (d < 0 || d > L || i < 0 || i >= nnodes(d)) return false;
        const int span = nnodes(L - d);
        for (int j = i * span; j < (i + 1) * span; j++) {
            if (leaf[j]) return false;  // two nodes on one root-to-leaf path
            leaf[j] = 1;
        }
        flags[d][i] = 1;
    }
    for (size_t j = 0; j < leaf.size(); j++)
        if (!leaf[j]) return false;  // a path that meets no node
    return true;
}
}  // namespace
#define ON_MY_DEVICE_W() DevScope dev_scope_(priv_ ? ((const wpt_priv*)priv_)->dev : -1)

// install flags (a valid partition): the parents above basis nodes, per depth, on the host and on the device
static int install_basis(wpt_priv* p, int L, std::vector<unsigned char>* flags)
{
    std::vector<unsigned char> above, below;  // "lies above basis nodes" of depth l and l + 1
    for (int l = L; l >= 0; l--) {
        above.assign((size_t)nnodes(l), 0);
        if (l < L)
            for (int i = 0; i < nnodes(l); i++)
                for (int q = 0; q < 4; q++) above[i] |= (unsigned char)(flags[l + 1][4 * i + q] | below[4 * i + q]);
        p->parents[l].clear();
        for (int i = 0; i < nnodes(l); i++)
            if (above[i]) p->parents[l].push_back(i);
        if (!p->parents[l].empty()) {
            const int rc = pdwt_memcpy_h2d(p->d_lists + p->ptr_off[l], p->parents[l].data(), p->parents[l].size() * sizeof(int));
            if (rc != PDWT_OK) return rc;
        }
        below.swap(above);
    }
    for (int l = 0; l <= L; l++) p->in_basis[l] = flags[l];
    return PDWT_OK;
}

int WaveletPackets::geometry(int Nr, int Nc, int hlen, int levels, int* nr, int* nc)
{
    if (Nr < 1 || Nc < 1 || hlen < 2 || (unsigned long long)Nr * (unsigned long long)Nc >= (1ull << 31)) return 0;
    if (levels < 1) levels = 1;
    int wmaxlev = w_ilog2((Nr < Nc ? Nr : Nc) / (hlen - 1));  // the rule of Wavelets (src/wt.cu:155-165)
    if (wmaxlev > kL) wmaxlev = kL;
    if (levels > wmaxlev) levels = wmaxlev;
    for (int l = 0; l <= levels; l++) {
        if (nr) nr[l] = Nr;
        if (nc) nc[l] = Nc;
        Nr = (Nr + 1) >> 1, Nc = (Nc + 1) >> 1;
    }
    return levels;
}

int WaveletPackets::path_index(const char* path, int* depth)
{
    if (!path) return -1;
    int i = 0, d = 0;
    for (; path[d]; d++) {
        if (d >= WPT_MAX_LEVELS) return -1;
        int q;
        switch (path[d]) {
        case 'a': q = 0; break;
        case 'h': q = 1; break;
        case 'v': q = 2; break;
        case 'd': q = 3; break;
        default: return -1;
        }
        i = 4 * i + q;
    }
    if (depth) *depth = d;
    return i;
}

WaveletPackets::WaveletPackets(DTYPE* img, int Nr, int Nc, const char* wname_, int levels, int memisonhost) : d_image(NULL), state(W_INIT), priv_(NULL)
{
    for (int l = 0; l <= kL; l++) d_nodes[l] = NULL;
    winfos.Nr = Nr, winfos.Nc = Nc, winfos.nlevels = levels, winfos.hlen = 0;
    strncpy(wname, wname_ ? wname_ : "", 127);
    wname[127] = 0;
    if (Nr < 1 || Nc < 1 || !wname_ || (unsigned long long)Nr * (unsigned long long)Nc >= (1ull << 31)) {
        puts("ERROR: WaveletPackets(): invalid image size or wavelet name");
        state = W_CREATION_ERROR;
        return;
    }
    if (levels < 1) {
        puts("Warning: cannot initialize wavelet coefficients with nlevels < 1. Forcing nlevels = 1");
        winfos.nlevels = 1;
    }
    wpt_priv* p = new (std::nothrow) wpt_priv();
    if (!p) {
        state = W_CREATION_ERROR;
        return;
    }
    priv_ = p;
    p->d_ptr = NULL, p->d_lists = NULL;
    p->dev = pdwt_get_device();
    const int hlen = SFX(pdwt_compute_filters_separable)(wname, 0, &p->f);
    if (hlen <= 0) {
        printf("ERROR: unknown wavelet name %s\n", wname);
        state = W_CREATION_ERROR;
        return;
    }
    p->f.hlen = hlen;
    winfos.hlen = hlen;
    const int wmaxlev = geometry(Nr, Nc, hlen, winfos.nlevels, p->nr, p->nc);
    if (winfos.nlevels > wmaxlev) {
        printf("Warning: required level (%d) is greater than the maximum possible level for %s packets (%d) on a %dx%d image.\n", winfos.nlevels, wname, wmaxlev, Nr, Nc);
        printf("Forcing nlevels = %d\n", wmaxlev);
        winfos.nlevels = wmaxlev;
    }
    if (winfos.nlevels < 1) {
        printf("ERROR: a %dx%d image is too small for one level of %s\n", Nr, Nc, wname);
        state = W_CREATION_ERROR;
        return;
    }
    const int L = winfos.nlevels;
    p->ptr_off[0] = 0;
    for (int l = 0; l <= L; l++) p->ptr_off[l + 1] = p->ptr_off[l] + (size_t)nnodes(l);
    int rc = PDWT_OK;
    for (int l = 0; l <= L && rc == PDWT_OK; l++) {
        const size_t nb = (size_t)nnodes(l) * p->nr[l] * p->nc[l] * sizeof(DTYPE);
        d_nodes[l] = (DTYPE*)pdwt_malloc(nb);
        if (!d_nodes[l]) rc = PDWT_ENOMEM;
        else if (l > 0) rc = pdwt_memset(d_nodes[l], 0, nb);
    }
    d_image = d_nodes[0];
    if (rc == PDWT_OK) {
        p->d_ptr = (DTYPE**)pdwt_malloc(p->ptr_off[L + 1] * sizeof(DTYPE*));
        p->d_lists = (int*)pdwt_malloc(p->ptr_off[L + 1] * sizeof(int));
        if (!p->d_ptr || !p->d_lists) rc = PDWT_ENOMEM;
    }
    if (rc == PDWT_OK) {
        std::vector<DTYPE*> tab(p->ptr_off[L + 1]);
        for (int l = 0; l <= L; l++)
            for (int i = 0; i < nnodes(l); i++) tab[p->ptr_off[l] + i] = d_nodes[l] + (size_t)i * p->nr[l] * p->nc[l];
        rc = pdwt_memcpy_h2d(p->d_ptr, tab.data(), tab.size() * sizeof(DTYPE*));
    }
    if (rc == PDWT_OK) {  // the default basis: every node of depth L
        std::vector<unsigned char> flags[kL + 1];
        for (int l = 0; l <= L; l++) flags[l].assign((size_t)nnodes(l), l == L ? 1 : 0);
        rc = install_basis(p, L, flags);
    }
    if (rc == PDWT_OK) {
        const size_t n = (size_t)Nr * Nc;
        if (!img) rc = pdwt_memset(d_image, 0, n * sizeof(DTYPE));
        else if (memisonhost) rc = pdwt_memcpy_h2d(d_image, img, n * sizeof(DTYPE));
        else rc = pdwt_memcpy_d2d_foreign(d_image, img, n * sizeof(DTYPE));
    }
    if (rc != PDWT_OK) {
        report("WaveletPackets", "(): allocation or upload", rc);
        state = W_CREATION_ERROR;
    }
}

WaveletPackets::~WaveletPackets()
{
    ON_MY_DEVICE_W();
    for (int l = 0; l <= kL; l++)
        if (d_nodes[l]) pdwt_free(d_nodes[l]);
    if (priv_) {
        if (P(priv_)->d_ptr) pdwt_free(P(priv_)->d_ptr);
        if (P(priv_)->d_lists) pdwt_free(P(priv_)->d_lists);
        delete P(priv_);
    }
}

void WaveletPackets::forward()
{
    ON_MY_DEVICE_W();
    if (state == W_CREATION_ERROR) {
        puts("Warning: forward transform not computed, as there was an error when creating the wavelets");
        return;
    }
    wpt_priv* p = P(priv_);
    for (int l = 0; l < winfos.nlevels; l++) {
        const int rc = SFX(pdwt_wpt2d_forward_level)(d_nodes[l], d_nodes[l + 1], p->nr[l], p->nc[l], NULL, nnodes(l), &p->f);
        if (rc != PDWT_OK) {
            report("WaveletPackets", "::forward()", rc);
            state = W_FORWARD_ERROR;
            return;
        }
    }
    state = W_FORWARD;
}

void WaveletPackets::inverse()
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
    wpt_priv* p = P(priv_);
    for (int l = winfos.nlevels - 1; l >= 0; l--) {
        const int n = (int)p->parents[l].size();
        if (!n) continue;
        const int* list = (n == nnodes(l)) ? NULL : p->d_lists + p->ptr_off[l];
        const int rc = SFX(pdwt_wpt2d_inverse_level)(d_nodes[l], d_nodes[l + 1], p->nr[l], p->nc[l], list, n, &p->f);
        if (rc != PDWT_OK) {
            report("WaveletPackets", "::inverse()", rc);
            state = W_INVERSE_ERROR;
            return;
        }
    }
    state = W_INVERSE;
}

int WaveletPackets::get_image(DTYPE* res)
{
    ON_MY_DEVICE_W();
    if (!d_image || !res || state == W_CREATION_ERROR) return 0;
    const size_t n = (size_t)winfos.Nr * winfos.Nc;
    if (pdwt_memcpy_d2h(res, d_image, n * sizeof(DTYPE)) != PDWT_OK) return 0;
    return (int)n;
}

void WaveletPackets::set_image(DTYPE* img, int mem_is_on_device)
{
    ON_MY_DEVICE_W();
    if (!d_image || !img || state == W_CREATION_ERROR) return;
    const size_t nb = (size_t)winfos.Nr * winfos.Nc * sizeof(DTYPE);
    const int rc = mem_is_on_device ? pdwt_memcpy_d2d_foreign(d_image, img, nb) : pdwt_memcpy_h2d(d_image, img, nb);
    if (rc != PDWT_OK) report("WaveletPackets", "::set_image()", rc);
    state = W_INIT;
}

long long WaveletPackets::node_shape(int depth, int* nr, int* nc) const
{
    if (state == W_CREATION_ERROR || depth < 0 || depth > winfos.nlevels) return 0;
    const wpt_priv* p = P(priv_);
    if (nr) *nr = p->nr[depth];
    if (nc) *nc = p->nc[depth];
    return (long long)p->nr[depth] * p->nc[depth];
}

int WaveletPackets::get_node(DTYPE* out, int depth, int idx)
{
    ON_MY_DEVICE_W();
    if (state == W_INVERSE) {
        puts("Warning: get_node(): inverse() has been performed, the coefficients has been modified and do not make sense anymore.");
        return 0;
    }
    const long long n = node_shape(depth, NULL, NULL);
    if (n <= 0 || !out || idx < 0 || idx >= nnodes(depth)) return 0;
    if (pdwt_memcpy_d2h(out, d_nodes[depth] + (size_t)idx * n, (size_t)n * sizeof(DTYPE)) != PDWT_OK) return 0;
    return (int)n;
}

long long WaveletPackets::get_level(DTYPE* out, int depth)
{
    ON_MY_DEVICE_W();
    if (state == W_INVERSE) {
        puts("Warning: get_level(): inverse() has been performed, the coefficients has been modified and do not make sense anymore.");
        return 0;
    }
    const long long n = node_shape(depth, NULL, NULL) * (depth >= 0 && depth <= kL ? nnodes(depth) : 0);
    if (n <= 0 || !out) return 0;
    if (pdwt_memcpy_d2h(out, d_nodes[depth], (size_t)n * sizeof(DTYPE)) != PDWT_OK) return 0;
    return n;
}

int WaveletPackets::set_node(DTYPE* in, int depth, int idx, int mem_is_on_device)
{
    ON_MY_DEVICE_W();
    if (!(state == W_FORWARD || state == W_THRESHOLD)) {
        puts("Warning: set_node(): refused, the tree does not hold the coefficients of a forward() (run forward() first)");
        return 0;
    }
    const long long n = node_shape(depth, NULL, NULL);
    if (n <= 0 || !in || idx < 0 || idx >= nnodes(depth)) return 0;
    DTYPE* dst = d_nodes[depth] + (size_t)idx * n;
    const int rc = mem_is_on_device ? pdwt_memcpy_d2d_foreign(dst, in, (size_t)n * sizeof(DTYPE)) : pdwt_memcpy_h2d(dst, in, (size_t)n * sizeof(DTYPE));
    if (rc != PDWT_OK) {
        report("WaveletPackets", "::set_node()", rc);
        return 0;
    }
    state = W_THRESHOLD;
    return (int)n;
}

intptr_t WaveletPackets::node_int_ptr(int depth, int idx)
{
    const long long n = node_shape(depth, NULL, NULL);
    if (n <= 0 || idx < 0 || idx >= nnodes(depth)) return 0;
    return (intptr_t)(d_nodes[depth] + (size_t)idx * n);
}

int WaveletPackets::node_costs(int depth, int kind, double* out)
{
    ON_MY_DEVICE_W();
    const long long n = node_shape(depth, NULL, NULL);
    if (!(state == W_FORWARD || state == W_THRESHOLD) || n <= 0 || !out) return PDWT_EINVAL;
    const int rc = SFX(pdwt_wpt2d_node_cost)(d_nodes[depth], (size_t)n, nnodes(depth), kind, out);
    if (rc != PDWT_OK) report("WaveletPackets", "::node_costs()", rc);
    return rc;
}

int WaveletPackets::best_basis(int kind)
{
    ON_MY_DEVICE_W();
    if (state != W_FORWARD || (kind != 0 && kind != 1)) return PDWT_EINVAL;
    const int L = winfos.nlevels;
    std::vector<double> best[kL + 1];
    std::vector<unsigned char> keep[kL + 1], flags[kL + 1];
    for (int l = 0; l <= L; l++) {
        best[l].resize((size_t)nnodes(l));
        if (const int rc = node_costs(l, kind, best[l].data()); rc != PDWT_OK) return rc;
        keep[l].assign((size_t)nnodes(l), 1);
        flags[l].assign((size_t)nnodes(l), 0);
    }
    for (int l = L - 1; l >= 0; l--)
        for (int i = 0; i < nnodes(l); i++) {
            const double* c = &best[l + 1][4 * (size_t)i];
            const double below = ((c[0] + c[1]) + c[2]) + c[3];
            if (!(best[l][i] <= below)) keep[l][i] = 0, best[l][i] = below;
        }
    flags[0][0] = 1;  // top-down: a node that is not kept hands over to its children
    for (int l = 0; l < L; l++)
        for (int i = 0; i < nnodes(l); i++)
            if (flags[l][i] && !keep[l][i]) {
                flags[l][i] = 0;
                for (int q = 0; q < 4; q++) flags[l + 1][4 * i + q] = 1;
            }
    if (const int rc = install_basis(P(priv_), L, flags); rc != PDWT_OK) return rc;
    return basis_size();
}

int WaveletPackets::set_basis(const int* depth, const int* idx, int n)
{
    ON_MY_DEVICE_W();
    if (state == W_CREATION_ERROR || state == W_THRESHOLD || state == W_THRESHOLD_ERROR) return PDWT_EINVAL;
    std::vector<unsigned char> flags[kL + 1];
    if (!flags_from_nodes(winfos.nlevels, depth, idx, n, flags)) return PDWT_EINVAL;
    return install_basis(P(priv_), winfos.nlevels, flags);
}

int WaveletPackets::basis_size() const { return get_basis(NULL, NULL); }

int WaveletPackets::get_basis(int* depth, int* idx) const
{
    if (state == W_CREATION_ERROR) return 0;
    const wpt_priv* p = P(priv_);
    int n = 0;
    for (int l = 0; l <= winfos.nlevels; l++)
        for (int i = 0; i < nnodes(l); i++)
            if (p->in_basis[l][i]) {
                if (depth) depth[n] = l;
                if (idx) idx[n] = i;
                n++;
            }
    return n;
}

void WaveletPackets::threshold(int op, DTYPE beta, int do_thresh_appcoeffs)
{
    ON_MY_DEVICE_W();
    if (state == W_INVERSE) {
        puts("Warning: WaveletPackets(): cannot threshold coefficients, as they were modified by W.inverse()");
        return;
    }
    if (state == W_CREATION_ERROR) return;
    wpt_priv* p = P(priv_);
    std::vector<DTYPE> betas;
    for (int l = 0; l <= winfos.nlevels; l++) {
        betas.assign((size_t)nnodes(l), (DTYPE)-1);
        int any = 0;
        for (int i = (do_thresh_appcoeffs ? 0 : 1); i < nnodes(l); i++)  // node 0 of every depth is the all-"a" path
            if (p->in_basis[l][i]) betas[i] = beta, any = 1;
        if (!any) continue;
        const size_t n = (size_t)p->nr[l] * p->nc[l];
        const int rc = SFX(pdwt_bandbatch_thresh)(op, p->d_ptr + p->ptr_off[l], &n, betas.data(), nnodes(l), 1);
        if (rc != PDWT_OK) {
            report("WaveletPackets", op ? "::hard_threshold()" : "::soft_threshold()", rc);
            state = W_THRESHOLD_ERROR;
            return;
        }
    }
    state = W_THRESHOLD;
}
void WaveletPackets::soft_threshold(DTYPE beta, int do_thresh_appcoeffs) { threshold(0, beta, do_thresh_appcoeffs); }
void WaveletPackets::hard_threshold(DTYPE beta, int do_thresh_appcoeffs) { threshold(1, beta, do_thresh_appcoeffs); }

double WaveletPackets::norm1()
{
    ON_MY_DEVICE_W();
    if (!(state == W_FORWARD || state == W_THRESHOLD)) return -1.0;
    wpt_priv* p = P(priv_);
    std::vector<double> c;
    double sum = 0.0;
    for (int l = 0; l <= winfos.nlevels; l++) {
        int any = 0;
        for (int i = 0; i < nnodes(l) && !any; i++) any = p->in_basis[l][i];
        if (!any) continue;
        c.resize((size_t)nnodes(l));
        if (node_costs(l, 0, c.data()) != PDWT_OK) return -1.0;
        for (int i = 0; i < nnodes(l); i++)
            if (p->in_basis[l][i]) sum += c[i];
    }
    return sum;
}

int WaveletPackets::node_stats(int depth, w_band_stats* out)
{
    ON_MY_DEVICE_W();
    const long long n = node_shape(depth, NULL, NULL);
    if (!(state == W_FORWARD || state == W_THRESHOLD) || n <= 0 || !out) return PDWT_EINVAL;
    wpt_priv* p = P(priv_);
    const size_t ne = (size_t)n;
    const int rc = SFX(pdwt_bandbatch_stats)(p->d_ptr + p->ptr_off[depth], &ne, nnodes(depth), 1, NULL, reinterpret_cast<pdwt_band_stats*>(out));
    if (rc != PDWT_OK) report("WaveletPackets", "::node_stats()", rc);
    return rc;
}

double WaveletPackets::estimate_sigma()
{
    ON_MY_DEVICE_W();
    if (!(state == W_FORWARD || state == W_THRESHOLD)) return -1.0;
    wpt_priv* p = P(priv_);
    const size_t n = (size_t)p->nr[1] * p->nc[1];
    const DTYPE* d = d_nodes[1] + 3 * n;  // node "d"
    const unsigned char want = 2;         // the median alone
    pdwt_band_stats s;
    const int rc = SFX(pdwt_bandlist_stats)(&d, &n, 1, &want, &s);
    if (rc != PDWT_OK) {
        report("WaveletPackets", "::estimate_sigma()", rc);
        return -1.0;
    }
    return s.median_abs / 0.6744897501960817;
}

// ---- flat C handle API (pdwt_amd/wpt.py) ------------------------------------------------------------------
#define WP(h) static_cast<WaveletPackets*>(h)
extern "C" {
void* pdwt_wpt_new(DTYPE* img, int Nr, int Nc, const char* wname, int levels, int memisonhost) { return new (std::nothrow) WaveletPackets(img, Nr, Nc, wname, levels, memisonhost); }
void pdwt_wpt_delete(void* h) { delete WP(h); }
void pdwt_wpt_forward(void* h) { WP(h)->forward(); }
void pdwt_wpt_inverse(void* h) { WP(h)->inverse(); }
int pdwt_wpt_get_image(void* h, DTYPE* out) { return WP(h)->get_image(out); }
void pdwt_wpt_set_image(void* h, DTYPE* img, int mem_is_on_device) { WP(h)->set_image(img, mem_is_on_device); }
int pdwt_wpt_state(void* h) { return (int)WP(h)->state; }
void pdwt_wpt_info(void* h, w_info_wpt* out) { *out = WP(h)->winfos; }
long long pdwt_wpt_node_shape(void* h, int depth, int* nr, int* nc) { return WP(h)->node_shape(depth, nr, nc); }
int pdwt_wpt_path_index(const char* path, int* depth) { return WaveletPackets::path_index(path, depth); }
int pdwt_wpt_geometry(int Nr, int Nc, int hlen, int levels, int* nr, int* nc) { return WaveletPackets::geometry(Nr, Nc, hlen, levels, nr, nc); }
int pdwt_wpt_get_node(void* h, DTYPE* out, int depth, int idx) { return WP(h)->get_node(out, depth, idx); }
long long pdwt_wpt_get_level(void* h, DTYPE* out, int depth) { return WP(h)->get_level(out, depth); }
int pdwt_wpt_set_node(void* h, DTYPE* in, int depth, int idx, int mem_is_on_device) { return WP(h)->set_node(in, depth, idx, mem_is_on_device); }
intptr_t pdwt_wpt_node_int_ptr(void* h, int depth, int idx) { return WP(h)->node_int_ptr(depth, idx); }
int pdwt_wpt_node_costs(void* h, int depth, int kind, double* out) { return WP(h)->node_costs(depth, kind, out); }
int pdwt_wpt_best_basis(void* h, int kind) { return WP(h)->best_basis(kind); }
int pdwt_wpt_set_basis(void* h, const int* depth, const int* idx, int n) { return WP(h)->set_basis(depth, idx, n); }
int pdwt_wpt_basis_size(void* h) { return WP(h)->basis_size(); }
int pdwt_wpt_get_basis(void* h, int* depth, int* idx) { return WP(h)->get_basis(depth, idx); }
void pdwt_wpt_soft_threshold(void* h, DTYPE beta, int app) { WP(h)->soft_threshold(beta, app); }
void pdwt_wpt_hard_threshold(void* h, DTYPE beta, int app) { WP(h)->hard_threshold(beta, app); }
double pdwt_wpt_norm1(void* h) { return WP(h)->norm1(); }
int pdwt_wpt_node_stats(void* h, int depth, w_band_stats* out) { return WP(h)->node_stats(depth, out); }
double pdwt_wpt_estimate_sigma(void* h) { return WP(h)->estimate_sigma(); }
}
#undef WP
