// wpt1d.cpp -- host side of `WaveletPackets1D` (include/wpt1d.h) above the "Batched 1-D wavelet packets" entry points of
// include/pdwt_hip.h, and its flat C handle API (pdwt_wp1h_*, the shape of wpt.cpp).  Plain host C++ like wt.cpp, built into libpdwt.so
// (float) and libpdwtd.so (-DDOUBLEPRECISION).  The basis (flags per depth, the node-state table of the inverse) and the best-basis
// search live here; the device sees the whole tree of the rows, one depth step, the moments or a per-node threshold over one depth.
#include <limits.h>
#include <math.h>
#include <new>
#include <string.h>
#include <vector>

#include "../../include/wpt1d.h"
#include "host_common.hpp"

static_assert(sizeof(w_band_stats) == sizeof(pdwt_band_stats), "w_band_stats must mirror pdwt_band_stats");

namespace {
constexpr int kL = WPT1D_MAX_LEVELS;
inline int nnodes(int depth) { return 1 << depth; }
inline size_t toff(int depth) { return ((size_t)1 << depth) - 1; }  // where depth l starts in the node tables

struct wp1_priv {
    filters_t f;
    int dev;  // the device current at construction; every method runs there
    int n[kL + 1];
    int fused;
    std::vector<unsigned char> in_basis[kL + 1];  // per depth: 1 = the node belongs to the basis
    std::vector<unsigned char> state;             // host copy of the node-state table (pdwt_wp1_state_table)
    unsigned char* d_state;                       // device: that table; depth l at toff(l)
    unsigned char* d_thr;                         // device: 1 = a basis node other than the all-"a" node of its depth
};
inline wp1_priv* P(void* p) { return (wp1_priv*)p; }

// install a basis given as pairs: the state table (which validates the partition), the flags, and both on the device
int install_basis(wp1_priv* p, int L, const int* depth, const int* idx, int n)
{
    std::vector<unsigned char> st((size_t)2 << L);
    if (const int rc = pdwt_wp1_state_table(L, depth, idx, n, st.data()); rc != PDWT_OK) return rc;
    std::vector<unsigned char> thr(st.size(), 0);
    for (int l = 0; l <= L; l++)
        for (int i = 1; i < nnodes(l); i++) thr[toff(l) + i] = st[toff(l) + i] == 1;
    if (const int rc = pdwt_memcpy_h2d(p->d_state, st.data(), st.size()); rc != PDWT_OK) return rc;
    if (const int rc = pdwt_memcpy_h2d(p->d_thr, thr.data(), thr.size()); rc != PDWT_OK) return rc;
    for (int l = 0; l <= L; l++) {
        p->in_basis[l].assign((size_t)nnodes(l), 0);
        for (int i = 0; i < nnodes(l); i++) p->in_basis[l][i] = st[toff(l) + i] == 1;
    }
    p->state.swap(st);
    return PDWT_OK;
}
}  // namespace
#define ON_MY_DEVICE_P() DevScope dev_scope_(priv_ ? ((const wp1_priv*)priv_)->dev : -1)

int WaveletPackets1D::geometry(int Nc, int hlen, int levels, int* n) { return pdwt_wp1_geometry(Nc, hlen, levels, n); }

int WaveletPackets1D::path_index(const char* path, int* depth)
{
    if (!path) return -1;
    int i = 0, d = 0;
    for (; path[d]; d++) {
        if (d >= WPT1D_MAX_LEVELS) return -1;
        if (path[d] != 'a' && path[d] != 'd') return -1;
        i = 2 * i + (path[d] == 'd');
    }
    if (depth) *depth = d;
    return i;
}

int WaveletPackets1D::frequency_order(int depth, int* out) { return pdwt_wp1_frequency_order(depth, out) == PDWT_OK ? 1 << depth : 0; }

WaveletPackets1D::WaveletPackets1D(DTYPE* rows, int Nr, int Nc, const char* wname_, int levels, int memisonhost) : d_image(NULL), state(W_INIT), priv_(NULL)
{
    for (int l = 0; l <= kL; l++) d_nodes[l] = NULL;
    winfos.Nr = Nr, winfos.Nc = Nc, winfos.nlevels = levels, winfos.hlen = 0;
    strncpy(wname, wname_ ? wname_ : "", 127);
    wname[127] = 0;
    if (Nr < 1 || Nc < 1 || !wname_ || (unsigned long long)Nr * (unsigned long long)Nc >= (1ull << 31)) {
        puts("ERROR: WaveletPackets1D(): invalid batch size or wavelet name");
        state = W_CREATION_ERROR;
        return;
    }
    if (levels < 1) {
        puts("Warning: cannot initialize wavelet coefficients with nlevels < 1. Forcing nlevels = 1");
        winfos.nlevels = 1;
    }
    wp1_priv* p = new (std::nothrow) wp1_priv();
    if (!p) {
        state = W_CREATION_ERROR;
        return;
    }
    priv_ = p;
    p->d_state = NULL, p->d_thr = NULL, p->fused = 0;
    p->dev = pdwt_get_device();
    const int hlen = SFX(pdwt_compute_filters_separable)(wname, 0, &p->f);
    if (hlen <= 0) {
        printf("ERROR: unknown wavelet name %s\n", wname);
        state = W_CREATION_ERROR;
        return;
    }
    p->f.hlen = hlen;
    winfos.hlen = hlen;
    const int wmaxlev = geometry(Nc, hlen, winfos.nlevels, p->n);
    if (winfos.nlevels > wmaxlev) {
        printf("Warning: required level (%d) is greater than the maximum possible level for %s packets (%d) on rows of %d samples.\n", winfos.nlevels, wname, wmaxlev, Nc);
        printf("Forcing nlevels = %d\n", wmaxlev);
        winfos.nlevels = wmaxlev;
    }
    if (winfos.nlevels < 1) {
        printf("ERROR: rows of %d samples are too short for one level of %s\n", Nc, wname);
        state = W_CREATION_ERROR;
        return;
    }
    const int L = winfos.nlevels;
    p->fused = pdwt_wp1_fused(Nc, hlen, L, (int)sizeof(DTYPE)) == 1;
    int rc = PDWT_OK;
    for (int l = 0; l <= L && rc == PDWT_OK; l++) {
        const size_t nb = (size_t)Nr * nnodes(l) * p->n[l] * sizeof(DTYPE);
        d_nodes[l] = (DTYPE*)pdwt_malloc(nb);
        if (!d_nodes[l]) rc = PDWT_ENOMEM;
        else if (l > 0) rc = pdwt_memset(d_nodes[l], 0, nb);
    }
    d_image = d_nodes[0];
    if (rc == PDWT_OK) {
        p->d_state = (unsigned char*)pdwt_malloc((size_t)2 << L);
        p->d_thr = (unsigned char*)pdwt_malloc((size_t)2 << L);
        if (!p->d_state || !p->d_thr) rc = PDWT_ENOMEM;
    }
    if (rc == PDWT_OK) {  // the default basis: every node of depth L
        std::vector<int> d((size_t)nnodes(L), L), i((size_t)nnodes(L));
        for (int k = 0; k < nnodes(L); k++) i[k] = k;
        rc = install_basis(p, L, d.data(), i.data(), nnodes(L));
    }
    if (rc == PDWT_OK) {
        const size_t n = (size_t)Nr * Nc;
        if (!rows) rc = pdwt_memset(d_image, 0, n * sizeof(DTYPE));
        else if (memisonhost) rc = pdwt_memcpy_h2d(d_image, rows, n * sizeof(DTYPE));
        else rc = pdwt_memcpy_d2d_foreign(d_image, rows, n * sizeof(DTYPE));
    }
    if (rc != PDWT_OK) {
        report("WaveletPackets1D", "(): allocation or upload", rc);
        state = W_CREATION_ERROR;
    }
}

WaveletPackets1D::~WaveletPackets1D()
{
    ON_MY_DEVICE_P();
    for (int l = 0; l <= kL; l++)
        if (d_nodes[l]) pdwt_free(d_nodes[l]);
    if (priv_) {
        if (P(priv_)->d_state) pdwt_free(P(priv_)->d_state);
        if (P(priv_)->d_thr) pdwt_free(P(priv_)->d_thr);
        delete P(priv_);
    }
}

int WaveletPackets1D::fused() const { return (priv_ && state != W_CREATION_ERROR) ? P(priv_)->fused : 0; }

void WaveletPackets1D::forward()
{
    ON_MY_DEVICE_P();
    if (state == W_CREATION_ERROR) {
        puts("Warning: forward transform not computed, as there was an error when creating the wavelets");
        return;
    }
    wp1_priv* p = P(priv_);
    const int rc = SFX(pdwt_wp1_forward)(d_image, d_nodes + 1, winfos.Nr, winfos.Nc, winfos.nlevels, &p->f);
    if (rc < 0) {
        report("WaveletPackets1D", "::forward()", rc);
        state = W_FORWARD_ERROR;
        return;
    }
    state = W_FORWARD;
}

void WaveletPackets1D::inverse()
{
    ON_MY_DEVICE_P();
    if (state == W_INVERSE) {
        puts("Warning: W.inverse() has already been run. Inverse is available in W.get_image()");
        return;
    }
    if (state == W_CREATION_ERROR || state == W_FORWARD_ERROR || state == W_THRESHOLD_ERROR) {
        puts("Warning: inverse transform not computed, as there was an error in a previous stage");
        return;
    }
    wp1_priv* p = P(priv_);
    if (!p->in_basis[0][0]) {  // (the batch itself as the basis: nothing to synthesise)
        const int rc = SFX(pdwt_wp1_inverse)(d_image, d_nodes + 1, winfos.Nr, winfos.Nc, winfos.nlevels, p->d_state, &p->f);
        if (rc < 0) {
            report("WaveletPackets1D", "::inverse()", rc);
            state = W_INVERSE_ERROR;
            return;
        }
    }
    state = W_INVERSE;
}

int WaveletPackets1D::get_image(DTYPE* res)
{
    ON_MY_DEVICE_P();
    if (!d_image || !res || state == W_CREATION_ERROR) return 0;
    const size_t n = (size_t)winfos.Nr * winfos.Nc;
    if (pdwt_memcpy_d2h(res, d_image, n * sizeof(DTYPE)) != PDWT_OK) return 0;
    return (int)n;
}

void WaveletPackets1D::set_image(DTYPE* rows, int mem_is_on_device)
{
    ON_MY_DEVICE_P();
    if (!d_image || !rows || state == W_CREATION_ERROR) return;
    const size_t nb = (size_t)winfos.Nr * winfos.Nc * sizeof(DTYPE);
    const int rc = mem_is_on_device ? pdwt_memcpy_d2d_foreign(d_image, rows, nb) : pdwt_memcpy_h2d(d_image, rows, nb);
    if (rc != PDWT_OK) report("WaveletPackets1D", "::set_image()", rc);
    state = W_INIT;
}

long long WaveletPackets1D::node_shape(int depth, int* nr, int* n) const
{
    if (state == W_CREATION_ERROR || depth < 0 || depth > winfos.nlevels) return 0;
    const wp1_priv* p = P(priv_);
    if (nr) *nr = winfos.Nr;
    if (n) *n = p->n[depth];
    return (long long)winfos.Nr * p->n[depth];
}

intptr_t WaveletPackets1D::node_int_ptr(int depth, int idx, long long* pitch)
{
    const long long n = node_shape(depth, NULL, NULL);
    if (n <= 0 || idx < 0 || idx >= nnodes(depth)) return 0;
    const int nl = P(priv_)->n[depth];
    if (pitch) *pitch = (long long)nnodes(depth) * nl;
    return (intptr_t)(d_nodes[depth] + (size_t)idx * nl);
}

int WaveletPackets1D::get_node(DTYPE* out, int depth, int idx)
{
    ON_MY_DEVICE_P();
    if (state == W_INVERSE) {
        puts("Warning: get_node(): inverse() has been performed, the coefficients has been modified and do not make sense anymore.");
        return 0;
    }
    long long pitch = 0;
    const intptr_t src = node_int_ptr(depth, idx, &pitch);
    if (!src || !out) return 0;
    const size_t w = (size_t)P(priv_)->n[depth] * sizeof(DTYPE);
    if (pdwt_memcpy2d(out, w, (const void*)src, (size_t)pitch * sizeof(DTYPE), w, (size_t)winfos.Nr, 1) != PDWT_OK) return 0;
    return (int)node_shape(depth, NULL, NULL);
}

long long WaveletPackets1D::get_level(DTYPE* out, int depth)
{
    ON_MY_DEVICE_P();
    if (state == W_INVERSE) {
        puts("Warning: get_level(): inverse() has been performed, the coefficients has been modified and do not make sense anymore.");
        return 0;
    }
    const long long n = node_shape(depth, NULL, NULL) * (depth >= 0 && depth <= kL ? nnodes(depth) : 0);
    if (n <= 0 || !out) return 0;
    if (pdwt_memcpy_d2h(out, d_nodes[depth], (size_t)n * sizeof(DTYPE)) != PDWT_OK) return 0;
    return n;
}

int WaveletPackets1D::set_node(DTYPE* in, int depth, int idx, int mem_is_on_device)
{
    ON_MY_DEVICE_P();
    if (!(state == W_FORWARD || state == W_THRESHOLD)) {
        puts("Warning: set_node(): refused, the tree does not hold the coefficients of a forward() (run forward() first)");
        return 0;
    }
    long long pitch = 0;
    const intptr_t dst = node_int_ptr(depth, idx, &pitch);
    if (!dst || !in) return 0;
    const size_t w = (size_t)P(priv_)->n[depth] * sizeof(DTYPE);
    const int rc = pdwt_memcpy2d((void*)dst, (size_t)pitch * sizeof(DTYPE), in, w, w, (size_t)winfos.Nr, mem_is_on_device ? 3 : 0);
    if (rc != PDWT_OK) {
        report("WaveletPackets1D", "::set_node()", rc);
        return 0;
    }
    state = W_THRESHOLD;
    return (int)node_shape(depth, NULL, NULL);
}

// the four moments of every (row, node) of a depth: 4 * Nr * 2^depth doubles, segment = row * 2^depth + node
static int depth_moments(WaveletPackets1D* W, void* priv, int depth, std::vector<double>& m)
{
    const long long nseg = (long long)W->winfos.Nr * nnodes(depth);
    m.resize(4 * (size_t)nseg);
    return SFX(pdwt_wp1_moments)(W->d_nodes[depth], nseg, P(priv)->n[depth], m.data());
}

int WaveletPackets1D::node_costs(int depth, int kind, double* out, double* per_row)
{
    ON_MY_DEVICE_P();
    if (!(state == W_FORWARD || state == W_THRESHOLD) || node_shape(depth, NULL, NULL) <= 0 || !out || (kind != 0 && kind != 1)) return PDWT_EINVAL;
    std::vector<double> m;
    const int rc = depth_moments(this, priv_, depth, m);
    if (rc != PDWT_OK) {
        report("WaveletPackets1D", "::node_costs()", rc);
        return rc;
    }
    const int nn = nnodes(depth), col = kind == 0 ? 0 : 3;
    for (int i = 0; i < nn; i++) out[i] = 0.0;
    for (int r = 0; r < winfos.Nr; r++)  // over the rows in row order
        for (int i = 0; i < nn; i++) {
            const double c = m[4 * ((size_t)r * nn + i) + col];
            out[i] += c;
            if (per_row) per_row[(size_t)r * nn + i] = c;
        }
    return PDWT_OK;
}

int WaveletPackets1D::best_basis(int kind)
{
    ON_MY_DEVICE_P();
    if (state != W_FORWARD || (kind != 0 && kind != 1)) return PDWT_EINVAL;
    const int L = winfos.nlevels;
    std::vector<double> best[kL + 1];
    std::vector<unsigned char> keep[kL + 1];
    for (int l = 0; l <= L; l++) {
        best[l].resize((size_t)nnodes(l));
        if (const int rc = node_costs(l, kind, best[l].data()); rc != PDWT_OK) return rc;
        keep[l].assign((size_t)nnodes(l), 1);
    }
    for (int l = L - 1; l >= 0; l--)
        for (int i = 0; i < nnodes(l); i++) {
            const double below = best[l + 1][2 * (size_t)i] + best[l + 1][2 * (size_t)i + 1];
            if (!(best[l][i] <= below)) keep[l][i] = 0, best[l][i] = below;
        }
    std::vector<int> bd, bi, todo_d(1, 0), todo_i(1, 0);  // top-down: a node that is not kept hands over to its children
    while (!todo_d.empty()) {
        const int d = todo_d.back(), i = todo_i.back();
        todo_d.pop_back(), todo_i.pop_back();
        if (keep[d][i]) bd.push_back(d), bi.push_back(i);
        else
            for (int q = 0; q < 2; q++) todo_d.push_back(d + 1), todo_i.push_back(2 * i + q);
    }
    if (const int rc = install_basis(P(priv_), L, bd.data(), bi.data(), (int)bd.size()); rc != PDWT_OK) return rc;
    return basis_size();
}

int WaveletPackets1D::set_basis(const int* depth, const int* idx, int n)
{
    ON_MY_DEVICE_P();
    if (state == W_CREATION_ERROR || state == W_THRESHOLD || state == W_THRESHOLD_ERROR) return PDWT_EINVAL;
    return install_basis(P(priv_), winfos.nlevels, depth, idx, n);
}

int WaveletPackets1D::basis_size() const { return get_basis(NULL, NULL); }

int WaveletPackets1D::get_basis(int* depth, int* idx) const
{
    if (state == W_CREATION_ERROR) return 0;
    const wp1_priv* p = P(priv_);
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

void WaveletPackets1D::threshold(int op, DTYPE beta, int do_thresh_appcoeffs)
{
    ON_MY_DEVICE_P();
    if (state == W_INVERSE) {
        puts("Warning: WaveletPackets1D(): cannot threshold coefficients, as they were modified by W.inverse()");
        return;
    }
    if (state == W_CREATION_ERROR) return;
    wp1_priv* p = P(priv_);
    for (int l = 0; l <= winfos.nlevels; l++) {
        int any = 0;
        for (int i = (do_thresh_appcoeffs ? 0 : 1); i < nnodes(l) && !any; i++) any = p->in_basis[l][i];  // node 0 of every depth is the all-"a" path
        if (!any) continue;
        const unsigned char* flags = (do_thresh_appcoeffs ? p->d_state : p->d_thr) + toff(l);
        const int rc = SFX(pdwt_wp1_thresh)(op, d_nodes[l], winfos.Nr, nnodes(l), p->n[l], flags, beta);
        if (rc != PDWT_OK) {
            report("WaveletPackets1D", op ? "::hard_threshold()" : "::soft_threshold()", rc);
            state = W_THRESHOLD_ERROR;
            return;
        }
    }
    state = W_THRESHOLD;
}
void WaveletPackets1D::soft_threshold(DTYPE beta, int do_thresh_appcoeffs) { threshold(0, beta, do_thresh_appcoeffs); }
void WaveletPackets1D::hard_threshold(DTYPE beta, int do_thresh_appcoeffs) { threshold(1, beta, do_thresh_appcoeffs); }

double WaveletPackets1D::norm1()
{
    ON_MY_DEVICE_P();
    if (!(state == W_FORWARD || state == W_THRESHOLD)) return -1.0;
    wp1_priv* p = P(priv_);
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

int WaveletPackets1D::node_stats(int depth, w_band_stats* out)
{
    ON_MY_DEVICE_P();
    const long long n = node_shape(depth, NULL, NULL);
    if (!(state == W_FORWARD || state == W_THRESHOLD) || n <= 0 || !out) return PDWT_EINVAL;
    std::vector<double> m;
    const int rc = depth_moments(this, priv_, depth, m);
    if (rc != PDWT_OK) {
        report("WaveletPackets1D", "::node_stats()", rc);
        return rc;
    }
    const int nn = nnodes(depth);
    for (int i = 0; i < nn; i++) out[i].n = (double)n, out[i].sum_abs = 0.0, out[i].sum_sq = 0.0, out[i].max_abs = 0.0, out[i].median_abs = NAN;
    for (int r = 0; r < winfos.Nr; r++)
        for (int i = 0; i < nn; i++) {
            const double* s = &m[4 * ((size_t)r * nn + i)];
            out[i].sum_abs += s[0], out[i].sum_sq += s[1];
            if (s[2] > out[i].max_abs) out[i].max_abs = s[2];
        }
    return PDWT_OK;
}

double WaveletPackets1D::estimate_sigma()
{
    ON_MY_DEVICE_P();
    if (!(state == W_FORWARD || state == W_THRESHOLD)) return -1.0;
    wp1_priv* p = P(priv_);
    // node "d" is a strided view: gathered into a contiguous scratch by a pitched device-to-device copy, then the median of the band list
    const size_t n = (size_t)winfos.Nr * p->n[1], w = (size_t)p->n[1] * sizeof(DTYPE);
    DTYPE* tmp = (DTYPE*)pdwt_malloc(n * sizeof(DTYPE));
    if (!tmp) return -1.0;
    int rc = pdwt_memcpy2d(tmp, w, d_nodes[1] + p->n[1], 2 * w, w, (size_t)winfos.Nr, 2);
    const unsigned char want = 2;  // the median alone
    pdwt_band_stats s;
    const DTYPE* band = tmp;
    if (rc == PDWT_OK) rc = SFX(pdwt_bandlist_stats)(&band, &n, 1, &want, &s);
    pdwt_free(tmp);
    if (rc != PDWT_OK) {
        report("WaveletPackets1D", "::estimate_sigma()", rc);
        return -1.0;
    }
    return s.median_abs / 0.6744897501960817;
}

// ---- flat C handle API (pdwt_amd/wpt.py) ------------------------------------------------------------------
#define WP(h) static_cast<WaveletPackets1D*>(h)
extern "C" {
void* pdwt_wp1h_new(DTYPE* rows, int Nr, int Nc, const char* wname, int levels, int memisonhost) { return new (std::nothrow) WaveletPackets1D(rows, Nr, Nc, wname, levels, memisonhost); }
void pdwt_wp1h_delete(void* h) { delete WP(h); }
void pdwt_wp1h_forward(void* h) { WP(h)->forward(); }
void pdwt_wp1h_inverse(void* h) { WP(h)->inverse(); }
int pdwt_wp1h_fused(void* h) { return WP(h)->fused(); }
int pdwt_wp1h_get_image(void* h, DTYPE* out) { return WP(h)->get_image(out); }
void pdwt_wp1h_set_image(void* h, DTYPE* rows, int mem_is_on_device) { WP(h)->set_image(rows, mem_is_on_device); }
int pdwt_wp1h_state(void* h) { return (int)WP(h)->state; }
void pdwt_wp1h_info(void* h, w_info_wpt1* out) { *out = WP(h)->winfos; }
long long pdwt_wp1h_node_shape(void* h, int depth, int* nr, int* n) { return WP(h)->node_shape(depth, nr, n); }
int pdwt_wp1h_path_index(const char* path, int* depth) { return WaveletPackets1D::path_index(path, depth); }
int pdwt_wp1h_geometry(int Nc, int hlen, int levels, int* n) { return WaveletPackets1D::geometry(Nc, hlen, levels, n); }
int pdwt_wp1h_frequency_order(int depth, int* out) { return WaveletPackets1D::frequency_order(depth, out); }
int pdwt_wp1h_get_node(void* h, DTYPE* out, int depth, int idx) { return WP(h)->get_node(out, depth, idx); }
long long pdwt_wp1h_get_level(void* h, DTYPE* out, int depth) { return WP(h)->get_level(out, depth); }
int pdwt_wp1h_set_node(void* h, DTYPE* in, int depth, int idx, int mem_is_on_device) { return WP(h)->set_node(in, depth, idx, mem_is_on_device); }
intptr_t pdwt_wp1h_node_int_ptr(void* h, int depth, int idx, long long* pitch) { return WP(h)->node_int_ptr(depth, idx, pitch); }
int pdwt_wp1h_node_costs(void* h, int depth, int kind, double* out, double* per_row) { return WP(h)->node_costs(depth, kind, out, per_row); }
int pdwt_wp1h_best_basis(void* h, int kind) { return WP(h)->best_basis(kind); }
int pdwt_wp1h_set_basis(void* h, const int* depth, const int* idx, int n) { return WP(h)->set_basis(depth, idx, n); }
int pdwt_wp1h_basis_size(void* h) { return WP(h)->basis_size(); }
int pdwt_wp1h_get_basis(void* h, int* depth, int* idx) { return WP(h)->get_basis(depth, idx); }
void pdwt_wp1h_soft_threshold(void* h, DTYPE beta, int app) { WP(h)->soft_threshold(beta, app); }
void pdwt_wp1h_hard_threshold(void* h, DTYPE beta, int app) { WP(h)->hard_threshold(beta, app); }
double pdwt_wp1h_norm1(void* h) { return WP(h)->norm1(); }
int pdwt_wp1h_node_stats(void* h, int depth, w_band_stats* out) { return WP(h)->node_stats(depth, out); }
double pdwt_wp1h_estimate_sigma(void* h) { return WP(h)->estimate_sigma(); }
}
#undef WP
