// wptb.cpp -- host side of `WaveletPacketsImages` (include/wpt_batch.h) above the batched packet entry points of include/pdwt_hip.h, and
// its flat C handle API (pdwt_wpbh_*, the shape of wpt.cpp).  Plain host C++, built into libpdwt.so (float) and libpdwtd.so
// (-DDOUBLEPRECISION).  The basis (flags per depth, the state table of the inverse and the chunk lists of its per-depth form, both
// uploaded when a basis is installed), the best-basis search over the summed costs and the per-image bookkeeping live here; the device
// sees whole transforms (pdwt_wptb_*), costs over chunks of forest nodes, and the batched statistics / threshold entries over a table of
// node pointers that is built on first use.
#include <limits.h>
#include <new>
#include <string.h>
#include <vector>

#include "../../include/wpt_batch.h"
#include "host_common.hpp"

static_assert(sizeof(w_band_stats) == sizeof(pdwt_band_stats), "w_band_stats must mirror pdwt_band_stats");

namespace {
constexpr int kL = WPT_MAX_LEVELS;
constexpr int kCostChunk = 65535;  // nodes per pdwt_wpt2d_node_cost call
inline int nnodes(int depth) { return 1 << (2 * depth); }
inline int state_off(int depth) { return (nnodes(depth) - 1) / 3; }

struct wpb_priv {
    filters_t f;
    int dev;  // the device current at construction; every method runs there
    int B, allow_fused, fused;
    int nr[kL + 1], nc[kL + 1];
    std::vector<unsigned char> in_basis[kL + 1];  // per depth: 1 = the node belongs to the basis
    std::vector<unsigned char> state;             // the state table of the inverse (pdwt_wptb_state_table)
    unsigned char* d_state;                       // device: its copy (the fused form)
    int* d_lists;                                 // device: pdwt_wptb_chunk_lists of it (the per-depth form), or NULL
    DTYPE** d_ptr;                                // device: the pointers of every (image, node), depth l at ptr_off[l]; built on first use
    size_t ptr_off[kL + 2];
};
inline wpb_priv* P(void* p) { return (wpb_priv*)p; }

// flags per depth from a list of nodes; false unless the nodes partition the tree
bool flags_from_nodes(int L, const int* depth, const int* idx, int n, std::vector<unsigned char>* flags)
{
    std::vector<unsigned char> st((size_t)state_off(L + 1));
    if (pdwt_wptb_state_table(L, depth, idx, n, st.data()) != PDWT_OK) return false;
    for (int l = 0; l <= L; l++) {
        flags[l].assign((size_t)nnodes(l), 0);
        for (int i = 0; i < nnodes(l); i++) flags[l][i] = st[state_off(l) + i] == 1;
    }
    return true;
}
}  // namespace
#define ON_MY_DEVICE_B() DevScope dev_scope_(priv_ ? ((const wpb_priv*)priv_)->dev : -1)

// install flags (a valid partition): the state table on the host and the device, the chunk lists of the per-depth form
static int install_basis(wpb_priv* p, int L, std::vector<unsigned char>* flags)
{
    std::vector<int> d, i;
    for (int l = 0; l <= L; l++)
        for (int k = 0; k < nnodes(l); k++)
            if (flags[l][k]) d.push_back(l), i.push_back(k);
    std::vector<unsigned char> st((size_t)state_off(L + 1));
    if (pdwt_wptb_state_table(L, d.data(), i.data(), (int)d.size(), st.data()) != PDWT_OK) return PDWT_EINVAL;
    int rc = pdwt_memcpy_h2d(p->d_state, st.data(), st.size());
    if (rc != PDWT_OK) return rc;
    if (p->d_lists && st[0] == 2) {
        const long long n = pdwt_wptb_chunk_lists(p->B, L, st.data(), NULL);
        if (n < 0) return (int)n;
        std::vector<int> lists((size_t)n, 0);
        pdwt_wptb_chunk_lists(p->B, L, st.data(), lists.data());
        rc = pdwt_memcpy_h2d(p->d_lists, lists.data(), lists.size() * sizeof(int));
        if (rc != PDWT_OK) return rc;
    }
    p->state.swap(st);
    for (int l = 0; l <= L; l++) p->in_basis[l] = flags[l];
    return PDWT_OK;
}

// the device table of node pointers (B 4^l pointers per depth, forest order), built when a statistic or a threshold first asks for it
static int need_ptr_table(wpb_priv* p, DTYPE* const* d_nodes, int L)
{
    if (p->d_ptr) return PDWT_OK;
    p->d_ptr = (DTYPE**)pdwt_malloc(p->ptr_off[L + 1] * sizeof(DTYPE*));
    if (!p->d_ptr) return PDWT_ENOMEM;
    std::vector<DTYPE*> tab(p->ptr_off[L + 1]);
    for (int l = 0; l <= L; l++) {
        const size_t per = (size_t)p->nr[l] * p->nc[l], n = (size_t)p->B * nnodes(l);
        for (size_t g = 0; g < n; g++) tab[p->ptr_off[l] + g] = d_nodes[l] + g * per;
    }
    const int rc = pdwt_memcpy_h2d(p->d_ptr, tab.data(), tab.size() * sizeof(DTYPE*));
    if (rc != PDWT_OK) {
        pdwt_free(p->d_ptr);
        p->d_ptr = NULL;
    }
    return rc;
}

int WaveletPacketsImages::geometry(int Nr, int Nc, int hlen, int levels, int* nr, int* nc) { return WaveletPackets::geometry(Nr, Nc, hlen, levels, nr, nc); }
int WaveletPacketsImages::path_index(const char* path, int* depth) { return WaveletPackets::path_index(path, depth); }

WaveletPacketsImages::WaveletPacketsImages(DTYPE* imgs, int B, int Nr, int Nc, const char* wname_, int levels, int memisonhost, int allow_fused)
    : d_image(NULL), state(W_INIT), priv_(NULL)
{
    for (int l = 0; l <= kL; l++) d_nodes[l] = NULL;
    winfos.B = B, winfos.Nr = Nr, winfos.Nc = Nc, winfos.nlevels = levels, winfos.hlen = 0;
    strncpy(wname, wname_ ? wname_ : "", 127);
    wname[127] = 0;
    if (Nr < 1 || Nc < 1 || !wname_ || (unsigned long long)Nr * (unsigned long long)Nc >= (1ull << 31)) {
        puts("ERROR: WaveletPacketsImages(): invalid image size or wavelet name");
        state = W_CREATION_ERROR;
        return;
    }
    if (B < 1 || B > 65535) {
        printf("ERROR: WaveletPacketsImages(): a batch holds 1 .. 65535 images (%d given)\n", B);
        state = W_CREATION_ERROR;
        return;
    }
    if (levels < 1) {
        puts("Warning: cannot initialize wavelet coefficients with nlevels < 1. Forcing nlevels = 1");
        winfos.nlevels = 1;
    }
    wpb_priv* p = new (std::nothrow) wpb_priv();
    if (!p) {
        state = W_CREATION_ERROR;
        return;
    }
    priv_ = p;
    p->d_ptr = NULL, p->d_lists = NULL, p->d_state = NULL;
    p->dev = -1;
    p->B = B, p->allow_fused = allow_fused ? 1 : 0, p->fused = 0;
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
    if ((long long)B * nnodes(L) > (1ll << 22)) {
        printf("ERROR: WaveletPacketsImages(): %d images of %d nodes exceed 2^22 nodes per depth\n", B, nnodes(L));
        state = W_CREATION_ERROR;
        return;
    }
    p->dev = pdwt_get_device();
    p->fused = p->allow_fused && pdwt_wptb_fused(Nr, Nc, hlen, L, (int)sizeof(DTYPE)) == 1;
    p->ptr_off[0] = 0;
    for (int l = 0; l <= L; l++) p->ptr_off[l + 1] = p->ptr_off[l] + (size_t)B * nnodes(l);
    int rc = PDWT_OK;
    for (int l = 0; l <= L && rc == PDWT_OK; l++) {
        const size_t nb = (size_t)B * nnodes(l) * p->nr[l] * p->nc[l] * sizeof(DTYPE);
        d_nodes[l] = (DTYPE*)pdwt_malloc(nb);
        if (!d_nodes[l]) rc = PDWT_ENOMEM;
        else if (l > 0) rc = pdwt_memset(d_nodes[l], 0, nb);
    }
    d_image = d_nodes[0];
    if (rc == PDWT_OK) {
        p->d_state = (unsigned char*)pdwt_malloc((size_t)state_off(L + 1));
        const long long nl = pdwt_wptb_tmp_elems(B, Nr, Nc, hlen, L, (int)sizeof(DTYPE), p->allow_fused);
        if (nl > 0) p->d_lists = (int*)pdwt_malloc((size_t)nl * sizeof(int));
        if (!p->d_state || nl < 0 || (nl > 0 && !p->d_lists)) rc = nl < 0 ? PDWT_EINVAL : PDWT_ENOMEM;
    }
    if (rc == PDWT_OK) {  // the default basis: every node of depth L
        std::vector<unsigned char> flags[kL + 1];
        for (int l = 0; l <= L; l++) flags[l].assign((size_t)nnodes(l), l == L ? 1 : 0);
        rc = install_basis(p, L, flags);
    }
    if (rc == PDWT_OK) {
        const size_t n = (size_t)B * Nr * Nc;
        if (!imgs) rc = pdwt_memset(d_image, 0, n * sizeof(DTYPE));
        else if (memisonhost) rc = pdwt_memcpy_h2d(d_image, imgs, n * sizeof(DTYPE));
        else rc = pdwt_memcpy_d2d_foreign(d_image, imgs, n * sizeof(DTYPE));
    }
    if (rc != PDWT_OK) {
        report("WaveletPacketsImages", "(): allocation or upload", rc);
        state = W_CREATION_ERROR;
    }
}

WaveletPacketsImages::~WaveletPacketsImages()
{
    ON_MY_DEVICE_B();
    for (int l = 0; l <= kL; l++)
        if (d_nodes[l]) pdwt_free(d_nodes[l]);
    if (priv_) {
        if (P(priv_)->d_ptr) pdwt_free(P(priv_)->d_ptr);
        if (P(priv_)->d_lists) pdwt_free(P(priv_)->d_lists);
        if (P(priv_)->d_state) pdwt_free(P(priv_)->d_state);
        delete P(priv_);
    }
}

int WaveletPacketsImages::fused() const { return state != W_CREATION_ERROR && priv_ ? P(priv_)->fused : 0; }

void WaveletPacketsImages::forward()
{
    ON_MY_DEVICE_B();
    if (state == W_CREATION_ERROR) {
        puts("Warning: forward transform not computed, as there was an error when creating the wavelets");
        return;
    }
    wpb_priv* p = P(priv_);
    const int rc = SFX(pdwt_wptb_forward)(d_image, d_nodes + 1, p->B, winfos.Nr, winfos.Nc, winfos.nlevels, &p->f, p->allow_fused);
    if (rc < 0) {
        report("WaveletPacketsImages", "::forward()", rc);
        state = W_FORWARD_ERROR;
        return;
    }
    state = W_FORWARD;
}

void WaveletPacketsImages::inverse()
{
    ON_MY_DEVICE_B();
    if (state == W_INVERSE) {
        puts("Warning: W.inverse() has already been run. Inverse is available in W.get_image()");
        return;
    }
    if (state == W_CREATION_ERROR || state == W_FORWARD_ERROR || state == W_THRESHOLD_ERROR) {
        puts("Warning: inverse transform not computed, as there was an error in a previous stage");
        return;
    }
    wpb_priv* p = P(priv_);
    if (p->state[0] == 2) {  // (a basis of the root alone: the images are the coefficients)
        const int rc = SFX(pdwt_wptb_inverse)(d_image, d_nodes + 1, p->B, winfos.Nr, winfos.Nc, winfos.nlevels, p->state.data(), p->d_state, p->d_lists, &p->f, p->allow_fused);
        if (rc < 0) {
            report("WaveletPacketsImages", "::inverse()", rc);
            state = W_INVERSE_ERROR;
            return;
        }
    }
    state = W_INVERSE;
}

long long WaveletPacketsImages::get_image(DTYPE* res)
{
    ON_MY_DEVICE_B();
    if (!d_image || !res || state == W_CREATION_ERROR) return 0;
    const size_t n = (size_t)winfos.B * winfos.Nr * winfos.Nc;
    if (pdwt_memcpy_d2h(res, d_image, n * sizeof(DTYPE)) != PDWT_OK) return 0;
    return (long long)n;
}

void WaveletPacketsImages::set_image(DTYPE* imgs, int mem_is_on_device)
{
    ON_MY_DEVICE_B();
    if (!d_image || !imgs || state == W_CREATION_ERROR) return;
    const size_t nb = (size_t)winfos.B * winfos.Nr * winfos.Nc * sizeof(DTYPE);
    const int rc = mem_is_on_device ? pdwt_memcpy_d2d_foreign(d_image, imgs, nb) : pdwt_memcpy_h2d(d_image, imgs, nb);
    if (rc != PDWT_OK) report("WaveletPacketsImages", "::set_image()", rc);
    state = W_INIT;
}

long long WaveletPacketsImages::node_shape(int depth, int* nr, int* nc) const
{
    if (state == W_CREATION_ERROR || depth < 0 || depth > winfos.nlevels) return 0;
    const wpb_priv* p = P(priv_);
    if (nr) *nr = p->nr[depth];
    if (nc) *nc = p->nc[depth];
    return (long long)p->nr[depth] * p->nc[depth];
}

long long WaveletPacketsImages::get_node(DTYPE* out, int depth, int idx)
{
    ON_MY_DEVICE_B();
    if (state == W_INVERSE) {
        puts("Warning: get_node(): inverse() has been performed, the coefficients has been modified and do not make sense anymore.");
        return 0;
    }
    const long long n = node_shape(depth, NULL, NULL);
    if (n <= 0 || !out || idx < 0 || idx >= nnodes(depth)) return 0;
    const size_t w = (size_t)n * sizeof(DTYPE);
    if (pdwt_memcpy2d(out, w, d_nodes[depth] + (size_t)idx * n, w * nnodes(depth), w, (size_t)winfos.B, 1) != PDWT_OK) return 0;
    return n * winfos.B;
}

long long WaveletPacketsImages::get_level(DTYPE* out, int depth)
{
    ON_MY_DEVICE_B();
    if (state == W_INVERSE) {
        puts("Warning: get_level(): inverse() has been performed, the coefficients has been modified and do not make sense anymore.");
        return 0;
    }
    const long long n = node_shape(depth, NULL, NULL) * (depth >= 0 && depth <= kL ? nnodes(depth) : 0) * winfos.B;
    if (n <= 0 || !out) return 0;
    if (pdwt_memcpy_d2h(out, d_nodes[depth], (size_t)n * sizeof(DTYPE)) != PDWT_OK) return 0;
    return n;
}

long long WaveletPacketsImages::set_node(DTYPE* in, int depth, int idx, int mem_is_on_device)
{
    ON_MY_DEVICE_B();
    if (!(state == W_FORWARD || state == W_THRESHOLD)) {
        puts("Warning: set_node(): refused, the tree does not hold the coefficients of a forward() (run forward() first)");
        return 0;
    }
    const long long n = node_shape(depth, NULL, NULL);
    if (n <= 0 || !in || idx < 0 || idx >= nnodes(depth)) return 0;
    const size_t w = (size_t)n * sizeof(DTYPE);
    const int rc = pdwt_memcpy2d(d_nodes[depth] + (size_t)idx * n, w * nnodes(depth), in, w, w, (size_t)winfos.B, mem_is_on_device ? 3 : 0);
    if (rc != PDWT_OK) {
        report("WaveletPacketsImages", "::set_node()", rc);
        return 0;
    }
    state = W_THRESHOLD;
    return n * winfos.B;
}

intptr_t WaveletPacketsImages::node_int_ptr(int depth, int idx, long long* pitch)
{
    const long long n = node_shape(depth, NULL, NULL);
    if (n <= 0 || idx < 0 || idx >= nnodes(depth)) return 0;
    if (pitch) *pitch = n * nnodes(depth);
    return (intptr_t)(d_nodes[depth] + (size_t)idx * n);
}

int WaveletPacketsImages::node_costs(int depth, int kind, double* per_image, double* summed)
{
    ON_MY_DEVICE_B();
    const long long n = node_shape(depth, NULL, NULL);
    if (!(state == W_FORWARD || state == W_THRESHOLD) || n <= 0 || (!per_image && !summed)) return PDWT_EINVAL;
    const int nn = nnodes(depth);
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

int WaveletPacketsImages::best_basis(int kind)
{
    ON_MY_DEVICE_B();
    if (state != W_FORWARD || (kind != 0 && kind != 1)) return PDWT_EINVAL;
    const int L = winfos.nlevels;
    std::vector<double> best[kL + 1];
    std::vector<unsigned char> keep[kL + 1], flags[kL + 1];
    for (int l = 0; l <= L; l++) {
        best[l].resize((size_t)nnodes(l));
        if (const int rc = node_costs(l, kind, NULL, best[l].data()); rc != PDWT_OK) return rc;
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

int WaveletPacketsImages::set_basis(const int* depth, const int* idx, int n)
{
    ON_MY_DEVICE_B();
    if (state == W_CREATION_ERROR || state == W_THRESHOLD || state == W_THRESHOLD_ERROR) return PDWT_EINVAL;
    std::vector<unsigned char> flags[kL + 1];
    if (!flags_from_nodes(winfos.nlevels, depth, idx, n, flags)) return PDWT_EINVAL;
    return install_basis(P(priv_), winfos.nlevels, flags);
}

int WaveletPacketsImages::basis_size() const { return get_basis(NULL, NULL); }

int WaveletPacketsImages::get_basis(int* depth, int* idx) const
{
    if (state == W_CREATION_ERROR) return 0;
    const wpb_priv* p = P(priv_);
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

void WaveletPacketsImages::threshold(int op, DTYPE beta, int do_thresh_appcoeffs)
{
    ON_MY_DEVICE_B();
    if (state == W_INVERSE) {
        puts("Warning: WaveletPacketsImages(): cannot threshold coefficients, as they were modified by W.inverse()");
        return;
    }
    if (state == W_CREATION_ERROR) return;
    wpb_priv* p = P(priv_);
    int rc = need_ptr_table(p, d_nodes, winfos.nlevels);
    std::vector<DTYPE> betas;
    for (int l = 0; l <= winfos.nlevels && rc == PDWT_OK; l++) {
        const int nn = nnodes(l);
        int any = 0;
        for (int i = (do_thresh_appcoeffs ? 0 : 1); i < nn && !any; i++) any = p->in_basis[l][i];  // node 0 of every depth is the all-"a" path
        if (!any) continue;
        betas.assign((size_t)p->B * nn, (DTYPE)-1);
        for (int i = (do_thresh_appcoeffs ? 0 : 1); i < nn; i++)
            if (p->in_basis[l][i])
                for (int b = 0; b < p->B; b++) betas[(size_t)b * nn + i] = beta;
        const size_t n = (size_t)p->nr[l] * p->nc[l];
        rc = SFX(pdwt_bandbatch_thresh)(op, p->d_ptr + p->ptr_off[l], &n, betas.data(), p->B * nn, 1);
    }
    if (rc != PDWT_OK) {
        report("WaveletPacketsImages", op ? "::hard_threshold()" : "::soft_threshold()", rc);
        state = W_THRESHOLD_ERROR;
        return;
    }
    state = W_THRESHOLD;
}
void WaveletPacketsImages::soft_threshold(DTYPE beta, int do_thresh_appcoeffs) { threshold(0, beta, do_thresh_appcoeffs); }
void WaveletPacketsImages::hard_threshold(DTYPE beta, int do_thresh_appcoeffs) { threshold(1, beta, do_thresh_appcoeffs); }

int WaveletPacketsImages::images_norm1(double* out)
{
    ON_MY_DEVICE_B();
    if (!(state == W_FORWARD || state == W_THRESHOLD) || !out) return PDWT_EINVAL;
    wpb_priv* p = P(priv_);
    std::vector<double> c;
    for (int b = 0; b < p->B; b++) out[b] = 0.0;
    for (int l = 0; l <= winfos.nlevels; l++) {
        const int nn = nnodes(l);
        int any = 0;
        for (int i = 0; i < nn && !any; i++) any = p->in_basis[l][i];
        if (!any) continue;
        c.resize((size_t)p->B * nn);
        if (const int rc = node_costs(l, 0, c.data(), NULL); rc != PDWT_OK) return rc;
        for (int b = 0; b < p->B; b++)
            for (int i = 0; i < nn; i++)
                if (p->in_basis[l][i]) out[b] += c[(size_t)b * nn + i];
    }
    return PDWT_OK;
}

double WaveletPacketsImages::norm1()
{
    if (!(state == W_FORWARD || state == W_THRESHOLD)) return -1.0;
    std::vector<double> per((size_t)winfos.B);
    if (images_norm1(per.data()) != PDWT_OK) return -1.0;
    double sum = 0.0;
    for (int b = 0; b < winfos.B; b++) sum += per[b];
    return sum;
}

int WaveletPacketsImages::node_stats(int depth, w_band_stats* out)
{
    ON_MY_DEVICE_B();
    const long long n = node_shape(depth, NULL, NULL);
    if (!(state == W_FORWARD || state == W_THRESHOLD) || n <= 0 || !out) return PDWT_EINVAL;
    wpb_priv* p = P(priv_);
    int rc = need_ptr_table(p, d_nodes, winfos.nlevels);
    const size_t ne = (size_t)n;
    if (rc == PDWT_OK) rc = SFX(pdwt_bandbatch_stats)(p->d_ptr + p->ptr_off[depth], &ne, p->B * nnodes(depth), 1, NULL, reinterpret_cast<pdwt_band_stats*>(out));
    if (rc != PDWT_OK) report("WaveletPacketsImages", "::node_stats()", rc);
    return rc;
}

double WaveletPacketsImages::estimate_sigma()
{
    ON_MY_DEVICE_B();
    if (!(state == W_FORWARD || state == W_THRESHOLD)) return -1.0;
    wpb_priv* p = P(priv_);
    // node "d" of every image, gathered into one run: the median is over the union
    const size_t n = (size_t)p->nr[1] * p->nc[1], w = n * sizeof(DTYPE), all = n * p->B;
    DTYPE* pool = (DTYPE*)pdwt_malloc(all * sizeof(DTYPE));
    if (!pool) return -1.0;
    int rc = pdwt_memcpy2d(pool, w, d_nodes[1] + 3 * n, 4 * w, w, (size_t)p->B, 2);
    pdwt_band_stats s;
    const unsigned char want = 2;  // the median alone
    const DTYPE* cp = pool;
    if (rc == PDWT_OK) rc = SFX(pdwt_bandlist_stats)(&cp, &all, 1, &want, &s);  // (synchronises)
    const int rf = pdwt_free(pool);
    if (rc != PDWT_OK || rf != PDWT_OK) {
        report("WaveletPacketsImages", "::estimate_sigma()", rc != PDWT_OK ? rc : rf);
        return -1.0;
    }
    return s.median_abs / 0.6744897501960817;
}

int WaveletPacketsImages::images_estimate_sigma(double* out)
{
    ON_MY_DEVICE_B();
    if (!(state == W_FORWARD || state == W_THRESHOLD) || !out) return PDWT_EINVAL;
    wpb_priv* p = P(priv_);
    const size_t n = (size_t)p->nr[1] * p->nc[1];
    std::vector<DTYPE*> tab((size_t)p->B);
    for (int b = 0; b < p->B; b++) tab[b] = d_nodes[1] + ((size_t)4 * b + 3) * n;  // node "d" of image b
    DTYPE** d_tab = (DTYPE**)pdwt_malloc(tab.size() * sizeof(DTYPE*));
    if (!d_tab) return PDWT_ENOMEM;
    std::vector<pdwt_band_stats> s((size_t)p->B);
    const unsigned char want = 2;
    int rc = pdwt_memcpy_h2d(d_tab, tab.data(), tab.size() * sizeof(DTYPE*));
    if (rc == PDWT_OK) rc = SFX(pdwt_bandbatch_stats)(d_tab, &n, p->B, 1, &want, s.data());  // (synchronises)
    const int rf = pdwt_free(d_tab);
    if (rc != PDWT_OK || rf != PDWT_OK) {
        report("WaveletPacketsImages", "::images_estimate_sigma()", rc != PDWT_OK ? rc : rf);
        return rc != PDWT_OK ? rc : rf;
    }
    for (int b = 0; b < p->B; b++) out[b] = s[b].median_abs / 0.6744897501960817;
    return PDWT_OK;
}

// ---- flat C handle API (pdwt_amd/wpt.py) ------------------------------------------------------------------
#define WB(h) static_cast<WaveletPacketsImages*>(h)
extern "C" {
void* pdwt_wpbh_new(DTYPE* imgs, int B, int Nr, int Nc, const char* wname, int levels, int memisonhost, int allow_fused)
{
    return new (std::nothrow) WaveletPacketsImages(imgs, B, Nr, Nc, wname, levels, memisonhost, allow_fused);
}
void pdwt_wpbh_delete(void* h) { delete WB(h); }
void pdwt_wpbh_forward(void* h) { WB(h)->forward(); }
void pdwt_wpbh_inverse(void* h) { WB(h)->inverse(); }
int pdwt_wpbh_fused(void* h) { return WB(h)->fused(); }
long long pdwt_wpbh_get_image(void* h, DTYPE* out) { return WB(h)->get_image(out); }
void pdwt_wpbh_set_image(void* h, DTYPE* imgs, int mem_is_on_device) { WB(h)->set_image(imgs, mem_is_on_device); }
int pdwt_wpbh_state(void* h) { return (int)WB(h)->state; }
void pdwt_wpbh_info(void* h, w_info_wptb* out) { *out = WB(h)->winfos; }
long long pdwt_wpbh_node_shape(void* h, int depth, int* nr, int* nc) { return WB(h)->node_shape(depth, nr, nc); }
int pdwt_wpbh_path_index(const char* path, int* depth) { return WaveletPacketsImages::path_index(path, depth); }
int pdwt_wpbh_geometry(int Nr, int Nc, int hlen, int levels, int* nr, int* nc) { return WaveletPacketsImages::geometry(Nr, Nc, hlen, levels, nr, nc); }
long long pdwt_wpbh_get_node(void* h, DTYPE* out, int depth, int idx) { return WB(h)->get_node(out, depth, idx); }
long long pdwt_wpbh_get_level(void* h, DTYPE* out, int depth) { return WB(h)->get_level(out, depth); }
long long pdwt_wpbh_set_node(void* h, DTYPE* in, int depth, int idx, int mem_is_on_device) { return WB(h)->set_node(in, depth, idx, mem_is_on_device); }
intptr_t pdwt_wpbh_node_int_ptr(void* h, int depth, int idx, long long* pitch) { return WB(h)->node_int_ptr(depth, idx, pitch); }
int pdwt_wpbh_node_costs(void* h, int depth, int kind, double* per_image, double* summed) { return WB(h)->node_costs(depth, kind, per_image, summed); }
int pdwt_wpbh_best_basis(void* h, int kind) { return WB(h)->best_basis(kind); }
int pdwt_wpbh_set_basis(void* h, const int* depth, const int* idx, int n) { return WB(h)->set_basis(depth, idx, n); }
int pdwt_wpbh_basis_size(void* h) { return WB(h)->basis_size(); }
int pdwt_wpbh_get_basis(void* h, int* depth, int* idx) { return WB(h)->get_basis(depth, idx); }
void pdwt_wpbh_soft_threshold(void* h, DTYPE beta, int app) { WB(h)->soft_threshold(beta, app); }
void pdwt_wpbh_hard_threshold(void* h, DTYPE beta, int app) { WB(h)->hard_threshold(beta, app); }
double pdwt_wpbh_norm1(void* h) { return WB(h)->norm1(); }
int pdwt_wpbh_images_norm1(void* h, double* out) { return WB(h)->images_norm1(out); }
int pdwt_wpbh_node_stats(void* h, int depth, w_band_stats* out) { return WB(h)->node_stats(depth, out); }
double pdwt_wpbh_estimate_sigma(void* h) { return WB(h)->estimate_sigma(); }
int pdwt_wpbh_images_estimate_sigma(void* h, double* out) { return WB(h)->images_estimate_sigma(out); }
}
#undef WB
