// wt_ext.cpp -- host side of the four boundary-mode classes of include/wt_ext.h, `BoundaryWavelets` (2-D), `BoundaryWavelets1D` (the
// last axis of a batch of rows), `BoundaryWavelets3D` (volumes) and `BoundaryWaveletsImages` (every image of a batch), above the
// "... with boundary modes" entry points of include/pdwt_hip.h, and their flat C handle APIs (pdwt_bw_*, pdwt_bw1_*, pdwt_bw3_*,
// pdwt_bwb_*: pdwt_amd/boundary.py).  Every method is written
// once, on their base `BoundaryTransform`; what differs between the classes is one `bw_ops` table each, and of code only the scratch
// and the walk over the levels.  Plain host C++ like wt.cpp, built into libpdwt.so (float) and libpdwtd.so (-DDOUBLEPRECISION).  The
// geometry and the band table live here; thresholds, norms and statistics go through the band-list entries (bandstats_host.hpp): no
// kernels of its own.
#include <limits.h>
#include <new>
#include <string.h>

#include "../../include/wt_ext.h"
#include "bandstats_host.hpp"
#include "host_common.hpp"

static_assert(3 * BW_MAX_LEVELS + 1 == pdwt_bl::kMaxBands, "the level clamp is the band limit of the band-list kernels");
static_assert(7 * BW3_MAX_LEVELS + 1 <= pdwt_bl::kMaxBands, "the level clamp stays within the band limit of the band-list kernels");
static_assert(BW3_MAX_LEVELS <= BW_MAX_LEVELS, "one geometry table serves the three classes");

namespace {
constexpr int kL = BW_MAX_LEVELS;
const char* const kModeNames[BW_NUM_MODES] = {"zero", "constant", "symmetric", "reflect", "periodic"};

// Sizes are {z, r, c} throughout; a class with fewer axes has 1 in front.  The LAST naxes of them are transformed.
struct bw_priv {
    filters_t f;
    int dev;           // the device current at construction; every method runs there
    int L, mode;       // winfos.nlevels after clamping, winfos.mode
    int n[3][kL + 1];  // per axis: [0] the input, [l] the bands of level l (an axis that is not transformed keeps its size)
    int fused;         // 1-D, batch: the transforms of this instance are one launch each
    DTYPE* d_bands;    // the one allocation behind d_coeffs
    DTYPE* d_tmp[2];   // the scratch of the level walk (see the three walks below); NULL where the walk needs none
    long long approx_off;  // 3-D: where the approximation of the levels 1 .. L-1 lies in d_tmp[0]
    void* d_tab;       // batch: the device table of the B * nb per-image band pointers of the images_* methods, built on first use
};
inline bw_priv* P(void* p) { return (bw_priv*)p; }
}  // namespace

// What one class contributes to the shared one: its name and nouns in messages, its band order, and its scratch and level walk.
struct bw_ops {
    const char* name;
    int naxes;             // transformed axes
    int max_levels;
    int per_level;         // detail bands of a level.  Bands: [A_L, then the levels]
    bool coarsest_first;   // ... level L first (3-D, the order of Wavelets3D) or level 1 first (the order of Wavelets)
    const char* noun;      // "invalid <noun> size or wavelet name"
    const char* size_fmt;  // the transformed sizes in the clamp messages
    const char* too_small;
    const char* unsupported;  // 3-D: the message of its separate size check (both places), NULL: the class has none
    int (*alloc_scratch)(bw_priv*, int rc);  // after the image and the bands, whose result is rc: the scratch of the walk; the new rc
    int (*forward)(BoundaryTransform&, bw_priv*);  // all levels; PDWT_OK or the code of the entry that failed
    int (*inverse)(BoundaryTransform&, bw_priv*);
    int max_batch;  // the batch of images: the largest dims[0] (part of the size check); 0: dims[0] is no batch
};

namespace {
// level (1 = finest) of band num
inline int band_level(const bw_ops& o, int L, int num)
{
    if (num == 0) return L;
    return o.coarsest_first ? L - (num - 1) / o.per_level : (num - 1) / o.per_level + 1;
}

long long shape_of(const bw_ops& o, const bw_priv* p, int num, int* shape)
{
    const int l = band_level(o, p->L, num);
    for (int a = 0; a < 3 && shape; a++) shape[a] = p->n[a][l];
    return (long long)p->n[0][l] * p->n[1][l] * p->n[2][l];
}

// the size limits of the 3-D level entries alone (Nz <= 65535, Nr * Nc < 2^31): a Haar level has no minimum length
inline bool volume_ok(const int* d) { return pdwt_num_bands_ext3d(d[0], d[1], d[2], 2, 1) > 0; }

// The levels an input of dims gets and, in out[a] where given, the size of axis a at level 0 .. that level: the rule of Wavelets
// (src/wt.cu:155-165) = PyWavelets' dwt_max_level over the transformed axes.  The size checks are the caller's.
int levels_and_sizes(const bw_ops& o, const int* dims, int hlen, int levels, int* const* out)
{
    if (hlen < 2 || hlen > PDWT_MAX_FILTER_WIDTH || (hlen & 1)) return 0;
    if (levels < 1) levels = 1;
    int N[3] = {dims[0], dims[1], dims[2]}, nmin = dims[2];
    for (int a = 3 - o.naxes; a < 3; a++) nmin = N[a] < nmin ? N[a] : nmin;
    int wmaxlev = w_ilog2(nmin / (hlen - 1));
    if (wmaxlev > o.max_levels) wmaxlev = o.max_levels;
    if (levels > wmaxlev) levels = wmaxlev;
    for (int l = 0; l <= levels; l++)
        for (int a = 0; a < 3; a++) {
            if (out[a]) out[a][l] = N[a];
            if (a >= 3 - o.naxes) N[a] = (N[a] + hlen - 1) >> 1;
        }
    return levels;
}

// ---- the scratch and the level walk of each class --------------------------------------------------------------------------------
// 2-D.  Two buffers of level-1 size for the intermediate approximations (levels 1 .. L-1), none for one level.  The approximation of
// level l is band 0 for l == L, else a buffer: level l is written from level l - 1 (forward) or read to rebuild it (inverse), so
// consecutive levels alternate between the two and neither direction touches a band it reads.
int alloc2(bw_priv* p, int rc)
{
    if (rc != PDWT_OK || p->L <= 1) return rc;
    const size_t n1 = (size_t)p->n[1][1] * p->n[2][1];
    p->d_tmp[0] = (DTYPE*)pdwt_malloc(n1 * sizeof(DTYPE));
    p->d_tmp[1] = (DTYPE*)pdwt_malloc(n1 * sizeof(DTYPE));
    return p->d_tmp[0] && p->d_tmp[1] ? PDWT_OK : PDWT_ENOMEM;
}
DTYPE* approx2(BoundaryTransform& W, bw_priv* p, int l) { return l == p->L ? W.d_coeffs[0] : p->d_tmp[(l - 1) & 1]; }

int forward2(BoundaryTransform& W, bw_priv* p)
{
    const DTYPE* src = W.d_image;
    for (int l = 1; l <= p->L; l++) {
        DTYPE* a = approx2(W, p, l);
        DTYPE** b = W.d_coeffs + 3 * (l - 1) + 1;
        const int rc = SFX(pdwt_ext2d_forward_level)(src, a, b[0], b[1], b[2], p->n[1][l - 1], p->n[2][l - 1], p->mode, &p->f);
        if (rc != PDWT_OK) return rc;
        src = a;
    }
    return PDWT_OK;
}

int inverse2(BoundaryTransform& W, bw_priv* p)
{
    for (int l = p->L; l >= 1; l--) {
        DTYPE* dst = l == 1 ? W.d_image : approx2(W, p, l - 1);
        DTYPE** b = W.d_coeffs + 3 * (l - 1) + 1;
        const int rc = SFX(pdwt_ext2d_inverse_level)(dst, approx2(W, p, l), b[0], b[1], b[2], p->n[1][l - 1], p->n[2][l - 1], &p->f);
        if (rc != PDWT_OK) return rc;
    }
    return PDWT_OK;
}

// 1-D.  The whole-transform entries choose between the one-launch kernels and the per-level loop, and say which ran (PDWT_EXT1D_FUSED
// is 1): only a negative value is an error.  The scratch is that of the loop, sized by the library (a size it refuses counts as
// PDWT_ENOMEM); a fused instance or one level has none.
int alloc1(bw_priv* p, int rc)
{
    const long long ntmp = pdwt_ext1d_tmp_elems(p->n[1][0], p->n[2][0], p->f.hlen, p->L, (int)sizeof(DTYPE));
    p->fused = pdwt_ext1d_fused(p->n[2][0], p->f.hlen, p->L, (int)sizeof(DTYPE)) == 1;
    if (ntmp < 0) return PDWT_ENOMEM;
    if (rc != PDWT_OK || ntmp == 0) return rc;
    p->d_tmp[0] = (DTYPE*)pdwt_malloc((size_t)ntmp * sizeof(DTYPE));
    return p->d_tmp[0] ? PDWT_OK : PDWT_ENOMEM;
}
int forward1(BoundaryTransform& W, bw_priv* p)
{
    const int rc = SFX(pdwt_ext1d_forward)(W.d_image, W.d_coeffs, p->n[1][0], p->n[2][0], p->L, p->mode, &p->f, p->d_tmp[0]);
    return rc < 0 ? rc : PDWT_OK;
}
int inverse1(BoundaryTransform& W, bw_priv* p)
{
    const int rc = SFX(pdwt_ext1d_inverse)(W.d_image, W.d_coeffs, p->n[1][0], p->n[2][0], p->L, &p->f, p->d_tmp[0]);
    return rc < 0 ? rc : PDWT_OK;
}

// 3-D.  One scratch, [the four x-y quadrants | the approximation of the levels 1 .. L-1], level-1 size (the layout is the library's
// alone).  The eight bands of level l in the order of the level entries are aaa, then the seven details; the approximation is band 0
// for l == L, else the scratch: level l + 1 reads it (x-y pass) before it writes its own there (z pass), and the inverse likewise.
// volume_scratch_ok: the library can size it (asked before anything is allocated).
inline bool volume_scratch_ok(const int* d, int hlen)
{
    return pdwt_ext3d_tmp_elems(d[0], d[1], d[2], hlen) > 0 && pdwt_ext3d_tmp_approx_offset(d[0], d[1], d[2], hlen) > 0;
}
int alloc3(bw_priv* p, int rc)  // (asked for whatever became of the image and the bands)
{
    p->approx_off = pdwt_ext3d_tmp_approx_offset(p->n[0][0], p->n[1][0], p->n[2][0], p->f.hlen);
    p->d_tmp[0] = (DTYPE*)pdwt_malloc((size_t)pdwt_ext3d_tmp_elems(p->n[0][0], p->n[1][0], p->n[2][0], p->f.hlen) * sizeof(DTYPE));
    return rc != PDWT_OK ? rc : p->d_tmp[0] ? PDWT_OK : PDWT_ENOMEM;
}
int walk3(BoundaryTransform& W, bw_priv* p, bool fwd)
{
    DTYPE* approx = p->d_tmp[0] + p->approx_off;
    for (int l = fwd ? 1 : p->L; l >= 1 && l <= p->L; l += fwd ? 1 : -1) {
        DTYPE* b[8];
        b[0] = l == p->L ? W.d_coeffs[0] : approx;
        for (int k = 0; k < 7; k++) b[1 + k] = W.d_coeffs[1 + 7 * (p->L - l) + k];
        DTYPE* img = l == 1 ? W.d_image : approx;  // the source of the forward level, the destination of the inverse one
        const int nz = p->n[0][l - 1], nr = p->n[1][l - 1], nc = p->n[2][l - 1];
        const int rc = fwd ? SFX(pdwt_ext3d_forward_level)(img, b, nz, nr, nc, p->mode, &p->f, p->d_tmp[0])
                           : SFX(pdwt_ext3d_inverse_level)(img, b, nz, nr, nc, &p->f, p->d_tmp[0]);
        if (rc != PDWT_OK) return rc;
    }
    return PDWT_OK;
}
int forward3(BoundaryTransform& W, bw_priv* p) { return walk3(W, p, true); }
int inverse3(BoundaryTransform& W, bw_priv* p) { return walk3(W, p, false); }

// Batch of images.  As 1-D: the whole-transform entries choose between the one-launch kernels (one workgroup per image) and the
// per-level loop over the stacks; the scratch is that of the loop (two level-1 stacks), sized by the library, none when fused.
int allocb(bw_priv* p, int rc)
{
    const long long ntmp = pdwt_ext2db_tmp_elems(p->n[0][0], p->n[1][0], p->n[2][0], p->f.hlen, p->L, (int)sizeof(DTYPE));
    p->fused = pdwt_ext2db_fused(p->n[1][0], p->n[2][0], p->f.hlen, p->L, (int)sizeof(DTYPE)) == 1;
    if (ntmp < 0) return PDWT_ENOMEM;
    if (rc != PDWT_OK || ntmp == 0) return rc;
    p->d_tmp[0] = (DTYPE*)pdwt_malloc((size_t)ntmp * sizeof(DTYPE));
    return p->d_tmp[0] ? PDWT_OK : PDWT_ENOMEM;
}
int forwardb(BoundaryTransform& W, bw_priv* p)
{
    const int rc = SFX(pdwt_ext2db_forward)(W.d_image, W.d_coeffs, p->n[0][0], p->n[1][0], p->n[2][0], p->L, p->mode, &p->f, p->d_tmp[0]);
    return rc < 0 ? rc : PDWT_OK;
}
int inverseb(BoundaryTransform& W, bw_priv* p)
{
    const int rc = SFX(pdwt_ext2db_inverse)(W.d_image, W.d_coeffs, p->n[0][0], p->n[1][0], p->n[2][0], p->L, &p->f, p->d_tmp[0]);
    return rc < 0 ? rc : PDWT_OK;
}

const bw_ops kOps2 = {"BoundaryWavelets", 2, BW_MAX_LEVELS, 3, false, "image", "a %dx%d image", "is too small", NULL, alloc2, forward2, inverse2, 0};
const bw_ops kOps1 = {"BoundaryWavelets1D", 1, BW_MAX_LEVELS, 1, false, "batch", "rows of %d samples", "are too short", NULL, alloc1, forward1, inverse1, 0};
const bw_ops kOps3 = {"BoundaryWavelets3D", 3, BW3_MAX_LEVELS, 7, true, "volume", "a %dx%dx%d volume", "is too small",
                      "unsupported volume size (Nz <= 65535 and Nr * Nc < 2^31 are required)", alloc3, forward3, inverse3, 0};
const bw_ops kOpsB = {"BoundaryWaveletsImages", 2, BW_MAX_LEVELS, 3, false, "image batch", "%dx%d images", "are too small", NULL, allocb, forwardb, inverseb,
                      BWB_MAX_IMAGES};
}  // namespace
#define ON_MY_DEVICE_B() DevScope dev_scope_(priv_ ? ((const bw_priv*)priv_)->dev : -1)

// ---- construction ------------------------------------------------------------------------------------------------------------------
BoundaryTransform::BoundaryTransform() : d_image(NULL), d_coeffs(NULL), state(W_INIT), ops_(NULL), priv_(NULL) { wname[0] = 0; }

void BoundaryTransform::create(const bw_ops& o, DTYPE* src, const int* dims, const char* wname_, int mode, int memisonhost, int* nlevels, int* hlen_out)
{
    ops_ = &o;
    strncpy(wname, wname_ ? wname_ : "", 127);
    wname[127] = 0;
    state = W_CREATION_ERROR;  // until the last line
    // (3-D states its limits in a message of its own, below)
    const bool too_large = (!o.unsupported && (unsigned long long)dims[1] * (unsigned long long)dims[2] >= (1ull << 31)) || (o.max_batch && dims[0] > o.max_batch);
    if (dims[0] < 1 || dims[1] < 1 || dims[2] < 1 || !wname_ || too_large) {
        printf("ERROR: %s(): invalid %s size or wavelet name\n", o.name, o.noun);
        return;
    }
    if (o.unsupported && !volume_ok(dims)) {
        printf("ERROR: %s(): %s\n", o.name, o.unsupported);
        return;
    }
    if (mode < 0 || mode >= BW_NUM_MODES) {
        printf("ERROR: %s(): unknown boundary mode %d (0 zero, 1 constant, 2 symmetric, 3 reflect, 4 periodic)\n", o.name, mode);
        return;
    }
    if (*nlevels < 1) {
        puts("Warning: cannot initialize wavelet coefficients with nlevels < 1. Forcing nlevels = 1");
        *nlevels = 1;
    }
    bw_priv* p = new (std::nothrow) bw_priv();
    if (!p) return;
    priv_ = p;
    p->dev = pdwt_get_device();
    const int hlen = SFX(pdwt_compute_filters_separable)(wname, 0, &p->f);
    if (hlen <= 0) {
        printf("ERROR: unknown wavelet name %s\n", wname);
        return;
    }
    p->f.hlen = hlen;
    *hlen_out = hlen;
    int* const sizes[3] = {p->n[0], p->n[1], p->n[2]};
    const int wmaxlev = levels_and_sizes(o, dims, hlen, *nlevels, sizes);
    char what[64];  // "a 24x26 image": the transformed sizes (a format with fewer %d leaves the rest alone)
    const int* d = dims + 3 - o.naxes;
    snprintf(what, sizeof(what), o.size_fmt, d[0], o.naxes > 1 ? d[1] : 0, o.naxes > 2 ? d[2] : 0);
    if (*nlevels > wmaxlev) {
        printf("Warning: required level (%d) is greater than the maximum possible level for %s (%d) on %s.\n", *nlevels, wname, wmaxlev, what);
        printf("Forcing nlevels = %d\n", wmaxlev);
        *nlevels = wmaxlev;
    }
    if (*nlevels < 1) {
        printf("ERROR: %s %s for one level of %s\n", what, o.too_small, wname);
        return;
    }
    const int L = p->L = *nlevels, nb = o.per_level * L + 1;
    p->mode = mode;
    if (o.unsupported && !volume_scratch_ok(dims, hlen)) {
        printf("ERROR: %s(): %s\n", o.name, o.unsupported);
        return;
    }
    // the band table: every band at a 256-byte offset of one zero-filled allocation
    size_t off[pdwt_bl::kMaxBands], total = 0;
    for (int k = 0; k < nb; k++) {
        off[k] = total;
        total += ((size_t)shape_of(o, p, k, NULL) * sizeof(DTYPE) + 255) & ~(size_t)255;
    }
    const size_t n = (size_t)dims[0] * dims[1] * dims[2];
    d_image = (DTYPE*)pdwt_malloc(n * sizeof(DTYPE));
    p->d_bands = (DTYPE*)pdwt_malloc(total);
    d_coeffs = (DTYPE**)calloc((size_t)nb, sizeof(DTYPE*));
    int rc = o.alloc_scratch(p, (d_image && p->d_bands && d_coeffs) ? PDWT_OK : PDWT_ENOMEM);
    if (rc == PDWT_OK) {
        for (int k = 0; k < nb; k++) d_coeffs[k] = (DTYPE*)((char*)p->d_bands + off[k]);
        rc = pdwt_memset(p->d_bands, 0, total);
    }
    if (rc == PDWT_OK) {
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

BoundaryTransform::~BoundaryTransform()
{
    ON_MY_DEVICE_B();
    if (d_image) pdwt_free(d_image);
    free(d_coeffs);
    if (priv_) {
        bw_priv* p = P(priv_);
        if (p->d_bands) pdwt_free(p->d_bands);
        if (p->d_tmp[0]) pdwt_free(p->d_tmp[0]);
        if (p->d_tmp[1]) pdwt_free(p->d_tmp[1]);
        if (p->d_tab) pdwt_free(p->d_tab);
        delete p;
    }
}

BoundaryWavelets::BoundaryWavelets(DTYPE* img, int Nr, int Nc, const char* wname_, int levels, int mode, int memisonhost)
{
    const int dims[3] = {1, Nr, Nc};
    winfos.Nr = Nr, winfos.Nc = Nc, winfos.nlevels = levels, winfos.hlen = 0, winfos.mode = mode;
    create(kOps2, img, dims, wname_, mode, memisonhost, &winfos.nlevels, &winfos.hlen);
}

BoundaryWavelets1D::BoundaryWavelets1D(DTYPE* img, int Nr, int Nc, const char* wname_, int levels, int mode, int memisonhost)
{
    const int dims[3] = {1, Nr, Nc};
    winfos.Nr = Nr, winfos.Nc = Nc, winfos.nlevels = levels, winfos.hlen = 0, winfos.mode = mode;
    create(kOps1, img, dims, wname_, mode, memisonhost, &winfos.nlevels, &winfos.hlen);
}

BoundaryWavelets3D::BoundaryWavelets3D(DTYPE* vol, int Nz, int Nr, int Nc, const char* wname_, int levels, int mode, int memisonhost)
{
    const int dims[3] = {Nz, Nr, Nc};
    winfos.Nz = Nz, winfos.Nr = Nr, winfos.Nc = Nc, winfos.nlevels = levels, winfos.hlen = 0, winfos.mode = mode;
    create(kOps3, vol, dims, wname_, mode, memisonhost, &winfos.nlevels, &winfos.hlen);
}

BoundaryWaveletsImages::BoundaryWaveletsImages(DTYPE* imgs, int B, int Nr, int Nc, const char* wname_, int levels, int mode, int memisonhost)
{
    const int dims[3] = {B, Nr, Nc};
    winfos.B = B, winfos.Nr = Nr, winfos.Nc = Nc, winfos.nlevels = levels, winfos.hlen = 0, winfos.mode = mode;
    create(kOpsB, imgs, dims, wname_, mode, memisonhost, &winfos.nlevels, &winfos.hlen);
}

// ---- the static geometry of each class: its own size check, then the shared rule -------------------------------------------------------
int BoundaryWavelets::geometry(int Nr, int Nc, int hlen, int levels, int* nr, int* nc)
{
    if (Nr < 1 || Nc < 1 || (unsigned long long)Nr * (unsigned long long)Nc >= (1ull << 31)) return 0;
    const int dims[3] = {1, Nr, Nc};
    int* const out[3] = {NULL, nr, nc};
    return levels_and_sizes(kOps2, dims, hlen, levels, out);
}

int BoundaryWavelets1D::geometry(int Nc, int hlen, int levels, int* n)
{
    if (Nc < 1) return 0;  // (a row on its own: the limit on Nr * Nc is the constructor's)
    const int dims[3] = {1, 1, Nc};
    int* const out[3] = {NULL, NULL, n};
    return levels_and_sizes(kOps1, dims, hlen, levels, out);
}

int BoundaryWavelets3D::geometry(int Nz, int Nr, int Nc, int hlen, int levels, int* nz, int* nr, int* nc)
{
    const int dims[3] = {Nz, Nr, Nc};
    if (!volume_ok(dims)) return 0;
    int* const out[3] = {nz, nr, nc};
    return levels_and_sizes(kOps3, dims, hlen, levels, out);
}

int BoundaryWavelets::mode_index(const char* name)
{
    if (!name) return -1;
    for (int m = 0; m < BW_NUM_MODES; m++)
        if (!strcmp(name, kModeNames[m])) return m;
    return -1;
}

// ---- transforms ----------------------------------------------------------------------------------------------------------------------
void BoundaryTransform::forward()
{
    ON_MY_DEVICE_B();
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

void BoundaryTransform::inverse()
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
    const int rc = ops_->inverse(*this, P(priv_));
    if (rc != PDWT_OK) {
        report(ops_->name, "::inverse()", rc);
        state = W_INVERSE_ERROR;
        return;
    }
    state = W_INVERSE;
}

// ---- data in and out -----------------------------------------------------------------------------------------------------------------
// get_image and get_coeff return an int: a count beyond INT_MAX is clamped.  Only a volume can be that large (Nr * Nc < 2^31 in every
// class, and a band of the other two is no larger than that bound allows), so for them the clamp is the plain cast it replaces.
static inline int clamp_int(long long n) { return n > (long long)INT_MAX ? INT_MAX : (int)n; }

int BoundaryTransform::get_image(DTYPE* res)
{
    ON_MY_DEVICE_B();
    if (!d_image || !res || state == W_CREATION_ERROR) return 0;
    const bw_priv* p = P(priv_);
    const size_t n = (size_t)p->n[0][0] * p->n[1][0] * p->n[2][0];
    if (pdwt_memcpy_d2h(res, d_image, n * sizeof(DTYPE)) != PDWT_OK) return 0;
    return clamp_int((long long)n);
}

void BoundaryTransform::set_image(DTYPE* img, int mem_is_on_device)
{
    ON_MY_DEVICE_B();
    if (!d_image || !img || state == W_CREATION_ERROR) return;
    const bw_priv* p = P(priv_);
    const size_t nb = (size_t)p->n[0][0] * p->n[1][0] * p->n[2][0] * sizeof(DTYPE);
    const int rc = mem_is_on_device ? pdwt_memcpy_d2d_foreign(d_image, img, nb) : pdwt_memcpy_h2d(d_image, img, nb);
    if (rc != PDWT_OK) report(ops_->name, "::set_image()", rc);
    state = W_INIT;
}

int BoundaryTransform::num_bands() const { return state == W_CREATION_ERROR ? 0 : ops_->per_level * P(priv_)->L + 1; }
int BoundaryWavelets1D::fused() const { return state == W_CREATION_ERROR || !priv_ ? 0 : P(priv_)->fused; }
int BoundaryWaveletsImages::fused() const { return state == W_CREATION_ERROR || !priv_ ? 0 : P(priv_)->fused; }

long long BoundaryTransform::band_shape(int num, int* shape) const
{
    if (state == W_CREATION_ERROR || num < 0 || num >= num_bands()) return 0;
    return shape_of(*ops_, P(priv_), num, shape);
}

long long BoundaryWavelets::coeff_shape(int num, int* nr, int* nc) const
{
    int s[3];
    const long long n = band_shape(num, s);
    if (n > 0 && nr) *nr = s[1];
    if (n > 0 && nc) *nc = s[2];
    return n;
}
long long BoundaryWavelets1D::coeff_shape(int num, int* nr, int* nc) const
{
    int s[3];
    const long long n = band_shape(num, s);
    if (n > 0 && nr) *nr = s[1];
    if (n > 0 && nc) *nc = s[2];
    return n;
}
long long BoundaryWavelets3D::coeff_shape(int num, int* nz, int* nr, int* nc) const
{
    int s[3];
    const long long n = band_shape(num, s);
    if (n > 0 && nz) *nz = s[0];
    if (n > 0 && nr) *nr = s[1];
    if (n > 0 && nc) *nc = s[2];
    return n;
}

long long BoundaryWaveletsImages::coeff_shape(int num, int* b, int* nr, int* nc) const
{
    int s[3];
    const long long n = band_shape(num, s);
    if (n > 0 && b) *b = s[0];
    if (n > 0 && nr) *nr = s[1];
    if (n > 0 && nc) *nc = s[2];
    return n;
}

int BoundaryTransform::get_coeff(DTYPE* coeff, int num)
{
    ON_MY_DEVICE_B();
    if (state == W_INVERSE) {
        puts("Warning: get_coeff(): inverse() has been performed; run forward() first.");
        return 0;
    }
    const long long n = band_shape(num, NULL);
    if (n <= 0 || !coeff) return 0;
    if (pdwt_memcpy_d2h(coeff, d_coeffs[num], (size_t)n * sizeof(DTYPE)) != PDWT_OK) return 0;
    return clamp_int(n);
}

void BoundaryTransform::set_coeff(DTYPE* coeff, int num, int mem_is_on_device)
{
    ON_MY_DEVICE_B();
    const long long n = band_shape(num, NULL);
    if (n <= 0 || !coeff) {
        if (state != W_CREATION_ERROR) printf("ERROR: set_coeff(): invalid coefficient index %d\n", num);
        return;
    }
    const size_t nb = (size_t)n * sizeof(DTYPE);
    const int rc = mem_is_on_device ? pdwt_memcpy_d2d_foreign(d_coeffs[num], coeff, nb) : pdwt_memcpy_h2d(d_coeffs[num], coeff, nb);
    if (rc != PDWT_OK) report(ops_->name, "::set_coeff()", rc);
}

intptr_t BoundaryTransform::image_int_ptr() { return (intptr_t)d_image; }
intptr_t BoundaryTransform::coeff_int_ptr(int num) { return band_shape(num, NULL) > 0 ? (intptr_t)d_coeffs[num] : 0; }

// ---- the band list (bandstats_host.hpp) ------------------------------------------------------------------------------------------
// pointer and size of every band; nb = 0 when the coefficients are not there to be read (need_forward: only those of a forward())
static pdwt_bl::BandList band_list(const BoundaryTransform& W, const bw_ops* o, const bw_priv* p, bool need_forward)
{
    pdwt_bl::BandList bl;
    bl.nb = 0;
    if (W.state == W_CREATION_ERROR || W.state == W_INVERSE || !W.d_coeffs) return bl;
    if (need_forward && !(W.state == W_FORWARD || W.state == W_THRESHOLD)) return bl;
    const int nb = W.num_bands();
    for (int k = 0; k < nb; k++) {
        bl.ptr[k] = W.d_coeffs[k];
        bl.n[k] = (size_t)shape_of(*o, p, k, NULL);
    }
    bl.nb = nb;
    // the last detail band of level 1: D1 (2-D), D_1 of all rows together (1-D), ddd of level 1 (3-D)
    bl.finest = o->coarsest_first ? o->per_level * p->L : o->per_level;
    // N of the universal threshold is the length of ONE signal: the transformed axes (1-D: a row, the batched-1-D rule of wt.h)
    bl.samples = 1.0;
    for (int a = 3 - o->naxes; a < 3; a++) bl.samples *= (double)p->n[a][0];
    return bl;
}
#define BAND_LIST(need_forward) band_list(*this, ops_, P(priv_), need_forward)

void BoundaryTransform::threshold(int op, DTYPE beta, int do_thresh_appcoeffs)
{
    ON_MY_DEVICE_B();
    if (state == W_INVERSE) {
        printf("Warning: %s(): cannot threshold coefficients after W.inverse() (run forward() first)\n", ops_->name);
        return;
    }
    const pdwt_bl::BandList bl = BAND_LIST(false);
    if (!bl.nb) return;
    DTYPE betas[pdwt_bl::kMaxBands];
    for (int k = 0; k < bl.nb; k++) betas[k] = beta;
    if (!do_thresh_appcoeffs) betas[0] = (DTYPE)-1;  // (a negative beta leaves the band alone)
    const int rc = pdwt_bl::threshold(bl, betas, op);
    if (rc != PDWT_OK) {
        report(ops_->name, op ? "::hard_threshold()" : "::soft_threshold()", rc);
        state = W_THRESHOLD_ERROR;
    }
    // (the state stays what it was: unlike the packet classes, a threshold here does not move to W_THRESHOLD)
}
void BoundaryTransform::soft_threshold(DTYPE beta, int do_thresh_appcoeffs) { threshold(0, beta, do_thresh_appcoeffs); }
void BoundaryTransform::hard_threshold(DTYPE beta, int do_thresh_appcoeffs) { threshold(1, beta, do_thresh_appcoeffs); }

double BoundaryTransform::norm1()
{
    ON_MY_DEVICE_B();
    const pdwt_bl::BandList bl = BAND_LIST(false);
    if (!bl.nb) return -1.0;
    w_band_stats s[pdwt_bl::kMaxBands];
    const int rc = pdwt_bl::stats(bl, -1, s, 0);
    if (rc != PDWT_OK) {
        report(ops_->name, "::norm1()", rc);
        return -1.0;
    }
    double sum = 0.0;
    for (int k = 0; k < bl.nb; k++) sum += s[k].sum_abs;
    return sum;
}

int BoundaryTransform::band_stats(int num, w_band_stats* out, int with_median)
{
    ON_MY_DEVICE_B();
    const pdwt_bl::BandList bl = BAND_LIST(true);
    if (!bl.nb || num < 0 || num >= bl.nb || !out) return PDWT_EINVAL;
    const int rc = pdwt_bl::stats(bl, num, out, with_median);
    if (rc != PDWT_OK) report(ops_->name, "::band_stats()", rc);
    return rc;
}

int BoundaryTransform::all_band_stats(w_band_stats* out, int with_median)
{
    ON_MY_DEVICE_B();
    const pdwt_bl::BandList bl = BAND_LIST(true);
    if (!bl.nb || !out) return PDWT_EINVAL;
    const int rc = pdwt_bl::stats(bl, -1, out, with_median);
    if (rc != PDWT_OK) report(ops_->name, "::all_band_stats()", rc);
    return rc;
}

double BoundaryTransform::estimate_sigma()
{
    ON_MY_DEVICE_B();
    const pdwt_bl::BandList bl = BAND_LIST(true);
    double sigma = -1.0;
    if (!bl.nb) return -1.0;
    const int rc = pdwt_bl::estimate_sigma(bl, &sigma);
    if (rc != PDWT_OK) {
        report(ops_->name, "::estimate_sigma()", rc);
        return -1.0;
    }
    return sigma;
}

void BoundaryTransform::threshold_bands(const DTYPE* betas, int kind)
{
    ON_MY_DEVICE_B();
    const pdwt_bl::BandList bl = BAND_LIST(true);
    if (!bl.nb || !betas || (kind != 0 && kind != 1)) return;
    const int rc = pdwt_bl::threshold(bl, betas, kind);
    if (rc != PDWT_OK) {
        report(ops_->name, "::threshold_bands()", rc);
        state = W_THRESHOLD_ERROR;
    }
}

double BoundaryTransform::denoise(int method, double sigma, int kind, DTYPE* betas_out)
{
    ON_MY_DEVICE_B();
    const pdwt_bl::BandList bl = BAND_LIST(true);
    if (!bl.nb || (method != 0 && method != 1) || (kind != 0 && kind != 1)) return -1.0;
    DTYPE betas[pdwt_bl::kMaxBands];
    const int rc = pdwt_bl::denoise(bl, method, kind, &sigma, betas);
    if (rc != PDWT_OK) {
        report(ops_->name, "::denoise()", rc);
        state = W_THRESHOLD_ERROR;
        return -1.0;
    }
    if (betas_out) memcpy(betas_out, betas, (size_t)bl.nb * sizeof(DTYPE));
    return sigma;
}

// ---- the batch of images, per image (the semantics of WaveletsImages, wt.cpp): the batch entries of bandstats_host.hpp over the slices
// of the stacks --------------------------------------------------------------------------------------------------------------------
namespace {
// the band geometry of ONE image (ptr[] = the slices of image 0) and the device table of all B * nb slices; nb = 0: refused
pdwt_bl::BandList image_geometry(const BoundaryTransform& W, const bw_ops* o, bw_priv* p, bool need_forward, DTYPE* const** tab)
{
    pdwt_bl::BandList g = band_list(W, o, p, need_forward);
    *tab = NULL;
    if (!g.nb) return g;
    const int B = p->n[0][0];
    for (int k = 0; k < g.nb; k++) g.n[k] /= (size_t)B;
    if (!p->d_tab) {  // (set_coeff copies INTO the stacks and no method moves them: built once)
        DTYPE** host = new (std::nothrow) DTYPE*[(size_t)B * g.nb];
        void* d = host ? pdwt_malloc((size_t)B * g.nb * sizeof(DTYPE*)) : NULL;
        if (d) {
            for (int b = 0; b < B; b++)
                for (int k = 0; k < g.nb; k++) host[(size_t)b * g.nb + k] = W.d_coeffs[k] + (size_t)b * g.n[k];
            if (pdwt_memcpy_h2d(d, host, (size_t)B * g.nb * sizeof(DTYPE*)) != PDWT_OK) {
                pdwt_free(d);
                d = NULL;
            }
        }
        delete[] host;
        p->d_tab = d;
    }
    *tab = (DTYPE* const*)p->d_tab;
    return g;
}
}  // namespace

int BoundaryWaveletsImages::images_all_band_stats(w_band_stats* out, int with_median)
{
    ON_MY_DEVICE_B();
    DTYPE* const* tab;
    const pdwt_bl::BandList g = image_geometry(*this, ops_, P(priv_), true, &tab);
    if (!g.nb || !out) return PDWT_EINVAL;
    if (!tab) return PDWT_ENOMEM;
    const int rc = pdwt_bl::batch_stats(g, tab, winfos.B, out, with_median);
    if (rc != PDWT_OK) report(ops_->name, "::images_all_band_stats()", rc);
    return rc;
}

int BoundaryWaveletsImages::images_estimate_sigma(double* sigma_out)
{
    ON_MY_DEVICE_B();
    DTYPE* const* tab;
    const pdwt_bl::BandList g = image_geometry(*this, ops_, P(priv_), true, &tab);
    if (!g.nb || !sigma_out) return PDWT_EINVAL;
    if (!tab) return PDWT_ENOMEM;
    pdwt_band_stats* s = new pdwt_band_stats[(size_t)winfos.B * g.nb];
    const int rc = pdwt_bl::batch_estimate_sigma(g, tab, winfos.B, s, sigma_out);
    delete[] s;
    if (rc != PDWT_OK) report(ops_->name, "::images_estimate_sigma()", rc);
    return rc;
}

int BoundaryWaveletsImages::images_threshold_bands(const DTYPE* betas, int kind)
{
    ON_MY_DEVICE_B();
    DTYPE* const* tab;
    const pdwt_bl::BandList g = image_geometry(*this, ops_, P(priv_), true, &tab);
    if (!g.nb || !betas || (kind != 0 && kind != 1)) return PDWT_EINVAL;
    if (!tab) return PDWT_ENOMEM;
    const int rc = pdwt_bl::batch_threshold(g, tab, winfos.B, betas, kind);
    if (rc != PDWT_OK) {
        report(ops_->name, "::images_threshold_bands()", rc);
        state = W_THRESHOLD_ERROR;
    }
    return rc;
}

int BoundaryWaveletsImages::images_denoise(int method, const double* sigma_in, int kind, double* sigma_out, DTYPE* betas_out)
{
    ON_MY_DEVICE_B();
    DTYPE* const* tab;
    const pdwt_bl::BandList g = image_geometry(*this, ops_, P(priv_), true, &tab);
    if (!g.nb || !sigma_out || (method != 0 && method != 1) || (kind != 0 && kind != 1)) return PDWT_EINVAL;
    if (!tab) return PDWT_ENOMEM;
    const size_t cnt = (size_t)winfos.B * g.nb;
    pdwt_band_stats* s = new pdwt_band_stats[cnt];
    DTYPE* betas = betas_out ? betas_out : new DTYPE[cnt];
    const int rc = pdwt_bl::batch_denoise(g, tab, winfos.B, method, kind, sigma_in, s, sigma_out, betas);
    if (!betas_out) delete[] betas;
    delete[] s;
    if (rc != PDWT_OK) {
        report(ops_->name, "::images_denoise()", rc);
        state = W_THRESHOLD_ERROR;
    }
    return rc;
}

int BoundaryWaveletsImages::images_norm1(double* out)
{
    ON_MY_DEVICE_B();
    DTYPE* const* tab;
    const pdwt_bl::BandList g = image_geometry(*this, ops_, P(priv_), false, &tab);
    if (!g.nb || !out) return PDWT_EINVAL;
    if (!tab) return PDWT_ENOMEM;
    w_band_stats* s = new w_band_stats[(size_t)winfos.B * g.nb];
    const int rc = pdwt_bl::batch_stats(g, tab, winfos.B, s, 0);
    for (int b = 0; b < winfos.B && rc == PDWT_OK; b++) {
        double acc = 0.0;
        for (int k = 0; k < g.nb; k++) acc += s[(size_t)b * g.nb + k].sum_abs;
        out[b] = acc;
    }
    delete[] s;
    if (rc != PDWT_OK) report(ops_->name, "::images_norm1()", rc);
    return rc;
}

// ---- flat C handle APIs (pdwt_amd/boundary.py): the same functions under four prefixes; new, info, geometry, coeff_shape (and fused)
// take the arguments of their class and are written out below ---------------------------------------------------------------------
#define BW_HANDLE_API(pfx, Cls)                                                                                                                   \
    void pfx##delete(void* h) { delete static_cast<Cls*>(h); }                                                                                    \
    void pfx##forward(void* h) { static_cast<Cls*>(h)->forward(); }                                                                               \
    void pfx##inverse(void* h) { static_cast<Cls*>(h)->inverse(); }                                                                               \
    int pfx##get_image(void* h, DTYPE* out) { return static_cast<Cls*>(h)->get_image(out); }                                                      \
    void pfx##set_image(void* h, DTYPE* img, int mem_is_on_device) { static_cast<Cls*>(h)->set_image(img, mem_is_on_device); }                    \
    int pfx##state(void* h) { return (int)static_cast<Cls*>(h)->state; }                                                                          \
    int pfx##mode_index(const char* name) { return BoundaryWavelets::mode_index(name); }                                                          \
    int pfx##num_bands(void* h) { return static_cast<Cls*>(h)->num_bands(); }                                                                     \
    int pfx##get_coeff(void* h, DTYPE* out, int num) { return static_cast<Cls*>(h)->get_coeff(out, num); }                                        \
    void pfx##set_coeff(void* h, DTYPE* in, int num, int mem_is_on_device) { static_cast<Cls*>(h)->set_coeff(in, num, mem_is_on_device); }        \
    intptr_t pfx##image_int_ptr(void* h) { return static_cast<Cls*>(h)->image_int_ptr(); }                                                        \
    intptr_t pfx##coeff_int_ptr(void* h, int num) { return static_cast<Cls*>(h)->coeff_int_ptr(num); }                                            \
    void pfx##soft_threshold(void* h, DTYPE beta, int app) { static_cast<Cls*>(h)->soft_threshold(beta, app); }                                   \
    void pfx##hard_threshold(void* h, DTYPE beta, int app) { static_cast<Cls*>(h)->hard_threshold(beta, app); }                                   \
    double pfx##norm1(void* h) { return static_cast<Cls*>(h)->norm1(); }                                                                          \
    int pfx##band_stats(void* h, int num, w_band_stats* out, int with_median) { return static_cast<Cls*>(h)->band_stats(num, out, with_median); } \
    int pfx##all_band_stats(void* h, w_band_stats* out, int with_median) { return static_cast<Cls*>(h)->all_band_stats(out, with_median); }       \
    double pfx##estimate_sigma(void* h) { return static_cast<Cls*>(h)->estimate_sigma(); }                                                        \
    void pfx##threshold_bands(void* h, const DTYPE* betas, int kind) { static_cast<Cls*>(h)->threshold_bands(betas, kind); }                      \
    double pfx##denoise(void* h, int method, double sigma, int kind, DTYPE* betas_out)                                                            \
    {                                                                                                                                             \
        return static_cast<Cls*>(h)->denoise(method, sigma, kind, betas_out);                                                                     \
    }

extern "C" {
BW_HANDLE_API(pdwt_bw_, BoundaryWavelets)
BW_HANDLE_API(pdwt_bw1_, BoundaryWavelets1D)
BW_HANDLE_API(pdwt_bw3_, BoundaryWavelets3D)
BW_HANDLE_API(pdwt_bwb_, BoundaryWaveletsImages)

void* pdwt_bw_new(DTYPE* img, int Nr, int Nc, const char* wname, int levels, int mode, int memisonhost)
{
    return new (std::nothrow) BoundaryWavelets(img, Nr, Nc, wname, levels, mode, memisonhost);
}
void pdwt_bw_info(void* h, w_info_bw* out) { *out = static_cast<BoundaryWavelets*>(h)->winfos; }
int pdwt_bw_geometry(int Nr, int Nc, int hlen, int levels, int* nr, int* nc) { return BoundaryWavelets::geometry(Nr, Nc, hlen, levels, nr, nc); }
long long pdwt_bw_coeff_shape(void* h, int num, int* nr, int* nc) { return static_cast<BoundaryWavelets*>(h)->coeff_shape(num, nr, nc); }

void* pdwt_bw1_new(DTYPE* img, int Nr, int Nc, const char* wname, int levels, int mode, int memisonhost)
{
    return new (std::nothrow) BoundaryWavelets1D(img, Nr, Nc, wname, levels, mode, memisonhost);
}
void pdwt_bw1_info(void* h, w_info_bw* out) { *out = static_cast<BoundaryWavelets1D*>(h)->winfos; }
int pdwt_bw1_geometry(int Nc, int hlen, int levels, int* n) { return BoundaryWavelets1D::geometry(Nc, hlen, levels, n); }
long long pdwt_bw1_coeff_shape(void* h, int num, int* nr, int* nc) { return static_cast<BoundaryWavelets1D*>(h)->coeff_shape(num, nr, nc); }
int pdwt_bw1_fused(void* h) { return static_cast<BoundaryWavelets1D*>(h)->fused(); }

void* pdwt_bw3_new(DTYPE* vol, int Nz, int Nr, int Nc, const char* wname, int levels, int mode, int memisonhost)
{
    return new (std::nothrow) BoundaryWavelets3D(vol, Nz, Nr, Nc, wname, levels, mode, memisonhost);
}
void pdwt_bw3_info(void* h, w_info_bw3* out) { *out = static_cast<BoundaryWavelets3D*>(h)->winfos; }
int pdwt_bw3_geometry(int Nz, int Nr, int Nc, int hlen, int levels, int* nz, int* nr, int* nc)
{
    return BoundaryWavelets3D::geometry(Nz, Nr, Nc, hlen, levels, nz, nr, nc);
}
long long pdwt_bw3_coeff_shape(void* h, int num, int* nz, int* nr, int* nc) { return static_cast<BoundaryWavelets3D*>(h)->coeff_shape(num, nz, nr, nc); }

void* pdwt_bwb_new(DTYPE* imgs, int B, int Nr, int Nc, const char* wname, int levels, int mode, int memisonhost)
{
    return new (std::nothrow) BoundaryWaveletsImages(imgs, B, Nr, Nc, wname, levels, mode, memisonhost);
}
void pdwt_bwb_info(void* h, w_info_bwb* out) { *out = static_cast<BoundaryWaveletsImages*>(h)->winfos; }
int pdwt_bwb_geometry(int Nr, int Nc, int hlen, int levels, int* nr, int* nc) { return BoundaryWavelets::geometry(Nr, Nc, hlen, levels, nr, nc); }
long long pdwt_bwb_coeff_shape(void* h, int num, int* b, int* nr, int* nc) { return static_cast<BoundaryWaveletsImages*>(h)->coeff_shape(num, b, nr, nc); }
int pdwt_bwb_fused(void* h) { return static_cast<BoundaryWaveletsImages*>(h)->fused(); }
int pdwt_bwb_images_all_band_stats(void* h, w_band_stats* out, int with_median) { return static_cast<BoundaryWaveletsImages*>(h)->images_all_band_stats(out, with_median); }
int pdwt_bwb_images_estimate_sigma(void* h, double* sigma_out) { return static_cast<BoundaryWaveletsImages*>(h)->images_estimate_sigma(sigma_out); }
int pdwt_bwb_images_threshold_bands(void* h, const DTYPE* betas, int kind) { return static_cast<BoundaryWaveletsImages*>(h)->images_threshold_bands(betas, kind); }
int pdwt_bwb_images_denoise(void* h, int method, const double* sigma_in, int kind, double* sigma_out, DTYPE* betas_out)
{
    return static_cast<BoundaryWaveletsImages*>(h)->images_denoise(method, sigma_in, kind, sigma_out, betas_out);
}
int pdwt_bwb_images_norm1(void* h, double* out) { return static_cast<BoundaryWaveletsImages*>(h)->images_norm1(out); }
}
