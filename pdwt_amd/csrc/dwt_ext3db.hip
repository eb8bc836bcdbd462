// dwt_ext3db.hip -- the 3-D transform with signal-extension boundary modes and its adjoints on a STACK of V volumes, every level in one
// driver call (include/pdwt_hip.h "Batched 3-D DWT with boundary modes").  Volume v of every result holds the bits that the chain of
// level entries of dwt_ext3d.hip / dwt_ext3d_adj.hip gives on volume v alone: a level here is the step that those entries run
// (dwt_ext3d_level.hpp), on V volumes.
//   x-y passes   the kernels of dwt_ext3d.hip and the 2-D level adjoint as they are, on chunks of the V * nz planes.
//   z passes     the kernels of z_stages.hpp instantiated for the stack jobs (ZStackJob, Adj3ZStackJob; nothing is restated here): grid
//                z = a (volume, quadrant) pair p = 4 * v + q, in chunks of at most 65535 pairs (a chunk may begin inside a volume);
//                the body is that of the one-volume kernels on column pointers offset by the volume: quadrant stack q is
//                V x nz x hr x hc, band stack k is V x hz x hr x hc, volume v of either starts v * planes * plane elements in.
// Every output element is written once by one thread; no atomics.  Nothing synchronises with the host between levels or chunks.
// Scratch: [the four quadrant stacks of level 1 | two approximation stacks of level 1 in turn (levels > 1) | the frames of the planes
// (forward adjoint)]; the quadrants and approximations of a deeper level are no larger (n >= hlen - 1 gives (n + hlen - 1) / 2 <= n);
// of the frames the level that needs most is taken.
#include "dwt_ext3d_level.hpp"
#include "vol3d.hpp"

namespace pdwt {

// ---- geometry (host, no device) ---------------------------------------------------------------------------------------------------
struct X3bGeom {
    int nz[kVolMaxLevels + 1], nr[kVolMaxLevels + 1], nc[kVolMaxLevels + 1];  // [0]: the volume; [l]: the bands of level l
    size_t V;
    size_t quads() const { return 4 * V * nz[0] * nr[1] * nc[1]; }
    size_t approx() const { return V * nz[1] * nr[1] * nc[1]; }
};

// What every entry refuses: V < 1, levels outside 1 .. 13, a level that the level entries refuse (adjoint: also what the 2-D level
// adjoint refuses on a chunk of planes), and a stack of 2^31 planes or 2^40 elements or more (plane counts are ints; every product of
// the scratch formulas stays far below 2^64).
static bool ext3db_geom(X3bGeom& g, int V, int Nz, int Nr, int Nc, int hlen, int levels, bool adjoint)
{
    if (V < 1 || levels < 1 || levels > kVolMaxLevels) return false;
    g.V = (size_t)V, g.nz[0] = Nz, g.nr[0] = Nr, g.nc[0] = Nc;
    for (int l = 0; l < levels; l++) {
        if (!ext3_level_ok(g.nz[l], g.nr[l], g.nc[l], hlen)) return false;
        const long long planes = (long long)V * g.nz[l];
        if (adjoint && !adj2_level_ok(planes < kZMaxSlots ? planes : kZMaxSlots, g.nr[l], g.nc[l], hlen)) return false;
        g.nz[l + 1] = ext_half(g.nz[l], hlen), g.nr[l + 1] = ext_half(g.nr[l], hlen), g.nc[l + 1] = ext_half(g.nc[l], hlen);
    }
    const unsigned long long planes = (unsigned long long)V * (unsigned long long)Nz;
    if (planes >= (1ull << 31)) return false;
    return planes * ((unsigned long long)Nr * (unsigned long long)Nc) < (1ull << 40);  // (Nr * Nc < 2^31: no overflow)
}

static size_t ext3db_tmp(const X3bGeom& g, int levels) { return g.quads() + (levels > 1 ? 2 * g.approx() : 0); }
// the frames of the planes of the level that needs most
static size_t ext3db_frames(const X3bGeom& g, int hlen, int levels)
{
    size_t most = 0;
    for (int l = 0; l < levels; l++) {
        const size_t e = g.V * g.nz[l] * adj_frame_elems(g.nr[l], g.nc[l], hlen);
        most = e > most ? e : most;
    }
    return most;
}

template <typename T>
static bool ext3db_table_ok(T* const* b, int levels)
{
    if (!b || levels < 1 || levels > kVolMaxLevels) return false;
    for (int k = 0; k < 7 * levels + 1; k++)
        if (!b[k]) return false;
    return true;
}

// ---- drivers -------------------------------------------------------------------------------------------------------------------
// Level l = 1 .. levels reads the stack of shape [l - 1] and gives the eight band stacks of shape [l]: aaa of the last level is band 0
// of the table, of any other one of the two approximation stacks in turn; the details are the bands 1 + 7 * (levels - l) ...
template <typename T>
static T* ext3db_approx(T* ping, size_t stack, int l) { return ping + (size_t)((l - 1) & 1) * stack; }  // aaa of level l < levels

template <typename T>
static int ext3db_forward(const T* src, T* const* b, int V, int Nz, int Nr, int Nc, int levels, int mode, const typename FiltersOf<T>::type* f, T* tmp, bool adjoint)
{
    X3bGeom g;
    if (!src || !f || !tmp || mode < 0 || mode >= EXT_NUM_MODES || !ext3db_table_ok(b, levels) || !ext3db_geom(g, V, Nz, Nr, Nc, f->hlen, levels, adjoint))
        return PDWT_EINVAL;
    const int hlen = f->hlen;
    const Taps2<T> taps = taps_fwd<T>(f);
    T* const ping = tmp + g.quads();
    for (int l = 1; l <= levels; l++) {
        const T* in = l == 1 ? src : ext3db_approx(ping, g.approx(), l - 1);
        T* lev[8];
        lev[0] = l == levels ? b[0] : ext3db_approx(ping, g.approx(), l);
        for (int k = 0; k < 7; k++) lev[1 + k] = b[band3(levels, l, k)];
        const Ext3Step<T> step{g.V, g.nz[l - 1], g.nr[l - 1], g.nc[l - 1], hlen, tmp};
        if (const int rc = ext3_forward_step<true, T>(step, in, lev, mode, taps); rc != PDWT_OK) return rc;
    }
    return PDWT_OK;
}

// mode < 0: the inverse; a mode: the adjoint of the forward transform.  Coarse to fine: the result of level l is aaa of level l - 1.
template <typename T>
static int ext3db_backward(T* dst, T* const* b, int V, int Nz, int Nr, int Nc, int levels, int mode, const typename FiltersOf<T>::type* f, T* tmp)
{
    const bool adjoint = mode >= 0;
    X3bGeom g;
    if (!dst || !f || !tmp || mode >= EXT_NUM_MODES || !ext3db_table_ok(b, levels) || !ext3db_geom(g, V, Nz, Nr, Nc, f->hlen, levels, adjoint)) return PDWT_EINVAL;
    const int hlen = f->hlen;
    const Taps2<T> taps = adjoint ? taps_adj<T>(f) : taps_inv<T>(f);
    T* const ping = tmp + g.quads();
    T* const frames = ping + (levels > 1 ? 2 * g.approx() : 0);
    for (int l = levels; l >= 1; l--) {
        T* out = l == 1 ? dst : ext3db_approx(ping, g.approx(), l - 1);
        T* lev[8];
        lev[0] = l == levels ? b[0] : ext3db_approx(ping, g.approx(), l);
        for (int k = 0; k < 7; k++) lev[1 + k] = b[band3(levels, l, k)];
        const Ext3Step<T> step{g.V, g.nz[l - 1], g.nr[l - 1], g.nc[l - 1], hlen, tmp};
        const int rc = adjoint ? ext3_adjoint_step<true, T>(step, out, lev, mode, f, taps, frames) : ext3_inverse_step<true, T>(step, out, lev, taps);
        if (rc != PDWT_OK) return rc;
    }
    return PDWT_OK;
}

template <typename T>
static int ext3db_inverse_adjoint(const T* src, T* const* b, int V, int Nz, int Nr, int Nc, int levels, const typename FiltersOf<T>::type* f, T* tmp)
{
    typename FiltersOf<T>::type g;
    if (!adj_inverse_bank<T>(g, f)) return PDWT_EINVAL;
    return ext3db_forward<T>(src, b, V, Nz, Nr, Nc, levels, EXT_ZERO, &g, tmp, true);
}

}  // namespace pdwt

using namespace pdwt;

extern "C" {
long long pdwt_ext3db_tmp_elems(int V, int Nz, int Nr, int Nc, int hlen, int levels)
{
    X3bGeom g;
    if (!ext3db_geom(g, V, Nz, Nr, Nc, hlen, levels, false)) return PDWT_EINVAL;
    return (long long)ext3db_tmp(g, levels);
}
long long pdwt_ext3db_adjoint_tmp_elems(int V, int Nz, int Nr, int Nc, int hlen, int levels)
{
    X3bGeom g;
    if (!ext3db_geom(g, V, Nz, Nr, Nc, hlen, levels, true)) return PDWT_EINVAL;
    return (long long)(ext3db_tmp(g, levels) + ext3db_frames(g, hlen, levels));
}
int pdwt_ext3db_forward_f32(const float* d_src, float* const* d_bands, int V, int Nz, int Nr, int Nc, int levels, int mode, const pdwt_filters_f32* f, float* d_tmp)
{
    return ext3db_forward<float>(d_src, d_bands, V, Nz, Nr, Nc, levels, mode, f, d_tmp, false);
}
int pdwt_ext3db_forward_f64(const double* d_src, double* const* d_bands, int V, int Nz, int Nr, int Nc, int levels, int mode, const pdwt_filters_f64* f, double* d_tmp)
{
    return ext3db_forward<double>(d_src, d_bands, V, Nz, Nr, Nc, levels, mode, f, d_tmp, false);
}
int pdwt_ext3db_inverse_f32(float* d_dst, float* const* d_bands, int V, int Nz, int Nr, int Nc, int levels, const pdwt_filters_f32* f, float* d_tmp)
{
    return ext3db_backward<float>(d_dst, d_bands, V, Nz, Nr, Nc, levels, -1, f, d_tmp);
}
int pdwt_ext3db_inverse_f64(double* d_dst, double* const* d_bands, int V, int Nz, int Nr, int Nc, int levels, const pdwt_filters_f64* f, double* d_tmp)
{
    return ext3db_backward<double>(d_dst, d_bands, V, Nz, Nr, Nc, levels, -1, f, d_tmp);
}
int pdwt_ext3db_forward_adjoint_f32(float* d_dst, float* const* d_bands, int V, int Nz, int Nr, int Nc, int levels, int mode, const pdwt_filters_f32* f, float* d_tmp)
{
    if (mode < 0) return PDWT_EINVAL;
    return ext3db_backward<float>(d_dst, d_bands, V, Nz, Nr, Nc, levels, mode, f, d_tmp);
}
int pdwt_ext3db_forward_adjoint_f64(double* d_dst, double* const* d_bands, int V, int Nz, int Nr, int Nc, int levels, int mode, const pdwt_filters_f64* f, double* d_tmp)
{
    if (mode < 0) return PDWT_EINVAL;
    return ext3db_backward<double>(d_dst, d_bands, V, Nz, Nr, Nc, levels, mode, f, d_tmp);
}
int pdwt_ext3db_inverse_adjoint_f32(const float* d_src, float* const* d_bands, int V, int Nz, int Nr, int Nc, int levels, const pdwt_filters_f32* f, float* d_tmp)
{
    return ext3db_inverse_adjoint<float>(d_src, d_bands, V, Nz, Nr, Nc, levels, f, d_tmp);
}
int pdwt_ext3db_inverse_adjoint_f64(const double* d_src, double* const* d_bands, int V, int Nz, int Nr, int Nc, int levels, const pdwt_filters_f64* f, double* d_tmp)
{
    return ext3db_inverse_adjoint<double>(d_src, d_bands, V, Nz, Nr, Nc, levels, f, d_tmp);
}
}
