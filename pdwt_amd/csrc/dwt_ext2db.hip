// dwt_ext2db.hip -- the batched 2-D transform with signal-extension boundary modes (include/pdwt_hip.h "Batched 2-D DWT with boundary
// modes"; the class: BoundaryWaveletsImages, include/wt_ext.h): pywt.wavedec2(x, w, mode, level, axes=(-2, -1)) of a B x Nr x Nc stack of
// images, the transform of dwt_ext.hip on every image.  Band `num` of the batch is one contiguous B x nr_l x nc_l stack, image-major.
//   k_ext2db_fwd_fused  the WHOLE pyramid of one image per workgroup (grid.x = B): the image is staged into LDS once (16-byte loads),
//                       every level is a row pass LDS -> LDS and a column pass whose H, V, D go to HBM and whose A stays in LDS as the
//                       next level's input; only A_L leaves.  Traffic: one read of the batch, one write of each band.
//   k_ext2db_inv_fused  coarse to fine the same way: A_L is staged once, the approximation of every other level stays in LDS, H then
//                       (V, D) are staged per level (at most two child bands resident), the last level writes the image.
//   per level           images that do not fit LDS, and the level entries of the C ABI: the x-y tile kernels of dwt_ext3d.hip with the
//                       images as the planes (run_ext3_xy: no kernel of its own), one launch per level and direction.
// The pipelines of the fused kernels are the functions of dwt_ext2db.hpp, their stages those of image_stages.hpp; all three forms (and a loop over BoundaryWavelets instances)
// compute the same bits.  Barriers between LDS stages are LDS-only (lgkmcnt), so the detail stores of a level are not waited for.
//
// Workgroup size 512.  An image above 80 KiB of LDS has the compute unit to itself; 256 threads would leave one wave per SIMD to hide
// the LDS latency of the tap loops, 512 leave two and still give every thread 256 vector registers (1024 would halve that for little
// gain: the deep levels have fewer positions than threads anyway).  Smaller images share the unit: 34 KB (64 x 64 float32) runs four
// workgroups per unit.
// LDS rule (ext2db_plan, the single source of truth).  Forward (Nr Nc + 2 Nr N_c1) elements + the two index tables; inverse
// 2 ru(N_r1 N_c1) + 2 Nr N_c1 elements (H, V, D are STAGED, two at a time, not read through the cache).  Fused when the larger fits 160 KiB.
#include <algorithm>

#include "dwt_ext2db.hpp"
#include "dwt_ext3d_xy.hpp"

namespace pdwt {

constexpr int kExt2dbMaxBatch = 65535;  // the images are grid.z of the per-level kernels

template <typename T, int HL>
__global__ __launch_bounds__(kExt2dbThreads) void k_ext2db_fwd_fused(const T* __restrict__ src, Ext2dbBands<T> b, int mode, Taps2<T> taps)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    T* img = reinterpret_cast<T*>(smem);                       // [Nr][Nc], later A_1, A_2, ...
    T* rb = img + b.nr[0] * b.nc[0];                           // [2][Nr][N_c1]: row pass lo | hi
    int* cmap = reinterpret_cast<int*>(rb + 2 * b.nr[0] * b.nc[1]);
    int* rmap = cmap + 2 * b.nc[1] + HL - 2;
    ext2db_fwd_image<T, HL, kExt2dbThreads>(img, rb, cmap, rmap, src, b, (size_t)blockIdx.x, mode, taps, (int)threadIdx.x, LdsBarrier());
}

template <typename T, int HL>
__global__ __launch_bounds__(kExt2dbThreads) void k_ext2db_inv_fused(T* __restrict__ dst, Ext2dbBands<T> b, Taps2<T> taps)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int cap = ext1d_ru4(b.nr[1] * b.nc[1]);
    T* ra = reinterpret_cast<T*>(smem);  // the approximation, then V
    T* rd = ra + cap;                    // H, then D
    T* cb = rd + cap;                    // [2][Nr][N_c1]
    ext2db_inv_image<T, HL, kExt2dbThreads>(ra, rd, cb, dst, b, (size_t)blockIdx.x, taps, (int)threadIdx.x, LdsBarrier());
}

// ---- geometry and the plan (host, no device) ------------------------------------------------------------------------------------------
// what a level refuses: a bad bank length, an axis shorter than hlen - 1 (the halo must fold at most once per period), sizes the 32-bit
// indices or the grid of the tile kernels cannot take
static bool ext2db_level_ok(long long B, int nr, int nc, int hlen)
{
    if (hlen < 2 || hlen > PDWT_MAX_FILTER_WIDTH || (hlen & 1)) return false;
    if (B < 1 || B > kExt2dbMaxBatch) return false;
    if (nr < 1 || nc < 1 || nr < hlen - 1 || nc < hlen - 1 || nr > (1 << 30) || nc > (1 << 30)) return false;
    if ((unsigned long long)nr * (unsigned long long)nc >= (1ull << 31)) return false;
    return idiv_up(ext_half(nr, hlen), TFY) <= 65535 && idiv_up(nr, TIY) <= 65535;
}
static bool ext2db_ok(long long B, int Nr, int Nc, int hlen, int levels)
{
    if (levels < 1 || levels > kExt2dbMaxLev) return false;
    for (int l = 0; l < levels; l++) {
        if (!ext2db_level_ok(B, Nr, Nc, hlen)) return false;
        Nr = ext_half(Nr, hlen), Nc = ext_half(Nc, hlen);
    }
    return true;
}

struct Ext2dbPlan {
    bool fused;
    size_t lds_fwd, lds_inv;  // of a workgroup (one image)
};
// (the maxima over the levels: level 1 holds them whenever every axis is at least hlen - 1 long, which ext2db_ok has checked)
static Ext2dbPlan ext2db_plan(int Nr, int Nc, int hlen, int levels, size_t elem)
{
    size_t in_max = 0, rb_max = 0, band_max = 0, tab = 0;
    int nr = Nr, nc = Nc;
    for (int l = 1; l <= levels; l++) {
        const int hr = ext_half(nr, hlen), hc = ext_half(nc, hlen);
        in_max = std::max(in_max, (size_t)nr * nc);
        rb_max = std::max(rb_max, 2 * (size_t)nr * hc);
        band_max = std::max(band_max, (size_t)ext1d_ru4(hr * hc));
        tab = std::max(tab, (size_t)(2 * hr + 2 * hc + 2 * hlen - 4));
        nr = hr, nc = hc;
    }
    Ext2dbPlan p;
    p.lds_fwd = (in_max + rb_max) * elem + tab * sizeof(int);
    p.lds_inv = (2 * band_max + rb_max) * elem;
    p.fused = std::max(p.lds_fwd, p.lds_inv) <= kLdsMax;
    return p;
}

template <typename T>
static bool ext2db_fill_bands(Ext2dbBands<T>& b, T* const* c, int Nr, int Nc, int hlen, int levels)
{
    if (!c) return false;
    b.nlev = levels, b.nr[0] = Nr, b.nc[0] = Nc;
    for (int l = 1; l <= levels; l++) b.nr[l] = ext_half(b.nr[l - 1], hlen), b.nc[l] = ext_half(b.nc[l - 1], hlen);
    for (int k = 0; k < 3 * levels + 1; k++) {
        if (!c[k]) return false;
        b.p[k] = c[k];
    }
    return true;
}

// ---- drivers -----------------------------------------------------------------------------------------------------------------
template <typename T>
static int ext2db_forward_level(const T* src, T* a, T* h, T* v, T* d, int B, int nr, int nc, int mode, const typename FiltersOf<T>::type* f)
{
    if (!src || !a || !h || !v || !d || !f || mode < 0 || mode >= EXT_NUM_MODES || !ext2db_level_ok(B, nr, nc, f->hlen)) return PDWT_EINVAL;
    Ext3XYJob<T> xy{};
    xy.src = src;
    xy.q[0] = a, xy.q[1] = h, xy.q[2] = v, xy.q[3] = d;
    xy.nr = nr, xy.nc = nc, xy.hr = ext_half(nr, f->hlen), xy.hc = ext_half(nc, f->hlen), xy.mode = mode;
    return run_ext3_xy<T>(f->hlen, true, xy, B, taps_fwd<T>(f));
}

template <typename T>
static int ext2db_inverse_level(T* dst, const T* a, const T* h, const T* v, const T* d, int B, int nr, int nc, const typename FiltersOf<T>::type* f)
{
    if (!dst || !a || !h || !v || !d || !f || !ext2db_level_ok(B, nr, nc, f->hlen)) return PDWT_EINVAL;
    Ext3XYJob<T> xy{};
    xy.dst = dst;  // (the inverse kernel only reads the quadrants)
    xy.q[0] = const_cast<T*>(a), xy.q[1] = const_cast<T*>(h), xy.q[2] = const_cast<T*>(v), xy.q[3] = const_cast<T*>(d);
    xy.nr = nr, xy.nc = nc, xy.hr = ext_half(nr, f->hlen), xy.hc = ext_half(nc, f->hlen), xy.mode = 0;
    return run_ext3_xy<T>(f->hlen, false, xy, B, taps_inv<T>(f));
}

template <typename T, int HL>
static int launch_ext2db_fwd_fused(const T* src, const Ext2dbBands<T>& b, int B, int mode, const Ext2dbPlan& p, const Taps2<T>& taps)
{
    const int rc = launch_lds(k_ext2db_fwd_fused<T, HL>, dim3(B), dim3(kExt2dbThreads), p.lds_fwd, src, b, mode, taps);
    return rc == PDWT_OK ? PDWT_EXT2DB_FUSED : rc;
}
template <typename T, int HL>
static int launch_ext2db_inv_fused(T* dst, const Ext2dbBands<T>& b, int B, const Ext2dbPlan& p, const Taps2<T>& taps)
{
    const int rc = launch_lds(k_ext2db_inv_fused<T, HL>, dim3(B), dim3(kExt2dbThreads), p.lds_inv, dst, b, taps);
    return rc == PDWT_OK ? PDWT_EXT2DB_FUSED : rc;
}

// The approximation stack of level l (1 .. L - 1) of the per-level path: the halves of d_tmp in turn (each B x N_r1 x N_c1 elements),
// as the ping buffers of BoundaryWavelets.
template <typename T>
static T* ext2db_tmp_of(T* tmp, size_t stack1, int l) { return tmp + ((l - 1) & 1) * stack1; }

template <typename T>
static int ext2db_forward(const T* src, T* const* c, int B, int Nr, int Nc, int levels, int mode, const typename FiltersOf<T>::type* f, T* tmp)
{
    Ext2dbBands<T> b;
    if (!src || !f || mode < 0 || mode >= EXT_NUM_MODES || !ext2db_ok(B, Nr, Nc, f->hlen, levels) || !ext2db_fill_bands(b, c, Nr, Nc, f->hlen, levels))
        return PDWT_EINVAL;
    const int hlen = f->hlen;
    const Ext2dbPlan p = ext2db_plan(Nr, Nc, hlen, levels, sizeof(T));
    if (p.fused) {
        const Taps2<T> taps = taps_fwd<T>(f);
        return with_filter_length<2>(hlen, [&](auto hl) { return launch_ext2db_fwd_fused<T, decltype(hl)::value>(src, b, B, mode, p, taps); });
    }
    if (!tmp) return PDWT_EINVAL;
    const size_t stack1 = (size_t)B * b.nr[1] * b.nc[1];
    for (int l = 1; l <= levels; l++) {
        T* a = l == levels ? b.p[0] : ext2db_tmp_of(tmp, stack1, l);
        T* const* d = b.p + 3 * (l - 1) + 1;
        if (const int rc = ext2db_forward_level<T>(src, a, d[0], d[1], d[2], B, b.nr[l - 1], b.nc[l - 1], mode, f); rc != PDWT_OK) return rc;
        src = a;
    }
    return PDWT_EXT2DB_LEVELS;
}

template <typename T>
static int ext2db_inverse(T* dst, T* const* c, int B, int Nr, int Nc, int levels, const typename FiltersOf<T>::type* f, T* tmp)
{
    Ext2dbBands<T> b;
    if (!dst || !f || !ext2db_ok(B, Nr, Nc, f->hlen, levels) || !ext2db_fill_bands(b, c, Nr, Nc, f->hlen, levels)) return PDWT_EINVAL;
    const int hlen = f->hlen;
    const Ext2dbPlan p = ext2db_plan(Nr, Nc, hlen, levels, sizeof(T));
    if (p.fused) {
        const Taps2<T> taps = taps_inv<T>(f);
        return with_filter_length<2>(hlen, [&](auto hl) { return launch_ext2db_inv_fused<T, decltype(hl)::value>(dst, b, B, p, taps); });
    }
    if (!tmp) return PDWT_EINVAL;
    const size_t stack1 = (size_t)B * b.nr[1] * b.nc[1];
    for (int l = levels; l >= 1; l--) {
        const T* a = l == levels ? b.p[0] : ext2db_tmp_of(tmp, stack1, l);
        T* out = l == 1 ? dst : ext2db_tmp_of(tmp, stack1, l - 1);
        T* const* d = b.p + 3 * (l - 1) + 1;
        if (const int rc = ext2db_inverse_level<T>(out, a, d[0], d[1], d[2], B, b.nr[l - 1], b.nc[l - 1], f); rc != PDWT_OK) return rc;
    }
    return PDWT_EXT2DB_LEVELS;
}

}  // namespace pdwt

using namespace pdwt;

extern "C" {
int pdwt_ext2db_fused(int Nr, int Nc, int hlen, int levels, int elem_size)
{
    if (!ext2db_ok(1, Nr, Nc, hlen, levels) || (elem_size != 4 && elem_size != 8)) return PDWT_EINVAL;
    return ext2db_plan(Nr, Nc, hlen, levels, (size_t)elem_size).fused ? 1 : 0;
}
long long pdwt_ext2db_tmp_elems(int B, int Nr, int Nc, int hlen, int levels, int elem_size)
{
    const int fu = pdwt_ext2db_fused(Nr, Nc, hlen, levels, elem_size);
    if (fu < 0 || !ext2db_ok(B, Nr, Nc, hlen, levels)) return PDWT_EINVAL;
    return fu ? 0 : 2ll * B * ext_half(Nr, hlen) * ext_half(Nc, hlen);
}
int pdwt_ext2db_forward_level_f32(const float* d_src, float* d_a, float* d_h, float* d_v, float* d_d, int B, int nr, int nc, int mode, const pdwt_filters_f32* f)
{
    return ext2db_forward_level<float>(d_src, d_a, d_h, d_v, d_d, B, nr, nc, mode, f);
}
int pdwt_ext2db_forward_level_f64(const double* d_src, double* d_a, double* d_h, double* d_v, double* d_d, int B, int nr, int nc, int mode, const pdwt_filters_f64* f)
{
    return ext2db_forward_level<double>(d_src, d_a, d_h, d_v, d_d, B, nr, nc, mode, f);
}
int pdwt_ext2db_inverse_level_f32(float* d_dst, const float* d_a, const float* d_h, const float* d_v, const float* d_d, int B, int nr, int nc, const pdwt_filters_f32* f)
{
    return ext2db_inverse_level<float>(d_dst, d_a, d_h, d_v, d_d, B, nr, nc, f);
}
int pdwt_ext2db_inverse_level_f64(double* d_dst, const double* d_a, const double* d_h, const double* d_v, const double* d_d, int B, int nr, int nc, const pdwt_filters_f64* f)
{
    return ext2db_inverse_level<double>(d_dst, d_a, d_h, d_v, d_d, B, nr, nc, f);
}
int pdwt_ext2db_forward_f32(const float* d_src, float* const* d_coeffs, int B, int Nr, int Nc, int levels, int mode, const pdwt_filters_f32* f, float* d_tmp)
{
    return ext2db_forward<float>(d_src, d_coeffs, B, Nr, Nc, levels, mode, f, d_tmp);
}
int pdwt_ext2db_forward_f64(const double* d_src, double* const* d_coeffs, int B, int Nr, int Nc, int levels, int mode, const pdwt_filters_f64* f, double* d_tmp)
{
    return ext2db_forward<double>(d_src, d_coeffs, B, Nr, Nc, levels, mode, f, d_tmp);
}
int pdwt_ext2db_inverse_f32(float* d_dst, float* const* d_coeffs, int B, int Nr, int Nc, int levels, const pdwt_filters_f32* f, float* d_tmp)
{
    return ext2db_inverse<float>(d_dst, d_coeffs, B, Nr, Nc, levels, f, d_tmp);
}
int pdwt_ext2db_inverse_f64(double* d_dst, double* const* d_coeffs, int B, int Nr, int Nc, int levels, const pdwt_filters_f64* f, double* d_tmp)
{
    return ext2db_inverse<double>(d_dst, d_coeffs, B, Nr, Nc, levels, f, d_tmp);
}
}
