// vol3d.hpp -- what the two volume transforms (dwt3d.hip, swt3d.hip) share besides their class: the band numbering, the size limits,
// the band table and the walks over it, and the dispatch on the filter length.  The kernels, the tiles, the scratch layout, the
// rest of the geometry (Geom3 / tmp3; the hlen and level-clamp check of swt_geom) and forward / inverse stay with each transform.
#pragma once
#include <type_traits>

#include "common.hpp"
#include "bandlist.hpp"

namespace pdwt {

// 0 that the compiler cannot see through: a tap index offset by it is not loop-invariant, so the scalar loads of the taps are
// issued inside each loop instead of all hoisted in front of the loops (2*HL doubles of a long bank do not fit the SGPRs)
__device__ __forceinline__ int opaque_zero()
{
    int z = 0;
    asm volatile("" : "+s"(z));
    return z;
}

constexpr int kVolMaxLevels = 13;                    // 7*13 + 1 = 92 bands <= the 97 of the band-table kernels (utils.hip)
constexpr int kVolMaxBands = 7 * kVolMaxLevels + 1;

static inline size_t pad64(size_t n) { return (n + 63) & ~(size_t)63; }  // 256-byte multiples for either precision

// band index of detail k (0..6: aad, ada, add, daa, dad, dda, ddd) of level lev (1 = finest)
static inline int band3(int L, int lev, int k) { return 1 + 7 * (L - lev) + k; }

// the z pass pairs: quadrant q (2 * x band + y band) -> (z low, z high) detail index of the level (-1: the approximation)
//   q0 (y a, x a): aaa, daa    q1 (y d, x a): ada, dda    q2 (y a, x d): aad, dad    q3 (y d, x d): add, ddd
constexpr int kZLow[4] = {-1, 1, 0, 2}, kZHigh[4] = {3, 5, 4, 6};

// the limits of both transforms: a plane is indexed with 32 bits (lanes across it) and z is a grid dimension
static inline bool vol_sizes_ok(const pdwt_info3d& w)
{
    if (w.Nz < 1 || w.Nr < 1 || w.Nc < 1 || w.nlevels < 1 || w.nlevels > kVolMaxLevels) return false;
    return (unsigned long long)w.Nr * (unsigned long long)w.Nc < (1ull << 31) && w.Nz <= 65535;
}

// ---- band table: 7L+1 bands in ONE zero-filled allocation at 256-byte offsets; band_size(k) = elements of band k -------------
template <typename T, typename BandSize>
static T** vol_create_bands(int L, BandSize band_size)
{
    const int nb = 7 * L + 1;
    size_t off[kVolMaxBands];
    size_t total = 0;
    for (int k = 0; k < nb; k++) {
        off[k] = total;
        total += ((size_t)band_size(k) * sizeof(T) + 255) & ~(size_t)255;
    }
    char* base = (char*)pdwt_malloc(total);
    if (!base) return nullptr;
    if (pdwt_memset(base, 0, total) != PDWT_OK) {
        (void)pdwt_free(base);
        return nullptr;
    }
    T** tab = (T**)calloc((size_t)nb + 1, sizeof(T*));  // slot [-1]: the allocation base (as coeffs.hip)
    if (!tab) {
        (void)pdwt_free(base);
        return nullptr;
    }
    tab[0] = (T*)base;
    for (int k = 0; k < nb; k++) tab[k + 1] = (T*)(base + off[k]);
    return tab + 1;
}
template <typename T>
static int vol_free_bands(T** c)
{
    if (!c) return PDWT_OK;
    const int rc = pdwt_free((void*)c[-1]);
    free(c - 1);
    return rc;
}

// thresholds: the 2-D rules of utils.hip ew_bands with 7 detail bands per level (the reference's w_call_soft_thresh /
// w_call_hard_thresh, do_swt or not: the same rule)
template <typename T, typename BandSize>
static int vol_thresh(int op, T** c, T beta, int L, int do_thresh_appcoeffs, int normalize, BandSize band_size)
{
    T* ptr[kVolMaxBands];
    size_t n[kVolMaxBands];
    T b[kVolMaxBands];
    int nb = 0;
    if (do_thresh_appcoeffs) {
        T beta2 = beta;
        if (normalize > 0 && op == BL_SOFT) {  // beta / sqrt(2)^nlevels, as in 2-D (src/common.cu:231-235)
            const int nl2 = L / 2;
            beta2 /= (T)(1 << nl2);
            if (nl2 * 2 != L) beta2 = (T)(beta2 / 1.4142135623730951);
        }
        ptr[nb] = c[0], n[nb] = (size_t)band_size(0), b[nb] = beta2, nb++;  // hard: the un-normalised beta (SURVEY B-4)
    }
    for (int lev = 1; lev <= L; lev++) {
        if (normalize > 0) beta = (T)(beta / 1.4142135623730951);
        for (int k = 0; k < 7; k++) {
            const int num = band3(L, lev, k);
            ptr[nb] = c[num], n[nb] = (size_t)band_size(num), b[nb] = beta, nb++;
        }
    }
    return band_list_ew<T>(op, ptr, n, b, nb);
}
template <typename T, typename BandSize>
static int vol_norm1(T** c, int L, double* out, BandSize band_size)
{
    T* ptr[kVolMaxBands];
    size_t n[kVolMaxBands];
    const int nb = 7 * L + 1;
    for (int k = 0; k < nb; k++) ptr[k] = c[k], n[k] = (size_t)band_size(k);
    return band_list_abs_sum<T>(ptr, n, nb, out);
}

// f(std::integral_constant<int, HL>) for the even HL = hlen of the bank table (2 .. 40); PDWT_EINVAL for any other length
template <int HL = 2, typename F>
static int with_filter_length(int hlen, F&& f)
{
    if constexpr (HL > PDWT_MAX_FILTER_WIDTH) {
        return PDWT_EINVAL;
    } else {
        if (hlen == HL) return f(std::integral_constant<int, HL>());
        return with_filter_length<HL + 2>(hlen, f);
    }
}

}  // namespace pdwt
