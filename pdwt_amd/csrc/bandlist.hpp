// bandlist.hpp -- the elementwise and reduction kernels of utils.hip over an explicit list of bands (the 3-D band walk of
// dwt3d.hip; the 1-D / 2-D entry points derive their list from pdwt_info instead).
#pragma once
#include <stddef.h>

namespace pdwt {
enum BandListOp { BL_SOFT = 0, BL_HARD = 1 };
// in place: band k (ptr[k], n[k] elements) <- op(band k, beta[k]); at most 97 bands, one launch
template <typename T> int band_list_ew(int op, T* const* ptr, const size_t* n, const T* beta, int nb);
// sum |c| over the bands, accumulated in double; synchronises and writes *out
template <typename T> int band_list_abs_sum(T* const* ptr, const size_t* n, int nb, double* out);
// per-band statistics (bandstats.hip): n, sum |c|, sum c^2, max |c| of every band in one launch, and the exact median of |c|
// of the bands with want_median[k] != 0 (NULL: none; NaN where not asked for or n[k] == 0); want_median[k] == 2 asks for the median
// ALONE (no moments pass over band k: its sums and max are NaN); synchronises and fills out[0 .. nb)
struct BandStats { double n, sum_abs, sum_sq, max_abs, median_abs; };
template <typename T> int band_list_stats(T* const* ptr, const size_t* n, int nb, const unsigned char* want_median, BandStats* out);
}  // namespace pdwt
