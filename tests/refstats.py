"""numpy restatement of the band statistics and of the threshold rules built on them (tests/test_bandstats_*.py): what the device
kernels of bandstats.hip must reproduce for a band downloaded with get_coeff."""
import numpy as np

MAD_SCALE = 0.6744897501960817


def ref_stats(b):
    """{n, sum_abs, sum_sq, max_abs, median_abs} of a band; the median is the mean of the two middle order statistics of |b|"""
    a = np.abs(np.asarray(b)).ravel()
    n = a.size
    s = np.sort(a)
    with np.errstate(over="ignore", invalid="ignore"):
        return {"n": float(n), "sum_abs": float(a.astype(np.float64).sum()), "sum_sq": float((a.astype(np.float64) ** 2).sum()),
                "max_abs": float(a.max()), "median_abs": 0.5 * (float(s[(n - 1) // 2]) + float(s[n // 2]))}


def ref_threshold(x, beta, kind):
    """soft: copysign(max(|x| - beta, 0), x); hard: x where |x| > beta, else 0 * x -- in the dtype of x; beta < 0: untouched"""
    x = np.asarray(x)
    if beta < 0:
        return x.copy()
    b = x.dtype.type(beta)
    if kind == "soft":
        return np.copysign(np.maximum(np.abs(x) - b, x.dtype.type(0)), x)
    with np.errstate(invalid="ignore"):
        return np.where(np.abs(x) - b > 0, x, x.dtype.type(0) * x)


def ref_betas(stats, sigma, method, samples):
    """the denoise() rules in double from restated statistics: band 0 -> -1"""
    out = [-1.0]
    for s in stats[1:]:
        if method == "visu":
            out.append(sigma * np.sqrt(2.0 * np.log(samples)))
        else:
            ms = s["sum_sq"] / s["n"]
            out.append(sigma ** 2 / np.sqrt(ms - sigma ** 2) if ms > sigma ** 2 else s["max_abs"])
    return np.array(out, dtype=np.float64)
