"""Reference of the 2-D DWT with signal-extension boundary modes (BoundaryWavelets) for the tests, in numpy: the index map of the five
modes, the two one-level formulas on lines, and rows-then-columns multi-level with the band order of Wavelets.  Nothing here touches
pdwt_amd; only the taps come from the oracle.

One level along one axis, a line x of n samples, a bank of even length F (L = dec_lo, H = dec_hi, IL = rec_lo, IH = rec_hi):
  forward   N = (n + F - 1) // 2,  a[i] = sum_k L[k] xe[2i + 1 - k],  d[i] = sum_k H[k] xe[2i + 1 - k]   (np.convolve(xe, L)[1::2])
  inverse   x[k] = sum_i a[i] IL[k + F - 2 - 2i] + d[i] IH[k + F - 2 - 2i]  over the i with a tap index in 0 .. F-1, k = 0 .. n-1
xe is x extended by the mode (PyWavelets' names): zero, constant, symmetric (half-sample mirror), reflect (whole-sample mirror; one
sample: the constant), periodic.  The sums run in ascending order of the sample index of the window, in the dtype asked for (float64
for the reference proper; float32 to measure what float32 arithmetic of this order can reach).
Bands: [A_L, H1, V1, D1, ..., H_L, V_L, D_L], level 1 the finest; A = row low / column low, H = row low / column high, V = row high /
column low, D = row high / column high ("row low" = the low pass along the rows, i.e. along axis 1).
"""
import numpy as np

from oracle import oracle as orc

MODES = ("zero", "constant", "symmetric", "reflect", "periodic")
MAX_LEVELS = 32

# the cases of the GPU tests (tests/test_ext2d_gpu.py), shared with the CPU checks of this reference: (shape, bank, levels, modes)
ALL = MODES
CASES = [
    ((7, 7), "db4", 1, ALL),                            # halo of n - 1 samples (below the level clamp of the class: level drivers)
    ((64, 64), "db2", 3, ALL),                          # multi-level, even sizes
    ((33, 47), "haar", 3, ALL),                         # odd sizes: the mode-dependent last sample
    ((61, 67), "db4", 2, ("symmetric", "reflect")),     # bands that cross one tile boundary
    ((104, 200), "db2", 2, ("symmetric", "zero")),      # an interior forward tile and border tiles on all four sides
    ((40, 72), "coif1", 2, ("symmetric",)),
    ((48, 48), "bior2.2", 2, ("symmetric",)),
    ((64, 96), "sym8", 2, ("symmetric",)),
    ((96, 80), "db20", 1, ("symmetric", "periodic")),   # 40 taps
]


def bank(wname, dtype=np.float64):
    """(F, {L, H, IL, IH}) in `dtype` (the float64 taps of the table rounded once)"""
    h, taps, _ = orc.filters(wname, np.float64)
    return h, {k: v.astype(dtype) for k, v in taps.items()}


def clamp_levels(shape, hlen, levels):
    """ilog2(min(Nr, Nc) / (hlen - 1)) as in Wavelets (PyWavelets' dwt_max_level), at most MAX_LEVELS; at least one level is asked for"""
    return max(0, min(max(int(levels), 1), orc.ilog2(min(shape) // (hlen - 1)), MAX_LEVELS))


def level_shapes(shape, hlen, levels):
    """[(nr_l, nc_l) for l = 0 .. levels]: the image, then the bands of each level"""
    out = [tuple(int(v) for v in shape)]
    for _ in range(levels):
        out.append(((out[-1][0] + hlen - 1) // 2, (out[-1][1] + hlen - 1) // 2))
    return out


def band_shapes(shape, hlen, levels):
    s = level_shapes(shape, hlen, levels)
    return [s[levels]] + [s[l] for l in range(1, levels + 1) for _ in range(3)]


def ext_index(j, n, mode):
    """(index into the line, valid) of xe[j] for an integer array j; valid is False where the sample is 0 (mode zero)"""
    j = np.asarray(j, np.int64)
    inside = (j >= 0) & (j < n)
    if mode == "zero":
        return np.clip(j, 0, n - 1), inside
    if mode == "constant":
        m = np.clip(j, 0, n - 1)
    elif mode == "symmetric":
        m = np.mod(j, 2 * n)
        m = np.where(m < n, m, 2 * n - 1 - m)
    elif mode == "reflect":
        if n == 1:
            m = np.zeros_like(j)
        else:
            m = np.mod(j, 2 * n - 2)
            m = np.where(m < n, m, 2 * n - 2 - m)
    elif mode == "periodic":
        m = np.mod(j, n)
    else:
        raise ValueError(mode)
    return m, np.ones(j.shape, bool)


def extend(x, lo, hi, mode):
    """xe[lo .. hi) of the last axis"""
    x = np.asarray(x)
    idx, ok = ext_index(np.arange(lo, hi), x.shape[-1], mode)
    return np.where(ok, x[..., idx], x.dtype.type(0))


def analysis(x, lo, hi, mode):
    """(a, d) along the LAST axis"""
    x = np.asarray(x)
    assert x.dtype == lo.dtype == hi.dtype, (x.dtype, lo.dtype)
    n, F = x.shape[-1], len(lo)
    N = (n + F - 1) // 2
    xe = extend(x, 2 - F, 2 * N, mode)  # xe[j] at position j + F - 2
    a = np.zeros(x.shape[:-1] + (N,), x.dtype)
    d = np.zeros_like(a)
    for j in range(F):  # ascending sample index: tap F-1-j on the sample 2i + 1 - (F-1-j)
        v = xe[..., j:j + 2 * N:2]
        a = a + v * lo[F - 1 - j]
        d = d + v * hi[F - 1 - j]
    return a, d


def synthesis(a, d, ilo, ihi, n):
    """the n samples along the LAST axis from N = (n + F - 1) // 2 coefficients per band; no extension"""
    a, d = np.asarray(a), np.asarray(d)
    assert a.dtype == d.dtype == ilo.dtype == ihi.dtype and a.shape == d.shape
    F = len(ilo)
    assert a.shape[-1] == (n + F - 1) // 2, (a.shape, n, F)
    k = np.arange(n)
    sa = np.zeros(a.shape[:-1] + (n,), a.dtype)
    sd = np.zeros_like(sa)
    for m in range(F // 2):  # coefficient (k >> 1) + m, tap F-2-2m (k even) / F-1-2m (k odd)
        t = np.where(k & 1, F - 1 - 2 * m, F - 2 - 2 * m)
        sa = sa + a[..., (k >> 1) + m] * ilo[t]
        sd = sd + d[..., (k >> 1) + m] * ihi[t]
    return sa + sd


def _T(x):
    return np.swapaxes(x, -1, -2)


def dwt2(x, taps, mode):
    """[A, H, V, D] of one level: rows first (axis 1), then columns (axis 0)"""
    lo, hi = analysis(x, taps["L"], taps["H"], mode)
    A, H = analysis(_T(lo), taps["L"], taps["H"], mode)
    V, D = analysis(_T(hi), taps["L"], taps["H"], mode)
    return [np.ascontiguousarray(_T(b)) for b in (A, H, V, D)]


def idwt2(bands, shape, taps):
    A, H, V, D = bands
    lo = _T(synthesis(_T(A), _T(H), taps["IL"], taps["IH"], shape[0]))
    hi = _T(synthesis(_T(V), _T(D), taps["IL"], taps["IH"], shape[0]))
    return np.ascontiguousarray(synthesis(lo, hi, taps["IL"], taps["IH"], shape[1]))


def wavedec2(x, wname, levels, mode, dtype=np.float64):
    """[A_L, H1, V1, D1, ..., H_L, V_L, D_L] of exactly `levels` levels (not clamped), computed in `dtype`"""
    _, taps = bank(wname, dtype)
    a = np.asarray(x).astype(dtype)
    det = []
    for _ in range(levels):
        a, h, v, d = dwt2(a, taps, mode)
        det += [h, v, d]
    return [a] + det


def waverec2(bands, shape, wname, dtype=np.float64):
    """the image of `shape` from the band table of wavedec2"""
    hlen, taps = bank(wname, dtype)
    levels = (len(bands) - 1) // 3
    shapes = level_shapes(shape, hlen, levels)
    a = np.asarray(bands[0]).astype(dtype)
    for l in range(levels, 0, -1):
        a = idwt2([a] + [np.asarray(b).astype(dtype) for b in bands[3 * (l - 1) + 1:3 * l + 1]], shapes[l - 1], taps)
    return a
