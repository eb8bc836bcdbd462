"""Reference of the ADJOINTS of the transforms with signal-extension boundary modes, in numpy (float64 for the reference proper; float32
to measure what float32 arithmetic of the kernels' order can reach).  The forward maps are those of tests/refext.py, which this module
imports and does not alter.

One level along one line of n samples, bank of even length F, N = (n + F - 1) // 2, cotangents abar, dbar of N entries:
  u[s]    = sum_i abar[i] L[2i + 1 - s] + dbar[i] H[2i + 1 - s]      s = 2 - F .. 2N - 1 (cell e = s + F - 2 of the extended line)
  xbar[k] = sum of u[s] over the s with ext_index(s) == k, in ascending s (s = k included)           -- the fold
u is the synthesis formula of refext on the coefficient lines padded with F/2 - 1 zeros, with the REVERSED analysis taps; the low and the
high sums are added once.  The adjoint of the inverse is refext.analysis in mode zero with IL and IH reversed.
2-D: columns first (A, H) and (V, D), then rows, onto the extended grid; then the fold along the rows of the grid (per extended row, ascending
sx) and along its columns (ascending sy).  Several levels: from the coarsest to the finest, the xbar of a level is the A cotangent of the next.
"""
import numpy as np

from tests import refext as R

# the GPU cases of tests/test_adjoint_gpu.py, shared with the float32 measurement of tests/test_refadj_cpu.py: (shape, bank, levels, modes)
ALL = R.MODES
CASES_2D = [
    ((7, 7), "db4", 1, ALL),                                     # halo of n - 1 samples; through the level driver
    ((33, 47), "haar", 3, ALL),                                  # odd sizes
    ((13, 18), "db2", 2, ALL),
    ((61, 67), "db4", 2, ("symmetric", "reflect")),
    ((104, 200), "db2", 2, ("symmetric", "zero", "periodic")),   # an interior tile and border tiles on all four sides
    ((48, 48), "bior2.2", 2, ("symmetric",)),
    ((96, 80), "db20", 1, ("symmetric", "periodic", "constant")),  # 40 taps, the longest gather
]
CASES_1D = [  # (rows, samples), bank, levels, modes, the form that runs
    ((5, 77), "haar", 3, ALL, "fused"),
    ((2, 4099), "db4", 5, ("symmetric", "periodic"), "fused"),
    ((2, 96), "db20", 1, ("symmetric", "constant"), "fused"),
    ((2, 40037), "db4", 3, ("symmetric", "reflect"), "levels"),
    ((70001, 16), "db2", 1, ("symmetric",), "level-driver"),     # more rows than a grid dimension
]


def synthesis_ext(abar, dbar, lo, hi):
    """u on the 2N + F - 2 cells of the extended line (last axis), the analysis taps lo, hi"""
    abar, dbar = np.asarray(abar), np.asarray(dbar)
    assert abar.dtype == dbar.dtype == lo.dtype == hi.dtype and abar.shape == dbar.shape
    F, N = len(lo), abar.shape[-1]
    pad = [(0, 0)] * (abar.ndim - 1) + [(F // 2 - 1, F // 2 - 1)]
    ap, dp = np.pad(abar, pad), np.pad(dbar, pad)
    rl, rh = lo[::-1], hi[::-1]
    e = np.arange(2 * N + F - 2)
    sa = np.zeros(abar.shape[:-1] + (e.size,), abar.dtype)
    sd = np.zeros_like(sa)
    for m in range(F // 2):  # padded coefficient (e >> 1) + m, reversed tap F-2-2m (e even) / F-1-2m (e odd)
        t = np.where(e & 1, F - 1 - 2 * m, F - 2 - 2 * m)
        sa = sa + ap[..., (e >> 1) + m] * rl[t]
        sd = sd + dp[..., (e >> 1) + m] * rh[t]
    return sa + sd


def preimages(n, F, mode):
    """(table, valid): table[k, j] = the j-th cell (ascending) of the extended line that the mode maps to sample k"""
    N = (n + F - 1) // 2
    s = np.arange(2 - F, 2 * N)
    idx, ok = R.ext_index(s, n, mode)
    lists = [[] for _ in range(n)]
    for e in range(s.size):
        if ok[e]:
            lists[int(idx[e])].append(e)
    width = max(len(l) for l in lists)
    tab = np.zeros((n, width), np.int64)
    val = np.zeros((n, width), bool)
    for k, l in enumerate(lists):
        tab[k, :len(l)] = l
        val[k, :len(l)] = True
    return tab, val


def fold(u, n, F, mode):
    """the transpose of the extension along the LAST axis: a vectorised gather in ascending s"""
    tab, val = preimages(n, F, mode)
    acc = np.zeros(u.shape[:-1] + (n,), u.dtype)
    for j in range(tab.shape[1]):
        acc = acc + np.where(val[:, j], u[..., tab[:, j]], u.dtype.type(0))
    return acc


def analysis_adjoint(abar, dbar, lo, hi, n, mode):
    """xbar (n samples along the last axis): the adjoint of refext.analysis(., lo, hi, mode)"""
    return fold(synthesis_ext(abar, dbar, lo, hi), n, len(lo), mode)


def synthesis_adjoint(xbar, ilo, ihi):
    """(abar, dbar): the adjoint of refext.synthesis(., ., ilo, ihi, n)"""
    return R.analysis(xbar, np.ascontiguousarray(ilo[::-1]), np.ascontiguousarray(ihi[::-1]), "zero")


def _T(x):
    return np.swapaxes(x, -1, -2)


def dwt2_adjoint(bands, shape, taps, mode):
    """the adjoint of refext.dwt2 on (..., nr, nc): columns, rows, fold along the rows, fold along the columns"""
    A, H, V, D = bands
    F = len(taps["L"])
    lo = _T(synthesis_ext(_T(A), _T(H), taps["L"], taps["H"]))   # (Er, hc)
    hi = _T(synthesis_ext(_T(V), _T(D), taps["L"], taps["H"]))
    U = synthesis_ext(lo, hi, taps["L"], taps["H"])              # (Er, Ec)
    return np.ascontiguousarray(_T(fold(_T(fold(U, shape[1], F, mode)), shape[0], F, mode)))


def idwt2_adjoint(xbar, taps):
    """[A, H, V, D] cotangents: the adjoint of refext.idwt2"""
    z = {"L": np.ascontiguousarray(taps["IL"][::-1]), "H": np.ascontiguousarray(taps["IH"][::-1])}
    return R.dwt2(xbar, z, "zero")


def wavedec2_adjoint(bands, shape, wname, mode, dtype=np.float64):
    """xbar of `shape` (leading axes kept) from the cotangents of refext.wavedec2's table"""
    hlen, taps = R.bank(wname, dtype)
    levels = (len(bands) - 1) // 3
    shapes = R.level_shapes(shape, hlen, levels)
    a = np.asarray(bands[0]).astype(dtype)
    for l in range(levels, 0, -1):
        a = dwt2_adjoint([a] + [np.asarray(b).astype(dtype) for b in bands[3 * (l - 1) + 1:3 * l + 1]], shapes[l - 1], taps, mode)
    return a


def waverec2_adjoint(xbar, wname, levels, dtype=np.float64):
    """the cotangent table [A_L, H1, V1, D1, ...] of refext.waverec2 from xbar"""
    _, taps = R.bank(wname, dtype)
    a = np.asarray(xbar).astype(dtype)
    det = []
    for _ in range(levels):
        a, h, v, d = idwt2_adjoint(a, taps)
        det += [h, v, d]
    return [a] + det


def lengths(n, hlen, levels):
    out = [int(n)]
    for _ in range(levels):
        out.append((out[-1] + hlen - 1) // 2)
    return out


def wavedec1(x, wname, levels, mode, dtype=np.float64):
    """[A_L, D_1, ..., D_L] along the last axis (the forward map, for the identities)"""
    _, taps = R.bank(wname, dtype)
    a = np.asarray(x).astype(dtype)
    det = []
    for _ in range(levels):
        a, d = R.analysis(a, taps["L"], taps["H"], mode)
        det.append(d)
    return [a] + det


def waverec1(bands, n, wname, dtype=np.float64):
    hlen, taps = R.bank(wname, dtype)
    levels = len(bands) - 1
    ns = lengths(n, hlen, levels)
    a = np.asarray(bands[0]).astype(dtype)
    for l in range(levels, 0, -1):
        a = R.synthesis(a, np.asarray(bands[l]).astype(dtype), taps["IL"], taps["IH"], ns[l - 1])
    return a


def wavedec1_adjoint(bands, n, wname, mode, dtype=np.float64):
    hlen, taps = R.bank(wname, dtype)
    levels = len(bands) - 1
    ns = lengths(n, hlen, levels)
    a = np.asarray(bands[0]).astype(dtype)
    for l in range(levels, 0, -1):
        a = analysis_adjoint(a, np.asarray(bands[l]).astype(dtype), taps["L"], taps["H"], ns[l - 1], mode)
    return a


def waverec1_adjoint(xbar, wname, levels, dtype=np.float64):
    _, taps = R.bank(wname, dtype)
    a = np.asarray(xbar).astype(dtype)
    det = []
    for _ in range(levels):
        a, d = synthesis_adjoint(a, taps["IL"], taps["IH"])
        det.append(d)
    return [a] + det


def dense(fn, n_in):
    """the matrix of the linear map fn on vectors of n_in entries, from unit impulses (fn returns a vector or a list of arrays)"""
    cols = []
    for j in range(n_in):
        e = np.zeros(n_in)
        e[j] = 1.0
        y = fn(e)
        cols.append(np.concatenate([np.ravel(v) for v in y]) if isinstance(y, (list, tuple)) else np.ravel(y))
    return np.stack(cols, axis=1)


def cotangent(shapes, lead, seed):
    """standard-normal float64 arrays of lead + shape whose values are float32 numbers, so that one reference serves both precisions"""
    rs = np.random.RandomState(seed)
    return [rs.standard_normal(tuple(lead) + tuple(s)).astype(np.float32).astype(np.float64) for s in shapes]


def rel_err(a, ref):
    den = np.abs(ref).max()
    return float(np.abs(np.asarray(a, np.float64) - ref).max() / (den if den > 0 else 1.0))
