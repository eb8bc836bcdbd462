"""The float64 direct-sum reference of the 2-D transforms of ``pdwt_amd.Wavelets`` (decimated and stationary, any number of
levels), composed from the per-axis primitives of tests/ref3d.py, which are written from the definitions and not from the oracle's
loops (the *_direct functions), and the same sums as one matrix per axis and level (the functions without the suffix, which the
tests use: two orders of magnitude faster).  ``forward`` / ``inverse`` dispatch over the four kinds, batched 1-D included.
tests/test_ref2d_cpu.py pins the band order and the odd-size rule against the PyWavelets goldens and the oracle.

  one level       rows first (axis 1: lo, hi), then columns (axis 0):  A = lo_y(lo_x)  H = hi_y(lo_x)  V = lo_y(hi_x)  D = hi_y(hi_x)
  inverse level   columns first: t1 = syn_y(A, H), t2 = syn_y(V, D); then rows: out = syn_x(t1, t2)
  odd sizes       (decimated) ref3d.dwt_ana repeats the last sample of an odd line, bands have (n + 1) // 2 samples; the synthesis
                  drops the last row / column of an odd output size
  band order      [A_L, H1, V1, D1, H2, V2, D2, ... HL, VL, DL]  (level 1 = finest; the class's get_coeff order)
  level clamp     min(levels, floor(log2(N // (hlen - 1)))), N = min(shape) in 2-D and the row length in 1-D
"""
import functools

import numpy as np

from tests import ref3d

KINDS = ("dwt2", "swt2", "dwt1", "swt1")


def levels_of(shape, wname, levels, kind="dwt2"):
    hlen = len(ref3d.bank(wname, 0)[0])
    n = min(shape) if kind in ("dwt2", "swt2") else shape[-1]
    q, L = n // max(hlen - 1, 1), 0
    while q > 1:
        q, L = q // 2, L + 1
    return min(max(levels, 1), L)


def _ana2(a, ana):
    lo, hi = ana(a, 1)
    A, H = ana(lo, 0)
    V, D = ana(hi, 0)
    return A, H, V, D


def _syn2(A, H, V, D, syn):
    return syn(syn(A, H, 0), syn(V, D, 0), 1)


def dwt2_forward_direct(img, wname, L):
    F = ref3d.bank(wname, 0)
    a, out = np.asarray(img, np.float64), []
    for _ in range(L):
        a, H, V, D = _ana2(a, lambda v, axis: ref3d.dwt_ana(v, axis, F))
        out += [H, V, D]
    return [a] + out


def dwt2_inverse_direct(coeffs, shape, wname):
    F = ref3d.bank(wname, 0)
    L = (len(coeffs) - 1) // 3
    shapes = [tuple(shape)]
    for _ in range(L):
        shapes.append(tuple((s + 1) // 2 for s in shapes[-1]))
    a = np.asarray(coeffs[0], np.float64)
    for lev in range(L, 0, -1):
        nout = shapes[lev - 1]
        H, V, D = coeffs[3 * lev - 2:3 * lev + 1]
        a = _syn2(a, H, V, D, lambda lo, hi, axis: ref3d.dwt_syn(lo, hi, axis, nout[axis], F))
    return a


def swt2_forward_direct(img, wname, L):
    F = ref3d.bank(wname, 1)
    a, out = np.asarray(img, np.float64), []
    for lev in range(1, L + 1):
        f = 2 ** (lev - 1)
        a, H, V, D = _ana2(a, lambda v, axis: ref3d.swt_ana(v, axis, F, f))
        out += [H, V, D]
    return [a] + out


def swt2_inverse_direct(coeffs, wname):
    F = ref3d.bank(wname, 1)
    L = (len(coeffs) - 1) // 3
    a = np.asarray(coeffs[0], np.float64)
    for lev in range(L, 0, -1):
        f = 2 ** (lev - 1)
        H, V, D = coeffs[3 * lev - 2:3 * lev + 1]
        a = _syn2(a, H, V, D, lambda lo, hi, axis: ref3d.swt_syn(lo, hi, axis, F, f))
    return a


# ---- the same sums as matrices ---------------------------------------------------------------------------------------------------
# The all-banks GPU module evaluates this reference some ten thousand times.  Along one axis every transform above is a linear map with
# a few non-zero taps per row, so the definitions of tests/ref3d.py are written down once per (bank, length, tap spacing) as dense
# float64 matrices -- entry by entry from the same index formulas, not by running the primitives -- and a level is two products.
# tests/test_ref2d_cpu.py holds the two forms to each other (the summation order differs: 1e-14).
@functools.lru_cache(maxsize=48)
def _ana_matrix(wname, n, f, mag=False):
    """(n_out x n) matrices (lo, hi) of the analysis along a line of n samples; f = 0: decimated, f >= 1: a-trous at tap spacing f;
    mag: of the magnitudes of the taps (see support)"""
    FL, FH = _bank(wname, f, mag)[:2]
    hlen = len(FL)
    if f:
        ne, rows, first = n, np.arange(n), np.arange(n) - (hlen // 2 - 1) * f
    else:
        ne = n + (n & 1)  # the line after repeating its last sample
        rows, first = np.arange(ne // 2), 2 * np.arange(ne // 2) - (hlen // 2 - 1)
    lo, hi = np.zeros((len(rows), ne)), np.zeros((len(rows), ne))
    for j in range(hlen):
        cols = (first + (f or 1) * j) % ne
        np.add.at(lo, (rows, cols), FL[hlen - 1 - j])
        np.add.at(hi, (rows, cols), FH[hlen - 1 - j])
    if ne != n:  # the repeated sample is the last one
        lo[:, n - 1] += lo[:, n]
        hi[:, n - 1] += hi[:, n]
        lo, hi = lo[:, :n], hi[:, :n]
    return np.ascontiguousarray(lo), np.ascontiguousarray(hi)


@functools.lru_cache(maxsize=48)
def _syn_matrix(wname, nin, nout, f):
    """(nout x nin) matrices (from the low branch, from the high branch) of the synthesis; f = 0: decimated into nout samples"""
    IL, IH = ref3d.bank(wname, 1 if f else 0)[2:]
    hlen = len(IL)
    sa, sd = np.zeros((nout, nin)), np.zeros((nout, nin))
    g = np.arange(nout)
    if f:
        for k in range(hlen):
            cols = (g - (hlen // 2) * f + f * k) % nin
            np.add.at(sa, (g, cols), IL[hlen - 1 - k] / 2)
            np.add.at(sd, (g, cols), IH[hlen - 1 - k] / 2)
        return sa, sd
    h2 = hlen // 2
    gp = g + (0 if h2 & 1 else 1)
    p, off = gp // 2, 1 - (gp & 1)
    for j in range(h2):
        cols, t = (p - h2 // 2 + j) % nin, hlen - 1 - (2 * j + off)
        np.add.at(sa, (g, cols), IL[t])
        np.add.at(sd, (g, cols), IH[t])
    return sa, sd


def _bank(wname, f, mag):
    F = ref3d.bank(wname, 1 if f else 0)
    return tuple(np.abs(t) for t in F) if mag else F


_DENSE_MAX = 4096  # longer lines (the 8192-sample rows of the batched 1-D one-buffer kernels) run the primitives themselves


def _ana(x, axis, wname, f, mag=False):
    if x.shape[axis] > _DENSE_MAX:
        F = _bank(wname, f, mag)
        return ref3d.swt_ana(x, axis, F, f) if f else ref3d.dwt_ana(x, axis, F)
    lo, hi = _ana_matrix(wname, x.shape[axis], f, mag)
    return (lo @ x, hi @ x) if axis == 0 else (x @ lo.T, x @ hi.T)


def _syn(a, d, axis, wname, nout, f):
    if nout > _DENSE_MAX:
        F = ref3d.bank(wname, 1 if f else 0)
        return ref3d.swt_syn(a, d, axis, F, f) if f else ref3d.dwt_syn(a, d, axis, nout, F)
    sa, sd = _syn_matrix(wname, a.shape[axis], nout, f)
    return sa @ a + sd @ d if axis == 0 else a @ sa.T + d @ sd.T


def _sizes(n, L):
    out = [n]
    for _ in range(L):
        out.append((out[-1] + 1) // 2)
    return out


def dwt2_forward(img, wname, L, mag=False):
    a, out = np.asarray(img, np.float64), []
    for _ in range(L):
        a, H, V, D = _ana2(a, lambda v, axis: _ana(v, axis, wname, 0, mag))
        out += [H, V, D]
    return [a] + out


def dwt2_inverse(coeffs, shape, wname):
    L = (len(coeffs) - 1) // 3
    nr, nc = _sizes(shape[0], L), _sizes(shape[1], L)
    a = np.asarray(coeffs[0], np.float64)
    for lev in range(L, 0, -1):
        nout = (nr[lev - 1], nc[lev - 1])
        H, V, D = coeffs[3 * lev - 2:3 * lev + 1]
        a = _syn2(a, H, V, D, lambda lo, hi, axis: _syn(lo, hi, axis, wname, nout[axis], 0))
    return a


def swt2_forward(img, wname, L, mag=False):
    a, out = np.asarray(img, np.float64), []
    for lev in range(1, L + 1):
        a, H, V, D = _ana2(a, lambda v, axis: _ana(v, axis, wname, 2 ** (lev - 1), mag))
        out += [H, V, D]
    return [a] + out


def swt2_inverse(coeffs, wname):
    L = (len(coeffs) - 1) // 3
    a = np.asarray(coeffs[0], np.float64)
    for lev in range(L, 0, -1):
        H, V, D = coeffs[3 * lev - 2:3 * lev + 1]
        a = _syn2(a, H, V, D, lambda lo, hi, axis: _syn(lo, hi, axis, wname, lo.shape[axis], 2 ** (lev - 1)))
    return a


def dwt1d_forward(lines, wname, L, mag=False):
    a, det = np.asarray(lines, np.float64), []
    for _ in range(L):
        a, d = _ana(a, 1, wname, 0, mag)
        det.append(d)
    return [a] + det


def dwt1d_inverse(coeffs, n, wname):
    L = len(coeffs) - 1
    sizes = _sizes(n, L)
    a = coeffs[0]
    for lev in range(L, 0, -1):
        a = _syn(a, coeffs[lev], 1, wname, sizes[lev - 1], 0)
    return a


def swt1d_forward(lines, wname, L, mag=False):
    a, det = np.asarray(lines, np.float64), []
    for lev in range(1, L + 1):
        a, d = _ana(a, 1, wname, 2 ** (lev - 1), mag)
        det.append(d)
    return [a] + det


def swt1d_inverse(coeffs, wname):
    a = coeffs[0]
    for lev in range(len(coeffs) - 1, 0, -1):
        a = _syn(a, coeffs[lev], 1, wname, a.shape[1], 2 ** (lev - 1))
    return a


def forward_direct(kind, x, wname, L):
    """the compositions of the ref3d primitives themselves (slow): what the matrix forms are pinned to"""
    x = np.asarray(x, np.float64)
    return {"dwt2": dwt2_forward_direct, "swt2": swt2_forward_direct, "dwt1": ref3d.dwt1d_forward, "swt1": ref3d.swt1d_forward}[kind](x, wname, L)


def inverse_direct(kind, coeffs, shape, wname):
    coeffs = [np.asarray(c, np.float64) for c in coeffs]
    if kind == "dwt2":
        return dwt2_inverse_direct(coeffs, shape, wname)
    if kind == "dwt1":
        return ref3d.dwt1d_inverse(coeffs, shape[-1], wname)
    return (swt2_inverse_direct if kind == "swt2" else ref3d.swt1d_inverse)(coeffs, wname)


def support(kind, x, wname, L):
    """the forward transform of |x| with the magnitudes of the taps: positive wherever ANY product of a non-zero sample with non-zero
    taps reaches a coefficient, exactly zero elsewhere.  Where it is zero every term of the coefficient is a product with a zero, so
    the coefficient is zero in any precision and any summation order (zeros of ``forward`` itself may be cancellations)"""
    return forward(kind, np.abs(np.asarray(x, np.float64)), wname, L, mag=True)


def forward(kind, x, wname, L, mag=False):
    """the coefficient list of ``Wavelets(x, wname, L, do_swt, ndim)`` in the class's band order"""
    x = np.asarray(x, np.float64)
    if kind == "dwt2":
        return dwt2_forward(x, wname, L, mag)
    if kind == "swt2":
        return swt2_forward(x, wname, L, mag)
    if kind == "dwt1":
        return dwt1d_forward(x, wname, L, mag)
    if kind == "swt1":
        return swt1d_forward(x, wname, L, mag)
    raise KeyError(kind)


def inverse(kind, coeffs, shape, wname):
    coeffs = [np.asarray(c, np.float64) for c in coeffs]
    if kind == "dwt2":
        return dwt2_inverse(coeffs, shape, wname)
    if kind == "swt2":
        return swt2_inverse(coeffs, wname)
    if kind == "dwt1":
        return dwt1d_inverse(coeffs, shape[-1], wname)
    if kind == "swt1":
        return swt1d_inverse(coeffs, wname)
    raise KeyError(kind)
