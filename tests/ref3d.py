"""A float64 direct-sum reference of the periodised 1-D and 3-D wavelet transforms, decimated and stationary (a-trous).

Plain numpy, written from the definitions below and not from the oracle's loops; it always computes in float64, whatever the
precision under test.  The only thing it takes from the project is the tap values (``bank``); tests/test_ref3d_cpu.py pins it
against the oracle's 1-D level, the numpy a-trous composition, the PyWavelets goldens and closed-form properties.

Definitions (F a filter of even length hlen, indices from 0):
  decimated analysis   out[i] = sum_j xe[2i - c + j] * F[hlen-1-j],  c = hlen/2 - 1,  j = 0 .. hlen-1,  i = 0 .. (n+1)//2 - 1
                       xe = the periodic extension of the line after repeating its last sample when its length n is odd
  decimated synthesis  g' = g + shift, p = g' // 2, off = 1 - (g' & 1), c = (hlen/2) // 2, shift = 0 if hlen/2 is odd else 1
                       out[g] = sum_{j < hlen/2} a[(p - c + j) mod nin] * IL[hlen-1-(2j+off)] + d[(p - c + j) mod nin] * IH[...]
  a-trous analysis     out[g] = sum_k x[(g - c + f*k) mod n] * F[hlen-1-k],  c = (hlen/2 - 1) * f,  f = 2^(lev-1)
  a-trous synthesis    out[g] = sum_k (a[(g - c + f*k) mod n] * IL[hlen-1-k] + d[...] * IH[hlen-1-k]) / 2,  c = (hlen/2) * f
  3-D level            x (axis 2), then y (axis 1), then z (axis 0); the inverse z, y, x; details in BAND_KEYS order (first
                       letter = z axis); further levels on the aaa band; coefficient list [A_L, level L .. level 1].
"""
import numpy as np

from oracle import oracle as orc

BAND_KEYS = ("aad", "ada", "add", "daa", "dad", "dda", "ddd")  # restated, not imported: storage order of a level's details


def bank(wname, do_swt=0, dt=np.float64):
    """(L, H, IL, IH) of a bank: the float64 taps, rounded to `dt`"""
    _, F, _ = orc.filters(wname, np.float64, do_swt)
    return tuple(np.asarray(F[k], np.float64).astype(dt) for k in ("L", "H", "IL", "IH"))


def _along(vec, ndim, axis):
    """a 1-D array as an ndim array that varies along `axis` only"""
    shape = [1] * ndim
    shape[axis] = len(vec)
    return np.asarray(vec).reshape(shape)


# ---- one level along an axis ----------------------------------------------------------------------------
def dwt_ana(x, axis, F, dt=np.float64):
    """(lo, hi) of the decimated analysis along `axis`; output length (n + 1) // 2"""
    x = np.asarray(x, dt)
    FL, FH = F[0], F[1]
    hlen, n = len(FL), x.shape[axis]
    if n & 1:  # repeat the last sample: the extended line has even length
        x = np.concatenate([x, np.take(x, [n - 1], axis=axis)], axis=axis)
    ne = x.shape[axis]
    c = hlen // 2 - 1
    i = np.arange((n + 1) // 2)
    lo = hi = 0.0
    for j in range(hlen):
        v = np.take(x, (2 * i - c + j) % ne, axis=axis)
        lo = lo + v * FL[hlen - 1 - j]
        hi = hi + v * FH[hlen - 1 - j]
    return lo, hi


def dwt_syn(a, d, axis, nout, F, dt=np.float64):
    """the decimated synthesis along `axis` of the low branch a and the high branch d into nout samples"""
    a, d = np.asarray(a, dt), np.asarray(d, dt)
    IL, IH = F[2], F[3]
    hlen, nin = len(IL), a.shape[axis]
    h2 = hlen // 2
    c = h2 // 2
    shift = 0 if h2 & 1 else 1
    gp = np.arange(nout) + shift
    p, off = gp // 2, 1 - (gp & 1)
    out = 0.0
    for j in range(h2):
        idx = (p - c + j) % nin
        t = hlen - 1 - (2 * j + off)  # tap index per output sample
        out = out + np.take(a, idx, axis=axis) * _along(IL[t], a.ndim, axis) + np.take(d, idx, axis=axis) * _along(IH[t], a.ndim, axis)
    return out


def swt_ana(x, axis, F, f, dt=np.float64):
    """(lo, hi) of the a-trous analysis along `axis` at tap spacing f"""
    x = np.asarray(x, dt)
    FL, FH = F[0], F[1]
    hlen, n = len(FL), x.shape[axis]
    c = (hlen // 2 - 1) * f
    g = np.arange(n)
    lo = hi = 0.0
    for k in range(hlen):
        v = np.take(x, (g - c + f * k) % n, axis=axis)
        lo = lo + v * FL[hlen - 1 - k]
        hi = hi + v * FH[hlen - 1 - k]
    return lo, hi


def swt_syn(a, d, axis, F, f, dt=np.float64):
    """the a-trous synthesis along `axis` at tap spacing f"""
    a, d = np.asarray(a, dt), np.asarray(d, dt)
    IL, IH = F[2], F[3]
    hlen, n = len(IL), a.shape[axis]
    c = (hlen // 2) * f
    g = np.arange(n)
    out = 0.0
    for k in range(hlen):
        idx = (g - c + f * k) % n
        out = out + np.take(a, idx, axis=axis) * IL[hlen - 1 - k] + np.take(d, idx, axis=axis) * IH[hlen - 1 - k]
    return out / 2


# ---- batched 1-D, several levels: lines along the last axis, [A_L, D_1 .. D_L] ---------------------------------
def dwt1d_forward(lines, wname, L):
    F = bank(wname, 0)
    a, det = np.asarray(lines, np.float64), []
    for _ in range(L):
        a, d = dwt_ana(a, -1, F)
        det.append(d)
    return [a] + det


def dwt1d_inverse(coeffs, n, wname):
    F = bank(wname, 0)
    L = len(coeffs) - 1
    sizes = [n]
    for _ in range(L):
        sizes.append((sizes[-1] + 1) // 2)
    a = coeffs[0]
    for lev in range(L, 0, -1):
        a = dwt_syn(a, coeffs[lev], -1, sizes[lev - 1], F)
    return a


def swt1d_forward(lines, wname, L):
    F = bank(wname, 1)
    a, det = np.asarray(lines, np.float64), []
    for lev in range(1, L + 1):
        a, d = swt_ana(a, -1, F, 2 ** (lev - 1))
        det.append(d)
    return [a] + det


def swt1d_inverse(coeffs, wname):
    F = bank(wname, 1)
    a = coeffs[0]
    for lev in range(len(coeffs) - 1, 0, -1):
        a = swt_syn(a, coeffs[lev], -1, F, 2 ** (lev - 1))
    return a


# ---- 3-D ---------------------------------------------------------------------------------------------
def _ana3(a, ana):
    bands = {"": a}
    for axis in (2, 1, 0):  # x, then y, then z: the key grows to the left, so its first letter is the z band
        nxt = {}
        for key, b in bands.items():
            nxt["a" + key], nxt["d" + key] = ana(b, axis)
        bands = nxt
    return bands


def _syn3(d, syn):
    """d: the 8 bands of a level by key; syn(a, d, axis) along z, then y, then x"""
    q = {k: syn(d["a" + k], d["d" + k], 0) for k in ("aa", "ad", "da", "dd")}
    r = {k: syn(q["a" + k], q["d" + k], 1) for k in ("a", "d")}
    return syn(r["a"], r["d"], 2)


def _pack(a, per_level):
    out = [a]
    for lev in range(len(per_level), 0, -1):
        out += per_level[lev - 1]
    return out


def _level_bands(coeffs, L, lev, a):
    d = dict(zip(BAND_KEYS, coeffs[1 + 7 * (L - lev):8 + 7 * (L - lev)]))
    d["aaa"] = a
    return d


def dwt3_forward(vol, wname, L, dt=np.float64):
    """dt = float32: the same sums with float32 taps, products and accumulators (what a float32 kernel can be held to)"""
    F = bank(wname, 0, dt)
    a, per_level = np.asarray(vol, dt), []
    for _ in range(L):
        b = _ana3(a, lambda v, axis: dwt_ana(v, axis, F, dt))
        per_level.append([b[k] for k in BAND_KEYS])
        a = b["aaa"]
    return _pack(a, per_level)


def dwt3_inverse(coeffs, shape, wname, L, dt=np.float64):
    F = bank(wname, 0, dt)
    shapes = [tuple(shape)]
    for _ in range(L):
        shapes.append(tuple((s + 1) // 2 for s in shapes[-1]))
    a = coeffs[0]
    for lev in range(L, 0, -1):
        nout = shapes[lev - 1]
        a = _syn3(_level_bands(coeffs, L, lev, a), lambda lo, hi, axis: dwt_syn(lo, hi, axis, nout[axis], F, dt))
    return a


def swt3_forward(vol, wname, L, dt=np.float64):
    F = bank(wname, 1, dt)
    a, per_level = np.asarray(vol, dt), []
    for lev in range(1, L + 1):
        f = 2 ** (lev - 1)
        b = _ana3(a, lambda v, axis: swt_ana(v, axis, F, f, dt))
        per_level.append([b[k] for k in BAND_KEYS])
        a = b["aaa"]
    return _pack(a, per_level)


def swt3_inverse(coeffs, wname, L, dt=np.float64):
    F = bank(wname, 1, dt)
    a = coeffs[0]
    for lev in range(L, 0, -1):
        f = 2 ** (lev - 1)
        a = _syn3(_level_bands(coeffs, L, lev, a), lambda lo, hi, axis: swt_syn(lo, hi, axis, F, f, dt))
    return a


def levels_of(shape, wname, levels):
    """the level clamp of both 3-D classes: min(levels, floor(log2(min(shape) // (hlen - 1))))"""
    hlen = len(bank(wname, 0)[0])
    q, L = min(shape) // max(hlen - 1, 1), 0
    while q > 1:
        q, L = q // 2, L + 1
    return min(levels, L)
