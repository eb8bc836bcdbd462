"""Reference of the 3-D DWT of volumes with signal-extension boundary modes (BoundaryWavelets3D) for the tests, in numpy: the one-level
formulas of tests/refext.py (`analysis` / `synthesis` on the last axis) applied along axis 2 (x), then 1 (y), then 0 (z), and back in
the order z, y, x.  Nothing here touches pdwt_amd; only the taps come from the oracle (through tests/refext.py).

Bands: the order of Wavelets3D / pywt.wavedecn, [A_L, the 7 details of level L, ..., those of level 1]; detail k of level lev (1 =
finest) is band 1 + 7 * (L - lev) + k, k in BAND_KEYS order (first letter = z axis, "a" = low pass).  A level's eight bands in the
order of the level drivers: LEVEL_KEYS = aaa, aad, ..., ddd.
"""
import numpy as np

from tests import refext as R

MODES = R.MODES
MAX_LEVELS = 13
BAND_KEYS = ("aad", "ada", "add", "daa", "dad", "dda", "ddd")  # restated, not imported: storage order of a level's details
LEVEL_KEYS = ("aaa",) + BAND_KEYS

# the cases of the GPU tests (tests/test_ext3d_gpu.py), shared with the CPU checks of this reference: (shape, bank, levels, modes)
ALL = MODES
CASES = [
    ((7, 7, 7), "db4", 1, ALL),                          # halo of n - 1 samples on all three axes (below the clamp of the class: level drivers)
    ((16, 16, 16), "db2", 2, ALL),                       # multi-level, even sizes; bands 9^3 then 6^3
    ((9, 33, 47), "haar", 3, ALL),                       # odd sizes on every axis: the mode-dependent last sample
    ((40, 24, 24), "db2", 2, ("symmetric", "zero")),     # 21 output planes: two z chunks, the second partial; the inverse crosses a z chunk
    ((6, 104, 200), "db2", 1, ("symmetric", "zero")),    # an interior x-y forward tile with border tiles on all four sides, in every plane
    ((24, 28, 32), "bior2.2", 2, ("reflect",)),          # the analysis bank is not the synthesis bank
    ((30, 32, 36), "sym8", 1, ("symmetric",)),
    ((40, 48, 40), "db20", 1, ("symmetric", "periodic")),  # 40 taps (level drivers)
]
DRIVER_CASES = ((7, 7, 7), (40, 48, 40))  # the shapes that run through the level drivers


def bank(wname, dtype=np.float64):
    return R.bank(wname, dtype)


def clamp_levels(shape, hlen, levels):
    """ilog2(min(Nz, Nr, Nc) / (hlen - 1)) as in Wavelets3D, at most MAX_LEVELS; at least one level is asked for"""
    return max(0, min(max(int(levels), 1), R.orc.ilog2(min(shape) // (hlen - 1)), MAX_LEVELS))


def level_shapes(shape, hlen, levels):
    """[(nz_l, nr_l, nc_l) for l = 0 .. levels]: the volume, then the bands of each level"""
    out = [tuple(int(v) for v in shape)]
    for _ in range(levels):
        out.append(tuple((n + hlen - 1) // 2 for n in out[-1]))
    return out


def band_shapes(shape, hlen, levels):
    s = level_shapes(shape, hlen, levels)
    return [s[levels]] + [s[l] for l in range(levels, 0, -1) for _ in range(7)]


def _ana_axis(x, axis, taps, mode):
    a, d = R.analysis(np.ascontiguousarray(np.moveaxis(x, axis, -1)), taps["L"], taps["H"], mode)
    return np.moveaxis(a, -1, axis), np.moveaxis(d, -1, axis)


def _syn_axis(a, d, axis, taps, n):
    out = R.synthesis(np.ascontiguousarray(np.moveaxis(a, axis, -1)), np.ascontiguousarray(np.moveaxis(d, axis, -1)), taps["IL"], taps["IH"], n)
    return np.moveaxis(out, -1, axis)


def dwt3(x, taps, mode):
    """{key: band} of one level: x (axis 2), then y (axis 1), then z (axis 0); the key grows to the left, so its first letter is z"""
    bands = {"": x}
    for axis in (2, 1, 0):
        nxt = {}
        for key, b in bands.items():
            nxt["a" + key], nxt["d" + key] = _ana_axis(b, axis, taps, mode)
        bands = nxt
    return {k: np.ascontiguousarray(v) for k, v in bands.items()}


def idwt3(bands, shape, taps):
    """the volume of `shape` from the eight bands by key: z, then y, then x"""
    q = {k: _syn_axis(bands["a" + k], bands["d" + k], 0, taps, shape[0]) for k in ("aa", "ad", "da", "dd")}
    r = {k: _syn_axis(q["a" + k], q["d" + k], 1, taps, shape[1]) for k in ("a", "d")}
    return np.ascontiguousarray(_syn_axis(r["a"], r["d"], 2, taps, shape[2]))


def wavedec3(x, wname, levels, mode, dtype=np.float64):
    """[A_L, level L ... level 1] of exactly `levels` levels (not clamped), computed in `dtype`"""
    _, taps = bank(wname, dtype)
    a = np.asarray(x).astype(dtype)
    per_level = []
    for _ in range(levels):
        b = dwt3(a, taps, mode)
        per_level.append([b[k] for k in BAND_KEYS])
        a = b["aaa"]
    out = [a]
    for lev in range(levels, 0, -1):
        out += per_level[lev - 1]
    return out


def waverec3(bands, shape, wname, dtype=np.float64):
    """the volume of `shape` from the band table of wavedec3"""
    hlen, taps = bank(wname, dtype)
    levels = (len(bands) - 1) // 7
    shapes = level_shapes(shape, hlen, levels)
    a = np.asarray(bands[0]).astype(dtype)
    for lev in range(levels, 0, -1):
        d = {k: np.asarray(b).astype(dtype) for k, b in zip(BAND_KEYS, bands[1 + 7 * (levels - lev):8 + 7 * (levels - lev)])}
        d["aaa"] = a
        a = idwt3(d, shapes[lev - 1], taps)
    return a


def make_input(shape, dt, kind="uniform"):
    """the inputs of the GPU tests: uniform(-100, 100) with seed 1, impulses on the eight corners, the wrapped ramp"""
    if kind == "uniform":
        return np.random.RandomState(1).uniform(-100, 100, shape).astype(dt)
    if kind == "impulse":
        x = np.zeros(shape, dt)
        vals = (100.0, -50.0, 25.0, -75.0, 60.0, -30.0, 15.0, -90.0)
        for v, (z, y, c) in zip(vals, [(z, y, c) for z in (0, -1) for y in (0, -1) for c in (0, -1)]):
            x[z, y, c] = v
        return x
    assert kind == "ramp"
    zz, yy, xx = np.mgrid[0:shape[0], 0:shape[1], 0:shape[2]]
    return ((3 * xx + 5 * yy + 7 * zz) % 17 - 8.0).astype(dt)
