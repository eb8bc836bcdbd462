"""Reference of the ADJOINTS of the 3-D transform with signal-extension boundary modes, in numpy (float64 for the reference proper; float32
to measure what float32 arithmetic of the kernels' order can reach).  The forward maps are those of tests/refext3d.py and the one-axis
adjoints those of tests/refadj.py; this module imports both and alters neither.

One level: the forward runs x, y, then z, so its adjoint runs z first -- `refadj.analysis_adjoint` along axis 0 on the pairs
("a" + k, "d" + k), k in aa, ad, da, dd (the fold along z included) -- and then the 2-D level adjoint `refadj.dwt2_adjoint` on every plane
with A, H, V, D = the quadrants aa, da, ad, dd (H is y-high / x-low: refext.dwt2).  This is the kernels' order.  The adjoint of the inverse
is `refext3d.dwt3` in mode zero with the reversed synthesis bank.  Several levels: from the coarsest to the finest, the xbar of a level is
the aaa cotangent of the next finer one; the band table is that of refext3d.wavedec3, [A_L, level L ... level 1].

Bounds of the GPU tests (tests/test_adjoint3d_gpu.py): the family's 1e-5 (float32) / 1e-12 (float64) of max|ref| holds for a case whose
float32 figure in this order is at most a quarter of it (tests/test_refadj3d_cpu.py measures every case); a case above the quarter would
get four times its figure in F32_BOUND_OF below.  None does: the figures are 1.1e-7 .. 3.7e-7 (the module docstring of the CPU test).
"""
import numpy as np

from tests import refadj as A
from tests import refext3d as R3

MODES = R3.MODES
QUADS = ("aa", "ad", "da", "dd")  # (y, x) letters of the four x-y quadrants

# the GPU cases: those of the forward tests plus a periodic run of the three-chunk shape (halo targets in the first and the last z chunk,
# none in the middle one) and the `constant` mode of the 40-tap bank (one sample has up to 39 pre-images per axis)
CASES = list(R3.CASES) + [((40, 24, 24), "db2", 2, ("periodic",)), ((40, 48, 40), "db20", 1, ("constant",))]
F32_BOUND = 1e-5
F32_BOUND_OF = {}  # (shape, bank, levels, mode) -> a bound of its own: four times the float32 figure of the reference's order (none needed)


def _z_adjoint(lo, hi, taps, nz, mode):
    """analysis_adjoint along axis 0"""
    out = A.analysis_adjoint(np.ascontiguousarray(np.moveaxis(lo, 0, -1)), np.ascontiguousarray(np.moveaxis(hi, 0, -1)), taps["L"], taps["H"], nz, mode)
    return np.ascontiguousarray(np.moveaxis(out, -1, 0))


def dwt3_adjoint(bands_by_key, shape, taps, mode):
    """xbar of `shape` = (nz, nr, nc) from the eight cotangent bands by key: the z adjoint (fold included), then the x-y adjoint per plane"""
    q = {k: _z_adjoint(bands_by_key["a" + k], bands_by_key["d" + k], taps, shape[0], mode) for k in QUADS}
    return A.dwt2_adjoint([q["aa"], q["da"], q["ad"], q["dd"]], shape[1:], taps, mode)


def idwt3_adjoint(xbar, taps):
    """{key: cotangent band}: the adjoint of refext3d.idwt3"""
    z = {"L": np.ascontiguousarray(taps["IL"][::-1]), "H": np.ascontiguousarray(taps["IH"][::-1])}
    return R3.dwt3(xbar, z, "zero")


def wavedec3_adjoint(bands, shape, wname, mode, dtype=np.float64):
    """xbar of `shape` from the cotangents of refext3d.wavedec3's table"""
    hlen, taps = R3.bank(wname, dtype)
    levels = (len(bands) - 1) // 7
    shapes = R3.level_shapes(shape, hlen, levels)
    a = np.asarray(bands[0]).astype(dtype)
    for lev in range(levels, 0, -1):
        d = {k: np.asarray(b).astype(dtype) for k, b in zip(R3.BAND_KEYS, bands[1 + 7 * (levels - lev):8 + 7 * (levels - lev)])}
        d["aaa"] = a
        a = dwt3_adjoint(d, shapes[lev - 1], taps, mode)
    return a


def waverec3_adjoint(xbar, wname, levels, dtype=np.float64):
    """the cotangent table [A_L, level L ... level 1] of refext3d.waverec3 from xbar"""
    _, taps = R3.bank(wname, dtype)
    a = np.asarray(xbar).astype(dtype)
    per_level = []
    for _ in range(levels):
        b = idwt3_adjoint(a, taps)
        per_level.append([b[k] for k in R3.BAND_KEYS])
        a = b["aaa"]
    out = [a]
    for lev in range(levels, 0, -1):
        out += per_level[lev - 1]
    return out


def bound(sfx, shape, wname, levels, mode):
    if sfx == "f64":
        return 1e-12
    return F32_BOUND_OF.get((tuple(shape), wname, levels, mode), F32_BOUND)
