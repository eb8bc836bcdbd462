"""Reference of the batched 1-D DWT with signal-extension boundary modes (BoundaryWavelets1D) for the tests: loops over the one-level
formulas of tests/refext.py (analysis / synthesis along the LAST axis) with the band order of Wavelets(ndim=1),
[A_L, D_1, ..., D_L], level 1 the finest.  An (Nr, Nc) array is Nr independent rows.  Nothing here touches pdwt_amd.
"""
import numpy as np

from oracle import oracle as orc
from tests import refext as R

MODES = R.MODES
MAX_LEVELS = R.MAX_LEVELS

# the cases of the GPU tests (tests/test_ext1d_gpu.py), shared with the CPU checks of this reference: ((Nr, Nc), bank, levels, modes)
ALL = MODES
CASES = [
    ((3, 7), "db4", 1, ALL),                              # halo of n - 1 samples (below the level clamp of the class: level drivers)
    ((4, 64), "db2", 3, ALL),                             # multi-level, even
    ((5, 77), "haar", 3, ALL),                            # odd lengths: the mode-dependent last sample
    ((3, 200), "db5", 3, ("symmetric", "reflect")),
    ((2, 1000), "sym8", 4, ("symmetric", "zero")),
    ((300, 33), "db2", 2, ("symmetric", "periodic")),     # many short rows: full packs and a partial last pack
    ((2, 4099), "db4", 5, ("symmetric", "constant")),     # odd long row, one launch
    ((3, 48), "bior2.2", 2, ("symmetric",)),
    ((3, 72), "coif1", 2, ("symmetric",)),
    ((2, 96), "db20", 1, ("symmetric", "periodic")),      # 40 taps
    ((2, 40037), "db4", 3, ("symmetric", "zero")),        # above any LDS budget: interior and border tiles of the per-level kernels
    ((70001, 16), "db2", 1, ("symmetric",)),              # more rows than a grid.y holds
]
FUSED_CASES = [(4, 64), (5, 77), (300, 33), (2, 4099), (2, 96)]  # where the two kernel forms are compared bit for bit


def clamp_levels(Nc, hlen, levels):
    """ilog2(Nc / (hlen - 1)) as in Wavelets(ndim=1) (PyWavelets' dwt_max_level), at most MAX_LEVELS; at least one level is asked for"""
    return max(0, min(max(int(levels), 1), orc.ilog2(Nc // (hlen - 1)), MAX_LEVELS))


def level_lens(Nc, hlen, levels):
    """[n_l for l = 0 .. levels]: the samples of a row, then the coefficients per row of each level"""
    out = [int(Nc)]
    for _ in range(levels):
        out.append((out[-1] + hlen - 1) // 2)
    return out


def band_lens(Nc, hlen, levels):
    """coefficients per row of [A_L, D_1, ..., D_L]"""
    n = level_lens(Nc, hlen, levels)
    return [n[levels]] + n[1:]


def wavedec(x, wname, levels, mode, dtype=np.float64):
    """[A_L, D_1, ..., D_L] of exactly `levels` levels (not clamped) along the last axis, computed in `dtype`"""
    _, taps = R.bank(wname, dtype)
    a = np.asarray(x).astype(dtype)
    det = []
    for _ in range(levels):
        a, d = R.analysis(a, taps["L"], taps["H"], mode)
        det.append(d)
    return [a] + det


def waverec(bands, n, wname, dtype=np.float64):
    """the rows of n samples from the band table of wavedec"""
    hlen, taps = R.bank(wname, dtype)
    levels = len(bands) - 1
    lens = level_lens(n, hlen, levels)
    a = np.asarray(bands[0]).astype(dtype)
    for l in range(levels, 0, -1):
        a = R.synthesis(a, np.asarray(bands[l]).astype(dtype), taps["IL"], taps["IH"], lens[l - 1])
    return a


def make_input(shape, dtype, kind="normal"):
    """the two inputs of the tests: seeded standard_normal, and the wrapped ramp ((3c + 5r) mod 17) - 8"""
    if kind == "normal":
        return np.random.RandomState(1).standard_normal(shape).astype(dtype)
    assert kind == "ramp"
    rr, cc = np.mgrid[0:shape[0], 0:shape[1]]
    return ((3 * cc + 5 * rr) % 17 - 8.0).astype(dtype)
