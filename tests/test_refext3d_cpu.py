"""CPU-only: pins tests/refext3d.py, the float64 reference of the boundary-mode volume tests (tests/test_ext3d_gpu.py).

  * Haar on an even-sized volume touches no extension: it equals the periodised reference tests/ref3d.dwt3_forward, whatever the mode;
  * one level of db3 on 11 x 5 x 6 equals np.pad (by F - 1 per side) along each axis followed by np.convolve and the samples 2i + F, with
    numpy's own pad modes standing for the five modes (bands aaa, dda, ddd): an independent statement of the index map and of the axis
    and key order;
  * every GPU case round-trips in float64 to a fifth of the GPU round-trip bound or better, so no bank needs a looser one;
  * the float32 evaluation of the reference stays within a quarter of the float32 forward bound on every input of the GPU tests;
  * the band shapes are (n + F - 1) // 2 per axis and level, in the band order of Wavelets3D.
"""
import numpy as np
import pytest

from tests import ref3d
from tests import refext3d as R3
from tests.helpers import band_err

FWD = {np.dtype(np.float32): 1e-5, np.dtype(np.float64): 1e-12}  # the bounds of tests/test_ext3d_gpu.py
RT = {k: 10 * v for k, v in FWD.items()}
NP_PAD = {"zero": "constant", "constant": "edge", "symmetric": "symmetric", "reflect": "reflect", "periodic": "wrap"}
_ids = ["%dx%dx%d-%s" % (c[0] + (c[1],)) for c in R3.CASES]


def test_haar_on_an_even_sized_volume_is_the_periodised_reference():
    x = R3.make_input((8, 12, 16), np.float64)
    want = ref3d.dwt3_forward(x, "haar", 2)
    for mode in R3.MODES:
        got = R3.wavedec3(x, "haar", 2, mode)
        assert len(got) == len(want) == 15
        assert all(g.shape == w.shape for g, w in zip(got, want))
        worst = max(band_err(g, w) for g, w in zip(got, want))
        print("haar 8x12x16 L2 %s: largest band error %.3e" % (mode, worst))
        assert worst <= 1e-14, (mode, worst)  # (measured: exactly 0; the same two-term sums in the same order)


def _conv_axis(x, axis, f, mode):
    F = len(f)
    n = x.shape[axis]
    N = (n + F - 1) // 2
    pad = [(0, 0)] * x.ndim
    pad[axis] = (F - 1, F - 1)
    p = np.pad(x, pad, mode=NP_PAD[mode])
    full = np.apply_along_axis(lambda v: np.convolve(v, f), axis, p)
    return np.take(full, 2 * np.arange(N) + F, axis=axis)


@pytest.mark.parametrize("mode", R3.MODES)
def test_one_level_against_pad_and_convolve(mode):
    shape, wname = (11, 5, 6), "db3"
    F, taps = R3.bank(wname)
    x = R3.make_input(shape, np.float64)
    got = R3.dwt3(x, taps, mode)
    assert set(got) == set(R3.LEVEL_KEYS)
    for key in ("aaa", "dda", "ddd"):
        b = x
        for axis, letter in ((2, key[2]), (1, key[1]), (0, key[0])):
            b = _conv_axis(b, axis, taps["L"] if letter == "a" else taps["H"], mode)
        e = band_err(got[key], b)
        print("db3 11x5x6 %s %s: %.3e" % (mode, key, e))
        assert got[key].shape == (8, 5, 5) and e <= 1e-13, (mode, key, e)  # (measured: 0 to 1.2e-15; sums of 6 terms)


@pytest.mark.parametrize("case", R3.CASES, ids=_ids)
def test_reference_round_trip_and_band_shapes(case):
    """Measured (float64, uniform(-100, 100)): sym8 1.4e-12 (the table's sym taps reconstruct only to about 1e-12), every other case at
    most 1.6e-15.  The GPU round-trip bound 1e-11 is kept for every bank: the reference alone stays at or below a fifth of it."""
    shape, wname, levels, modes = case
    F, _ = R3.bank(wname)
    x = R3.make_input(shape, np.float64)
    shapes = R3.level_shapes(shape, F, levels)
    for l in range(1, levels + 1):
        assert shapes[l] == tuple((n + F - 1) // 2 for n in shapes[l - 1])
    for mode in modes:
        bands = R3.wavedec3(x, wname, levels, mode)
        assert [b.shape for b in bands] == R3.band_shapes(shape, F, levels) and len(bands) == 7 * levels + 1
        assert bands[0].shape == shapes[levels] and all(b.shape == shapes[1] for b in bands[-7:])
        e = band_err(R3.waverec3(bands, shape, wname), x)
        print("reference round trip %s %s L%d %s: %.3e" % (shape, wname, levels, mode, e))
        assert e <= RT[np.dtype(np.float64)] / 5, (mode, e)
    # the two shapes below the clamp of the class run through the level drivers
    assert R3.clamp_levels(shape, F, levels) == (0 if shape in R3.DRIVER_CASES else levels)


@pytest.mark.parametrize("case", R3.CASES, ids=_ids)
def test_float32_evaluation_is_within_a_quarter_of_the_bound(case):
    """Measured over the three inputs of the GPU tests: at most 6.7e-7 (db20), a quarter of the bound being 2.5e-6."""
    shape, wname, levels, modes = case
    worst = 0.0
    for kind in ("uniform", "impulse", "ramp"):
        x = R3.make_input(shape, np.float32, kind)
        for mode in modes:
            ref = R3.wavedec3(x, wname, levels, mode, np.float64)
            got = R3.wavedec3(x, wname, levels, mode, np.float32)
            assert all(g.dtype == np.float32 for g in got)
            for k, (g, r) in enumerate(zip(got, ref)):
                e = band_err(g, r)
                worst = max(worst, e)
                assert e <= FWD[np.dtype(np.float32)] / 4, (kind, mode, k, e)
    print("%s %s: worst float32 band error of the reference %.3e" % (shape, wname, worst))
