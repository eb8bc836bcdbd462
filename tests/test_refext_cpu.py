"""CPU-only: pins tests/refext.py (the reference of the boundary-mode GPU tests) and the host geometry of BoundaryWavelets.

  * `zero` equals np.convolve(x, L)[1::2] on lines of odd and even length;
  * `periodic` on even sizes, banks with F/2 odd: the coefficients from the offset (F/2 - 1)/2 equal the oracle's one-level
    periodised transform (all four bands: this also pins the orientation of H and V);
  * `symmetric` Haar on an even-sized image equals the oracle's Haar level (no extension is touched);
  * perfect reconstruction of every mode over 1-3 levels on odd and even sizes, n = F - 1 included, and the reference's own round-trip
    error per bank of the GPU cases (it decides which banks keep the 10x round-trip bound there);
  * the float32 evaluation of the reference stays within a quarter of the float32 bar of its float64 evaluation on the GPU cases;
  * pdwt_bw_geometry and pdwt_ext_band_shape of the built libraries (no GPU needed) give the reference's shapes on all the cases; a clamp
    to 0 levels and mode 5 are refused.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import oracle as orc
from tests import refext as R
from tests.helpers import band_err

FWD = {np.dtype(np.float32): 1e-5, np.dtype(np.float64): 1e-12}  # the bounds of tests/test_ext2d_gpu.py
RT = {k: 10 * v for k, v in FWD.items()}
BANKS = sorted({c[1] for c in R.CASES})


def _img(shape, dt=np.float64):
    return np.random.RandomState(1).uniform(-100, 100, shape).astype(dt)


# ---- the formulas on lines -------------------------------------------------------------------------------
@pytest.mark.parametrize("wname", ["haar", "db2", "db3", "sym8"])
@pytest.mark.parametrize("n", [16, 17, 33])
def test_zero_is_the_full_convolution_at_odd_indices(wname, n):
    F, t = R.bank(wname)
    if n < F - 1:
        pytest.skip("line shorter than the bank")
    x = _img((3, n))
    a, d = R.analysis(x, t["L"], t["H"], "zero")
    assert a.shape == (3, (n + F - 1) // 2)
    for r in range(3):
        assert np.allclose(a[r], np.convolve(x[r], t["L"])[1::2], rtol=0, atol=1e-12)
        assert np.allclose(d[r], np.convolve(x[r], t["H"])[1::2], rtol=0, atol=1e-12)


def test_the_index_map():
    n = 5
    j = np.arange(-7, 13)
    assert list(R.ext_index(j, n, "constant")[0]) == [0] * 7 + [0, 1, 2, 3, 4] + [4] * 8
    assert list(R.ext_index(j, n, "periodic")[0]) == [3, 4, 0, 1, 2, 3, 4, 0, 1, 2, 3, 4, 0, 1, 2, 3, 4, 0, 1, 2]
    # ... x1 x0 | x0 x1 ... x4 | x4 x3 ...   and   ... x2 x1 | x0 x1 ... x4 | x3 x2 ...
    assert list(R.ext_index(np.arange(-3, 8), n, "symmetric")[0]) == [2, 1, 0, 0, 1, 2, 3, 4, 4, 3, 2]
    assert list(R.ext_index(np.arange(-3, 8), n, "reflect")[0]) == [3, 2, 1, 0, 1, 2, 3, 4, 3, 2, 1]
    assert list(R.ext_index(np.arange(-2, 3), 1, "reflect")[0]) == [0] * 5  # one sample: the constant
    idx, ok = R.ext_index(np.arange(-2, 7), n, "zero")
    assert list(ok) == [False, False, True, True, True, True, True, False, False]
    for mode in R.MODES:  # inside the line every mode is the identity
        idx, ok = R.ext_index(np.arange(n), n, mode)
        assert list(idx) == list(range(n)) and ok.all()


@pytest.mark.parametrize("wname", ["haar", "db3", "db5", "db7", "coif1"])
@pytest.mark.parametrize("shape", [(32, 48), (64, 64)])
def test_periodic_against_the_oracle_periodisation(wname, shape):
    F, _ = R.bank(wname)
    assert (F // 2) % 2 == 1
    off = (F // 2 - 1) // 2
    x = _img(shape)
    O = orc.OracleWavelets(x, wname, 1)
    O.forward()
    got = R.wavedec2(x, wname, 1, "periodic")
    hr, hc = shape[0] // 2, shape[1] // 2
    for q, name in enumerate("AHVD"):
        e = band_err(got[q][off:off + hr, off:off + hc], O.coeffs[q])
        assert e <= 1e-13, (name, e)


@pytest.mark.parametrize("shape", [(32, 48), (16, 20)])
def test_symmetric_haar_on_even_sizes_is_the_oracle_haar_level(shape):
    x = _img(shape)
    O = orc.OracleWavelets(x, "haar", 1)
    O.forward()
    for mode in R.MODES:  # even sizes: no extension is touched, whatever the mode
        got = R.wavedec2(x, "haar", 1, mode)
        for q in range(4):
            assert got[q].shape == O.coeffs[q].shape and band_err(got[q], O.coeffs[q]) <= 1e-14, (mode, q)


# ---- perfect reconstruction ------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("wname", ["haar", "db2", "db3"])
def test_perfect_reconstruction_on_lines_and_small_images(wname, mode):
    F, t = R.bank(wname)
    for n in (max(F - 1, 1), F, F + 1, 16, 17, 33):
        x = _img((2, n))
        a, d = R.analysis(x, t["L"], t["H"], mode)
        assert band_err(R.synthesis(a, d, t["IL"], t["IH"], n), x) <= 1e-13, n
    for shape in ((max(F - 1, 1), F + 1), (16, 17), (33, 20)):
        for levels in (1, 2, 3):
            x = _img(shape)
            bands = R.wavedec2(x, wname, levels, mode)
            assert [b.shape for b in bands] == R.band_shapes(shape, F, levels)
            assert band_err(R.waverec2(bands, shape, wname), x) <= 1e-12, (shape, levels)


@functools.lru_cache(maxsize=None)
def reference_round_trip(wname):
    """the largest float64 round-trip error of the reference alone over the GPU cases of a bank"""
    worst = 0.0
    for shape, w, levels, modes in R.CASES:
        if w != wname:
            continue
        x = _img(shape)
        for mode in modes:
            worst = max(worst, band_err(R.waverec2(R.wavedec2(x, w, levels, mode), shape, w), x))
    return worst


@pytest.mark.parametrize("wname", BANKS)
def test_reference_round_trip_per_bank(wname):
    """Measured (float64, uniform(-100, 100), the GPU cases): bior2.2 6.4e-16, coif1 7.1e-16, db2 8.5e-16, db20 1.1e-15, db4 5.7e-16,
    haar 1.0e-15, sym8 8.7e-13 (the table's sym taps reconstruct only to about 1e-12).  The GPU round-trip bound 1e-11 may
    be kept for a bank whose figure here stays below a tenth of it (1e-12): every bank of the cases does, so no bank has a looser one."""
    e = reference_round_trip(wname)
    print("reference round trip %s: %.3e" % (wname, e))
    assert e <= 0.1 * RT[np.dtype(np.float64)], e


# ---- float32 arithmetic of this order reaches the float32 bar -------------------------------------------------------
@pytest.mark.parametrize("case", R.CASES, ids=["%dx%d-%s" % (c[0] + (c[1],)) for c in R.CASES])
def test_float32_evaluation_is_within_a_quarter_of_the_bar(case):
    shape, wname, levels, modes = case
    x = _img(shape, np.float32)
    worst = 0.0
    for mode in modes:
        ref = R.wavedec2(x, wname, levels, mode, np.float64)
        got = R.wavedec2(x, wname, levels, mode, np.float32)
        assert all(g.dtype == np.float32 for g in got)
        for k, (g, r) in enumerate(zip(got, ref)):
            e = band_err(g, r)
            worst = max(worst, e / (FWD[np.dtype(np.float32)] / 4))
            assert e <= FWD[np.dtype(np.float32)] / 4, (mode, k, e)
        e = band_err(R.waverec2(got, shape, wname, np.float32), x)
        worst = max(worst, e / (RT[np.dtype(np.float32)] / 4))
        assert e <= RT[np.dtype(np.float32)] / 4, (mode, "round trip", e)
    print("%s %s: worst ratio to a quarter of the bar %.3f" % (shape, wname, worst))


# ---- the host geometry of the built libraries (no GPU) -------------------------------------------------------------------
def _host():
    from pdwt_amd import _native as N
    return N, N.hip(), N.host(np.float32), N.host(np.float64)


@pytest.mark.parametrize("case", R.CASES, ids=["%dx%d-%s" % (c[0] + (c[1],)) for c in R.CASES])
def test_library_geometry_equals_the_reference(case):
    shape, wname, levels, _ = case
    N, hip, h32, h64 = _host()
    F, _ = R.bank(wname)
    want = R.band_shapes(shape, F, levels)
    assert hip.pdwt_num_bands_ext(shape[0], shape[1], F, levels) == len(want) == 3 * levels + 1
    for k, (r, c) in enumerate(want):
        br, bc = C.c_int(), C.c_int()
        assert hip.pdwt_ext_band_shape(shape[0], shape[1], F, levels, k, C.byref(br), C.byref(bc)) == r * c
        assert (br.value, bc.value) == (r, c), k
    assert hip.pdwt_ext_band_shape(shape[0], shape[1], F, levels, len(want), None, None) == -1
    clamped = R.clamp_levels(shape, F, levels)
    for L in (h32, h64):
        nr, nc = (C.c_int * 33)(), (C.c_int * 33)()
        assert L.pdwt_bw_geometry(shape[0], shape[1], F, levels, nr, nc) == clamped
        assert [(nr[l], nc[l]) for l in range(clamped + 1)] == R.level_shapes(shape, F, clamped)
    if shape == (7, 7):
        assert clamped == 0  # ilog2(7 / 7): one level of db4 on 7 x 7 is below the clamp of the class (the level drivers take it)
    else:
        assert clamped == levels


def test_geometry_clamps_and_refusals():
    N, hip, h32, h64 = _host()
    assert h32.pdwt_bw_geometry(96, 80, 8, 9, None, None) == 3       # ilog2(80 / 7)
    assert h32.pdwt_bw_geometry(64, 64, 4, 0, None, None) == 1       # levels < 1 asks for 1
    assert h32.pdwt_bw_geometry(6, 64, 8, 2, None, None) == 0        # too small for one level
    assert h32.pdwt_bw_geometry(64, 64, 7, 2, None, None) == 0 and h32.pdwt_bw_geometry(64, 64, 42, 1, None, None) == 0
    assert h32.pdwt_bw_geometry(1 << 16, 1 << 15, 2, 40, None, None) == 0  # Nr * Nc >= 2^31
    assert h64.pdwt_bw_geometry(1 << 15, 1 << 15, 2, 40, None, None) == 15
    assert hip.pdwt_num_bands_ext(6, 64, 8, 1) == -1 and hip.pdwt_num_bands_ext(7, 64, 8, 1) == 4   # a line below F - 1
    assert hip.pdwt_num_bands_ext(64, 64, 4, 33) == -1 and hip.pdwt_num_bands_ext(64, 64, 4, 0) == -1
    assert [h32.pdwt_bw_mode_index(m.encode()) for m in R.MODES] == [0, 1, 2, 3, 4]
    assert h32.pdwt_bw_mode_index(b"smooth") == -1 and h32.pdwt_bw_mode_index(b"periodization") == -1


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_a_clamp_to_zero_levels_and_mode_five_are_refused(dt):
    """Both refusals come before anything touches a device: W_CREATION_ERROR from the constructor, PDWT_EINVAL from the level driver."""
    from pdwt_amd.wavelets import W_CREATION_ERROR
    N, hip, h32, h64 = _host()
    L = h32 if dt == np.float32 else h64
    try:
        for args in ((6, 64, b"db4", 2, 2), (64, 64, b"db2", 1, 5), (64, 64, b"db2", 1, -1), (64, 64, b"nosuchwavelet", 1, 2)):
            h = L.pdwt_bw_new(None, args[0], args[1], args[2], args[3], args[4], 1)
            assert h and L.pdwt_bw_state(h) == W_CREATION_ERROR, args
            assert L.pdwt_bw_num_bands(h) == 0 and L.pdwt_bw_coeff_shape(h, 0, None, None) == 0
            L.pdwt_bw_forward(h)
            L.pdwt_bw_inverse(h)
            assert L.pdwt_bw_state(h) == W_CREATION_ERROR
            L.pdwt_bw_delete(h)
    finally:
        C.CDLL(None).fflush(None)  # the class reports on the C stdout: leave nothing in its buffer for a later test's capture
    sfx = "f32" if dt == np.float32 else "f64"
    f = (N.Filters32 if dt == np.float32 else N.Filters64)()
    assert getattr(hip, "pdwt_compute_filters_separable_" + sfx)(b"db4", 0, C.byref(f)) == 8
    f.hlen = 8
    buf = np.zeros(64, dt)  # host memory: a refused call dereferences nothing
    p = buf.ctypes.data
    fwd, inv = getattr(hip, "pdwt_ext2d_forward_level_" + sfx), getattr(hip, "pdwt_ext2d_inverse_level_" + sfx)
    assert fwd(p, p, p, p, p, 61, 67, 5, C.byref(f)) == -1 and fwd(p, p, p, p, p, 61, 67, -1, C.byref(f)) == -1
    assert fwd(p, p, p, p, p, 6, 67, 2, C.byref(f)) == -1 and fwd(p, p, p, p, p, 61, 6, 2, C.byref(f)) == -1
    assert inv(p, p, p, p, p, 6, 67, C.byref(f)) == -1 and inv(p, p, p, p, None, 61, 67, C.byref(f)) == -1
    f.hlen = 7
    assert fwd(p, p, p, p, p, 61, 67, 2, C.byref(f)) == -1
