"""CPU-only: the numpy reference of the batched 1-D DWT with boundary modes (tests/refext1d.py) pinned against independent formulas,
and what the built libraries answer about BoundaryWavelets1D without a device (geometry, clamp, refusals, exported symbols).

Bounds of the GPU tests (tests/test_ext1d_gpu.py): 1e-5 (float32) / 1e-12 (float64) per band, 10x for a round trip.  Here the
reference itself must stay well inside them: float64 round trips below a tenth of the float64 round-trip bound, and its float32
evaluation within a quarter of the float32 bounds on every case and input of the GPU tests."""
import ctypes as C
import functools

import numpy as np
import pytest

import pdwt_amd
from pdwt_amd import _native as nat
from tests import refext as R
from tests import refext1d as R1
from tests.helpers import band_err

RUNS = [(shape, wname, levels, mode) for shape, wname, levels, modes in R1.CASES for mode in modes]
_ids = ["%dx%d-%s-L%d-%s" % (r[0] + r[1:]) for r in RUNS]


@functools.lru_cache(maxsize=None)
def _dec(shape, wname, levels, mode, kind="normal"):
    x = R1.make_input(shape, np.float64, kind)
    return x, R1.wavedec(x, wname, levels, mode, np.float64)


@pytest.mark.parametrize("shape,wname,levels", [(c[0], c[1], c[2]) for c in R1.CASES if c[0][0] <= 300])
def test_mode_zero_is_the_full_convolution_at_the_odd_indices(shape, wname, levels):
    x, bands = _dec(shape, wname, levels, "zero")
    F, taps = R.bank(wname)
    assert [b.shape for b in bands] == [(shape[0], n) for n in R1.band_lens(shape[1], F, levels)]
    for r in range(min(shape[0], 5)):
        a = x[r]
        for l in range(1, levels + 1):
            d = np.convolve(a, taps["H"])[1::2]
            a = np.convolve(a, taps["L"])[1::2]
            assert d.shape == bands[l][r].shape and np.abs(d - bands[l][r]).max() <= 1e-12 * max(1.0, np.abs(d).max()), (r, l)
        assert np.abs(a - bands[0][r]).max() <= 1e-12 * np.abs(a).max()


@pytest.mark.parametrize("mode", R1.MODES)
@pytest.mark.parametrize("shape,wname", [((5, 77), "haar"), ((9, 64), "db2"), ((8, 33), "db4")])
def test_level_1_is_the_row_pass_of_the_2d_reference(shape, wname, mode):
    """dwt2 = rows, then columns: the column pass of the level-1 bands of wavedec gives the four bands of refext.dwt2, bit for bit"""
    x = R1.make_input(shape, np.float64, "ramp") + R1.make_input(shape, np.float64)
    _, taps = R.bank(wname)
    a, d = R1.wavedec(x, wname, 1, mode)
    A, H, V, D = R.dwt2(x, taps, mode)
    cols = lambda b: [np.ascontiguousarray(q.T) for q in R.analysis(np.ascontiguousarray(b.T), taps["L"], taps["H"], mode)]
    for got, want in zip(cols(a) + cols(d), (A, H, V, D)):
        assert np.array_equal(got, want)


@pytest.mark.parametrize("shape,wname,levels,mode", RUNS, ids=_ids)
def test_perfect_reconstruction_and_the_float32_evaluation(shape, wname, levels, mode):
    for kind in ("normal", "ramp"):
        x, bands = _dec(shape, wname, levels, mode, kind)
        assert min(np.abs(b).max() for b in bands) > 1.0  # no band near zero: a plain per-band bound holds
        rt = band_err(R1.waverec(bands, shape[1], wname), x)
        b32 = R1.wavedec(x.astype(np.float32), wname, levels, mode, np.float32)
        ref32 = R1.wavedec(x.astype(np.float32), wname, levels, mode, np.float64)
        e32 = max(band_err(g, r) for g, r in zip(b32, ref32))
        rt32 = band_err(R1.waverec(b32, shape[1], wname, np.float32), x.astype(np.float32))
        print("%s %s L%d %s %s: float64 round trip %.2e, float32 worst band %.2e round trip %.2e" % (shape, wname, levels, mode, kind, rt, e32, rt32))
        assert rt <= 1e-12, rt
        assert e32 <= 0.25 * 1e-5 and rt32 <= 0.25 * 1e-4, (e32, rt32)


# ---- the built libraries, without a device ---------------------------------------------------------------------------------------------
HANDLE_NAMES = ["new", "delete", "forward", "inverse", "get_image", "set_image", "state", "info", "geometry", "mode_index", "fused", "num_bands", "coeff_shape",
                "get_coeff", "set_coeff", "image_int_ptr", "coeff_int_ptr", "soft_threshold", "hard_threshold", "norm1", "band_stats", "all_band_stats",
                "estimate_sigma", "threshold_bands", "denoise"]


def test_new_symbols_are_exported_from_the_three_libraries():
    L = pdwt_amd.hip()
    for n in ("pdwt_num_bands_ext1d", "pdwt_ext1d_band_len", "pdwt_ext1d_fused", "pdwt_ext1d_tmp_elems"):
        assert hasattr(L, n), n
    for n in ("forward_level", "inverse_level", "forward", "inverse"):
        for sfx in ("f32", "f64"):
            assert hasattr(L, "pdwt_ext1d_%s_%s" % (n, sfx)), (n, sfx)
    for dt in (np.float32, np.float64):
        H = nat.host(dt)
        for n in HANDLE_NAMES:
            assert hasattr(H, "pdwt_bw1_" + n), (dt, n)
            assert n in ("fused",) or hasattr(H, "pdwt_bw_" + n), n  # name for name with the 2-D handle API
    assert hasattr(pdwt_amd, "BoundaryWavelets1D")


@pytest.mark.parametrize("shape,wname,levels", [(c[0], c[1], c[2]) for c in R1.CASES])
def test_geometry_of_the_class_and_of_the_c_abi(shape, wname, levels):
    L, H = pdwt_amd.hip(), nat.host(np.float32)
    F, _ = R.bank(wname)
    Nc = shape[1]
    want_levels = R1.clamp_levels(Nc, F, levels)
    n = (C.c_int * 33)()
    assert H.pdwt_bw1_geometry(Nc, F, levels, n) == want_levels
    if want_levels:
        assert want_levels == levels and list(n[:levels + 1]) == R1.level_lens(Nc, F, levels)
    else:
        assert shape == (3, 7)  # the one case below the clamp
    # the C ABI does not clamp: any row of at least hlen - 1 samples
    lens = R1.band_lens(Nc, F, levels)
    assert L.pdwt_num_bands_ext1d(Nc, F, levels) == levels + 1
    assert [L.pdwt_ext1d_band_len(Nc, F, levels, k) for k in range(levels + 1)] == lens
    assert L.pdwt_ext1d_band_len(Nc, F, levels, levels + 1) == -1 and L.pdwt_ext1d_band_len(Nc, F, levels, -1) == -1


def test_clamp_and_refusals_without_a_device():
    L, H = pdwt_amd.hip(), nat.host(np.float64)
    n = (C.c_int * 33)()
    assert H.pdwt_bw1_geometry(4099, 8, 40, n) == 9 == R1.clamp_levels(4099, 8, 40)   # ilog2(4099 / 7) = 9
    assert H.pdwt_bw1_geometry(64, 4, 0, n) == 1                                       # levels < 1 asks for 1
    assert H.pdwt_bw1_geometry(7, 8, 1, n) == 0 and H.pdwt_bw1_geometry(6, 8, 1, None) == 0  # a clamp to 0 levels
    assert H.pdwt_bw1_geometry(64, 3, 1, n) == 0 and H.pdwt_bw1_geometry(64, 42, 1, n) == 0 and H.pdwt_bw1_geometry(0, 4, 1, n) == 0
    assert H.pdwt_bw1_geometry(1 << 30, 2, 99, None) == 30
    assert H.pdwt_bw1_mode_index(b"symmetric") == 2 and H.pdwt_bw1_mode_index(b"smooth") == -1
    # sizes the entries refuse
    assert L.pdwt_num_bands_ext1d(7, 8, 1) == 2 and L.pdwt_num_bands_ext1d(6, 8, 1) == -1
    assert L.pdwt_num_bands_ext1d(64, 4, 0) == -1 and L.pdwt_num_bands_ext1d(64, 4, 33) == -1 and L.pdwt_num_bands_ext1d(64, 5, 1) == -1
    assert L.pdwt_ext1d_band_len(6, 8, 1, 0) == -1 and L.pdwt_ext1d_band_len(64, 42, 1, 0) == -1
    # the one-launch rule needs no device either: a row of 4099 samples fits, one of 40037 cannot in either precision
    for es in (4, 8):
        assert L.pdwt_ext1d_fused(4099, 8, 5, es) == 1 and L.pdwt_ext1d_fused(40037, 8, 3, es) == 0
        assert L.pdwt_ext1d_tmp_elems(2, 4099, 8, 5, es) == 0 and L.pdwt_ext1d_tmp_elems(2, 40037, 8, 3, es) == 2 * 2 * ((40037 + 7) // 2)
        assert L.pdwt_ext1d_tmp_elems(2, 40037, 8, 1, es) == 0
    assert L.pdwt_ext1d_fused(64, 4, 1, 2) == -1
    # mode 5, 0 levels and NULL pointers are refused before anything touches a device (the pointers are never dereferenced)
    for sfx, FT in (("f32", nat.Filters32), ("f64", nat.Filters64)):
        f = FT()
        assert getattr(L, "pdwt_compute_filters_separable_" + sfx)(b"db2", 0, C.byref(f)) == 4
        f.hlen = 4
        fake = C.c_void_p(4096)
        tab = (C.c_void_p * 2)(4096, 4096)
        assert getattr(L, "pdwt_ext1d_forward_level_" + sfx)(fake, fake, fake, 4, 64, 5, C.byref(f)) == -1
        assert getattr(L, "pdwt_ext1d_forward_level_" + sfx)(fake, fake, fake, 4, 64, -1, C.byref(f)) == -1
        assert getattr(L, "pdwt_ext1d_forward_level_" + sfx)(fake, fake, fake, 4, 2, 2, C.byref(f)) == -1
        assert getattr(L, "pdwt_ext1d_inverse_level_" + sfx)(fake, None, fake, 4, 64, C.byref(f)) == -1
        assert getattr(L, "pdwt_ext1d_forward_" + sfx)(fake, tab, 4, 64, 1, 5, C.byref(f), None) == -1
        assert getattr(L, "pdwt_ext1d_forward_" + sfx)(fake, tab, 4, 64, 0, 2, C.byref(f), None) == -1
        assert getattr(L, "pdwt_ext1d_inverse_" + sfx)(fake, tab, 4, 64, 0, C.byref(f), None) == -1
        assert getattr(L, "pdwt_ext1d_inverse_" + sfx)(fake, None, 4, 64, 1, C.byref(f), None) == -1
