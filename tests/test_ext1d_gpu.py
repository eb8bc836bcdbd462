"""BoundaryWavelets1D (the batched 1-D DWT with signal-extension boundary modes, all levels in one launch where a row fits LDS) on the
GPU against tests/refext1d.py, the float64 numpy reference (pinned on the CPU in tests/test_refext1d_cpu.py).

Metric: tests/helpers.band_err per band (max |got - ref| / max |ref| of that band).  Bounds, those of tests/test_ext2d_gpu.py: 1e-5
(float32) and 1e-12 (float64) for every band of a forward and for an inverse alone; 10x those for a round trip.  The reference alone
round-trips every case to below 4e-13 and its float32 evaluation stays below 3e-7 per band (tests/test_refext1d_cpu.py): under a tenth of
each bound.  No band of any case is near zero (every band maximum is above 1), so a plain per-band bound holds.

Inputs: seeded standard_normal, and the wrapped ramp ((3c + 5r) mod 17) - 8 (where symmetric, reflect and constant differ at both ends
of every row, with detail bands that are not small).

The 3 x 7 db4 case lies below the level clamp of the class (ilog2(7 / 7) = 0 levels: W_CREATION_ERROR), so it runs through the level
drivers, which take any row of at least hlen - 1 samples.  The two kernel forms (one launch for all levels / one launch per level) must
agree bit for bit; (2, 4099) must take the one-launch path and (2, 40037) cannot.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import pdwt_amd
from pdwt_amd import BoundaryWavelets1D, DeviceArray, Wavelets
from pdwt_amd import _native as nat
from pdwt_amd.wavelets import W_CREATION_ERROR, W_FORWARD, W_INIT, W_INVERSE
from tests import refext as R
from tests import refext1d as R1
from tests.helpers import band_err
from tests.refstats import MAD_SCALE, ref_betas, ref_stats, ref_threshold

pytestmark = pytest.mark.gpu

FWD = {np.dtype(np.float32): 1e-5, np.dtype(np.float64): 1e-12}
RT = {k: 10 * v for k, v in FWD.items()}
SUM_TOL = 1e-10  # sums accumulated in double (tests/test_ext2d_gpu.py)
DTYPES = [np.float32, np.float64]
RUNS = [(shape, wname, levels, mode) for shape, wname, levels, modes in R1.CASES for mode in modes]
CLASS_RUNS = [r for r in RUNS if r[0] != (3, 7)]
FUSED_RUNS = [r for r in RUNS if r[0] in R1.FUSED_CASES]


def _id(r):
    return "%dx%d-%s-L%d-%s" % (r[0] + r[1:])


@functools.lru_cache(maxsize=None)
def _ref(shape, wname, levels, mode, dtname, kind="normal"):
    """(batch in the dtype under test, float64 reference bands of it): computed once per case and shared; callers do not modify them"""
    x = R1.make_input(shape, np.dtype(dtname), kind)
    bands = R1.wavedec(x, wname, levels, mode, np.float64)
    for b in bands:
        b.setflags(write=False)
    x.setflags(write=False)
    return x, bands


def _check_bands(got, ref, bound, what):
    assert len(got) == len(ref), (what, len(got), len(ref))
    errs = []
    for k, (g, r) in enumerate(zip(got, ref)):
        assert g.shape == r.shape, (what, k, g.shape, r.shape)
        errs.append(band_err(g, r))
    print("%s: A%d %.3e" % (what, len(ref) - 1, errs[0]) + "".join(" | D%d %.3e" % (l, errs[l]) for l in range(1, len(ref))))
    for k, e in enumerate(errs):
        assert e <= bound, (what, "band", k, e)
    return max(errs)


def _raw_bands(W):
    """every band read straight from device memory, whatever the state"""
    W.sync()
    return [DeviceArray(W, W.coeff_int_ptr(k), W.coeff_shape(k), W.dtype).numpy() for k in range(W.nbands)]


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


class _Dev:
    """a few device buffers of the library's allocator, freed on exit"""

    def __init__(self):
        self.L, self.ptrs = pdwt_amd.hip(), []

    def __enter__(self):
        return self

    def put(self, arr):
        a = np.ascontiguousarray(arr)
        p = self.L.pdwt_malloc(a.nbytes)
        assert p
        self.ptrs.append(p)
        assert self.L.pdwt_memcpy_h2d(p, a.ctypes.data, a.nbytes) == 0
        return p

    def get(self, p, shape, dt):
        out = np.empty(shape, dt)
        assert self.L.pdwt_sync() == 0 and self.L.pdwt_memcpy_d2h(out.ctypes.data, p, out.nbytes) == 0
        return out

    def __exit__(self, *exc):
        self.L.pdwt_sync()
        for p in self.ptrs:
            self.L.pdwt_free(p)
        return False


def _bank(wname, dt):
    L = pdwt_amd.hip()
    sfx = "f32" if np.dtype(dt) == np.float32 else "f64"
    f = (nat.Filters32 if sfx == "f32" else nat.Filters64)()
    h = getattr(L, "pdwt_compute_filters_separable_" + sfx)(wname.encode(), 0, C.byref(f))
    assert h > 0
    f.hlen = h
    return L, sfx, f, h


def _chain_forward(D, x, wname, levels, mode, dt):
    """[A_L, D_1, ..., D_L] by chaining pdwt_ext1d_forward_level_* by hand"""
    L, sfx, f, h = _bank(wname, dt)
    nr, n = x.shape
    src, det = D.put(x), []
    for _ in range(levels):
        N = (n + h - 1) // 2
        a, d = D.put(np.full((nr, N), np.nan, dt)), D.put(np.full((nr, N), np.nan, dt))
        assert getattr(L, "pdwt_ext1d_forward_level_" + sfx)(src, a, d, nr, n, R1.MODES.index(mode), C.byref(f)) == 0
        det.append(D.get(d, (nr, N), dt))
        src, n = a, N
    return [D.get(src, (nr, n), dt)] + det


def _chain_inverse(D, bands, n0, wname, dt):
    L, sfx, f, h = _bank(wname, dt)
    levels, nr = len(bands) - 1, bands[0].shape[0]
    lens = R1.level_lens(n0, h, levels)
    a = D.put(bands[0])
    for l in range(levels, 0, -1):
        out = D.put(np.full((nr, lens[l - 1]), np.nan, dt))
        assert getattr(L, "pdwt_ext1d_inverse_level_" + sfx)(out, a, D.put(bands[l]), nr, lens[l - 1], C.byref(f)) == 0
        a = out
    return D.get(a, (nr, n0), dt)


# ---- one level through the drivers (also the shapes below the clamp of the class) ---------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("mode", R1.MODES)
def test_one_level_of_3x7_db4_through_the_level_drivers(mode, dt):
    """the halo of n - 1 samples: every window position outside the row folds once, to the far end of the line"""
    shape = (3, 7)
    x, ref = _ref(shape, "db4", 1, mode, np.dtype(dt).name)
    W = BoundaryWavelets1D(x, "db4", 1, mode)
    assert W.state == W_CREATION_ERROR and W.nbands == 0 and not W.fused  # the class refuses it: a clamp to 0 levels
    with _Dev() as D:
        got = _chain_forward(D, x, "db4", 1, mode, dt)
        assert got[0].shape == (3, 7)
        _check_bands(got, ref, FWD[np.dtype(dt)], "3x7 db4 %s %s" % (mode, np.dtype(dt).name))
        e = band_err(_chain_inverse(D, got, 7, "db4", dt), x)
        print("round trip %.3e" % e)
        assert e <= RT[np.dtype(dt)], e


@pytest.mark.parametrize("dt", DTYPES)
def test_more_rows_than_a_grid_dimension_through_the_level_drivers(dt):
    shape, wname = (70001, 16), "db2"
    x, ref = _ref(shape, wname, 1, "symmetric", np.dtype(dt).name)
    with _Dev() as D:
        got = _chain_forward(D, x, wname, 1, "symmetric", dt)
        _check_bands(got, ref, FWD[np.dtype(dt)], "70001x16 db2 level drivers %s" % np.dtype(dt).name)
        e = band_err(_chain_inverse(D, got, 16, wname, dt), x)
        assert e <= RT[np.dtype(dt)], e


# ---- forward and round trip of the class --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape,wname,levels,mode", CLASS_RUNS, ids=[_id(r) for r in CLASS_RUNS])
def test_forward_every_band_and_round_trip(shape, wname, levels, mode, dt):
    x, ref = _ref(shape, wname, levels, mode, np.dtype(dt).name)
    W = BoundaryWavelets1D(x, wname, levels, mode)
    assert W.state == W_INIT and W.dtype == np.dtype(dt) and W.levels == levels and W.mode == mode and W.nbands == levels + 1 and W.shape == shape
    F = W.info.hlen
    assert [W.coeff_shape(k) for k in range(W.nbands)] == [(shape[0], n) for n in R1.band_lens(shape[1], F, levels)]
    if shape == (2, 4099):
        assert W.fused
    if shape == (2, 40037):
        assert not W.fused
    what = "%s %s L%d %s %s %s" % (shape, wname, levels, mode, np.dtype(dt).name, "one launch" if W.fused else "per level")
    W.forward()
    assert W.state == W_FORWARD
    got = W.coeffs
    _check_bands(got, ref, FWD[np.dtype(dt)], what)
    assert _same_bits(W.get_image(), x)  # forward() leaves the batch bit-unchanged
    W.set_image(np.zeros(shape, dt))  # the reconstruction must come from the bands, not from what the image still held
    assert W.state == W_INIT
    W.inverse()
    assert W.state == W_INVERSE
    e = band_err(W.get_image(), x)
    print("round trip %.3e" % e)
    assert e <= RT[np.dtype(dt)], e
    assert all(_same_bits(a, b) for a, b in zip(_raw_bands(W), got))  # inverse() leaves the bands bit-unchanged
    # the wrapped ramp through the same instance
    xr, refr = _ref(shape, wname, levels, mode, np.dtype(dt).name, "ramp")
    W.set_image(xr)
    W.forward()
    _check_bands(W.coeffs, refr, FWD[np.dtype(dt)], what + " ramp")
    W.inverse()
    e = band_err(W.get_image(), xr)
    assert e <= RT[np.dtype(dt)], e


# ---- the two kernel forms ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape,wname,levels,mode", FUSED_RUNS, ids=[_id(r) for r in FUSED_RUNS])
def test_one_launch_and_level_kernels_agree_bit_for_bit(shape, wname, levels, mode, dt):
    x, _ = _ref(shape, wname, levels, mode, np.dtype(dt).name)
    W = BoundaryWavelets1D(x, wname, levels, mode)
    assert W.fused and W.levels == levels
    W.forward()
    got = W.coeffs
    with _Dev() as D:
        chained = _chain_forward(D, x, wname, levels, mode, dt)
        for k, (a, b) in enumerate(zip(got, chained)):
            assert _same_bits(a, b), ("forward band", k)
        W.inverse()
        assert _same_bits(W.get_image(), _chain_inverse(D, got, shape[1], wname, dt))


# ---- the inverse alone ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape,wname,levels", [((5, 77), "haar", 3), ((300, 33), "db2", 2), ((2, 4099), "db4", 5), ((2, 96), "db20", 1), ((2, 40037), "db4", 3)])
def test_inverse_from_bands_written_with_set_coeff(shape, wname, levels, dt):
    """random bands (not the transform of any batch), against the reference inverse: tests the inverse without the forward"""
    F, _ = R.bank(wname)
    rs = np.random.RandomState(9)
    bands = [rs.standard_normal((shape[0], n)).astype(dt) for n in R1.band_lens(shape[1], F, levels)]
    want = R1.waverec(bands, shape[1], wname, np.float64)
    W = BoundaryWavelets1D(np.zeros(shape, dt), wname, levels, "symmetric")
    assert W.levels == levels
    for k, b in enumerate(bands):
        W.set_coeff(b, k)
    assert W.state == W_INIT and all(_same_bits(a, b) for a, b in zip(W.coeffs, bands))
    W.inverse()
    assert W.state == W_INVERSE
    e = band_err(W.get_image(), want)
    print("%s %s L%d %s: inverse of random bands %.3e" % (shape, wname, levels, np.dtype(dt).name, e))
    assert e <= FWD[np.dtype(dt)], e
    assert all(_same_bits(a, b) for a, b in zip(_raw_bands(W), bands))


# ---- corner impulses: the ends of a row, and no leak between the rows of a pack -----------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("mode", R1.MODES)
@pytest.mark.parametrize("shape,wname,levels,row", [((300, 33), "db2", 2, 17), ((5, 77), "haar", 3, 2), ((4, 64), "db2", 3, 0), ((2, 4099), "db4", 5, 1)])
def test_corner_impulses_stay_in_their_row(shape, wname, levels, row, mode, dt):
    for col in (0, shape[1] - 1):
        x = np.zeros(shape, dt)
        x[row, col] = 1.0
        ref = R1.wavedec(x[row:row + 1], wname, levels, mode, np.float64)
        W = BoundaryWavelets1D(x, wname, levels, mode)
        W.forward()
        got = W.coeffs
        for k, g in enumerate(got):
            others = np.delete(g, row, axis=0)
            assert not others.any(), (col, "band", k, "leaks into", np.argwhere(others)[:3])
            # (a band whose reference is exactly 0 -- Haar details of a constant extension -- is held to the bound in absolute terms,
            # the input being 1: helpers.band_err divides by 1 there)
            assert band_err(g[row:row + 1], ref[k]) <= FWD[np.dtype(dt)], (col, k)
        W.inverse()
        out = W.get_image()
        assert not np.delete(out, row, axis=0).any() and band_err(out, x) <= RT[np.dtype(dt)]


def test_the_modes_differ_on_the_ramp_and_only_near_the_ends():
    shape, wname, F = (3, 200), "db4", 8
    got = {}
    for mode in R1.MODES:
        W = BoundaryWavelets1D(R1.make_input(shape, np.float64, "ramp"), wname, 1, mode)
        W.forward()
        got[mode] = W.coeffs
    lo, hi = (F - 2) // 2, (shape[1] - 2) // 2 + 1  # positions whose window 2i + 1 - k lies inside 0 .. n-1
    for a in range(5):
        for b in range(a + 1, 5):
            ga, gb = got[R1.MODES[a]], got[R1.MODES[b]]
            assert any(not np.array_equal(u, v) for u, v in zip(ga, gb)), (R1.MODES[a], R1.MODES[b])
            for u, v in zip(ga, gb):
                assert np.array_equal(u[:, lo:hi], v[:, lo:hi])


# ---- thresholds, norms, statistics ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("kind,app", [("soft", 0), ("hard", 0), ("soft", 1), ("hard", 1)])
def test_thresholds_touch_exactly_the_bands_they_should(kind, app, dt):
    x = R1.make_input((6, 200), dt)
    W = BoundaryWavelets1D(x, "db4", 2, "symmetric")
    W.forward()
    before = W.coeffs
    getattr(W, kind + "_threshold")(0.5, do_thresh_appcoeffs=app)
    after = W.coeffs
    for k, (b, a) in enumerate(zip(before, after)):
        if k == 0 and not app:
            assert _same_bits(a, b)  # the approximation only when asked
        else:
            assert _same_bits(a, ref_threshold(b, 0.5, kind)) and not _same_bits(a, b), k
    want = sum(np.abs(a.astype(np.float64)).sum() for a in after)
    assert abs(W.norm1() - want) <= SUM_TOL * want
    betas = [-1.0, 0.25, 0.0]
    W.threshold_bands(betas, kind)
    for k, (b, a) in enumerate(zip(after, W.coeffs)):
        assert _same_bits(a, ref_threshold(b, betas[k], kind)), k


@pytest.mark.parametrize("dt", DTYPES)
def test_norm1_statistics_sigma_and_denoise_on_the_reference_bands(dt):
    """the reference's bands written with set_coeff, so that the statistics are those of tests/refstats.py on known data"""
    shape, wname, levels = (12, 300), "sym8", 2
    rs = np.random.RandomState(7)
    x = (rs.standard_normal(shape) * 3 + rs.uniform(-1, 1, shape).cumsum(axis=-1)).astype(dt)
    bands = [b.astype(dt) for b in R1.wavedec(x, wname, levels, "symmetric", np.float64)]
    stats = [ref_stats(b) for b in bands]

    def fresh():
        W = BoundaryWavelets1D(x, wname, levels, "symmetric")
        W.forward()
        for k, b in enumerate(bands):
            W.set_coeff(b, k)
        assert W.state == W_FORWARD
        return W

    W = fresh()
    want = sum(s["sum_abs"] for s in stats)
    assert abs(W.norm1() - want) <= SUM_TOL * want
    every, plain = W.all_band_stats(with_median=True), W.all_band_stats()
    for k, s in enumerate(stats):
        one = W.band_stats(k)
        assert one["n"] == s["n"] and one["max_abs"] == s["max_abs"] and one["median_abs"] == s["median_abs"], k
        assert abs(one["sum_abs"] - s["sum_abs"]) <= SUM_TOL * s["sum_abs"] and abs(one["sum_sq"] - s["sum_sq"]) <= SUM_TOL * s["sum_sq"], k
        for key in one:
            assert np.float64(one[key]).tobytes() == np.float64(every[k][key]).tobytes(), (k, key)
            if key != "median_abs":
                assert np.float64(one[key]).tobytes() == np.float64(plain[k][key]).tobytes(), (k, key)
        assert np.isnan(plain[k]["median_abs"])
    sigma = stats[1]["median_abs"] / MAD_SCALE  # the finest detail band: D_1, all rows together
    assert W.estimate_sigma() == sigma
    for method in ("visu", "bayes"):
        for kind in ("soft", "hard"):
            for given in (None, 0.8):
                W = fresh()
                r = W.denoise(method, sigma=given, kind=kind)
                s_used = sigma if given is None else given
                assert r["sigma"] == s_used
                betas = r["betas"]
                assert betas.dtype == np.dtype(dt) and betas.shape == (levels + 1,) and betas[0] == -1
                wantb = ref_betas(stats, s_used, method, float(shape[1]))  # N of the universal threshold: the length of a row
                rel = np.abs(betas[1:].astype(np.float64) - wantb[1:]) / np.abs(wantb[1:])
                assert rel.max() <= (1e-6 if dt == np.float32 else 1e-10), (method, kind, rel.max())
                for k, (b, a) in enumerate(zip(bands, W.coeffs)):
                    assert _same_bits(a, ref_threshold(b, betas[k], kind)), (method, kind, k)
                assert W.state == W_FORWARD


# ---- state machine and errors ----------------------------------------------------------------------------------------------------------
def test_state_machine_refusals_leave_the_data_alone():
    x = R1.make_input((4, 64), np.float32)
    W = BoundaryWavelets1D(x, "db2", 3)
    assert W.mode == "symmetric"

    def all_refuse(stats_only):
        calls = [lambda: W.band_stats(1), lambda: W.all_band_stats(), lambda: W.estimate_sigma(), lambda: W.threshold_bands([1.0] * W.nbands),
                 lambda: W.denoise("bayes"), lambda: W.denoise("visu", sigma=1.0)]
        if not stats_only:
            calls += [lambda: W.get_coeff(0), lambda: W.coeffs, lambda: W.soft_threshold(1.0), lambda: W.hard_threshold(1.0), lambda: W.norm1()]
        for call in calls:
            with pytest.raises(RuntimeError):
                call()

    all_refuse(stats_only=True)  # before forward(): the statistics need the coefficients of a forward()
    W.forward()
    with pytest.raises(IndexError):
        W.band_stats(W.nbands)
    with pytest.raises(IndexError):
        W.coeff_shape(4)
    with pytest.raises(IndexError):
        W.coeff_view(-1)
    with pytest.raises(ValueError):
        W.threshold_bands([1.0] * (W.nbands - 1))
    with pytest.raises(ValueError):
        W.denoise("sure")
    with pytest.raises(ValueError):
        W.set_coeff(np.zeros((3, 3), np.float32), 1)
    W.inverse()
    assert W.state == W_INVERSE
    snap, img = _raw_bands(W), W.get_image()
    all_refuse(stats_only=False)  # after inverse()
    W.inverse()  # refused with a warning
    assert W.state == W_INVERSE and _same_bits(W.get_image(), img)
    assert all(_same_bits(a, b) for a, b in zip(_raw_bands(W), snap))
    W.set_image(x)
    assert W.state == W_INIT
    all_refuse(stats_only=True)
    W.forward()
    assert W.state == W_FORWARD and W.estimate_sigma() >= 0


def test_creation_errors_and_bad_arguments():
    x = R1.make_input((4, 64), np.float32)
    assert BoundaryWavelets1D(x, "nosuchwavelet", 2).state == W_CREATION_ERROR
    assert BoundaryWavelets1D(x, "db2", 2, mode=5).state == W_CREATION_ERROR
    for shape in ((64, 6), (3, 7)):  # ilog2(6 / 7) = ilog2(7 / 7) = 0 levels
        W = BoundaryWavelets1D(R1.make_input(shape, np.float32), "db4", 2)
        assert W.state == W_CREATION_ERROR and W.nbands == 0 and not W.fused
        W.forward()
        W.inverse()
        assert W.state == W_CREATION_ERROR
        for call in (lambda: W.get_coeff(0), lambda: W.get_image(), lambda: W.set_image(np.zeros(shape, np.float32)), lambda: W.norm1()):
            with pytest.raises((RuntimeError, IndexError)):
                call()
    with pytest.raises(ValueError):
        BoundaryWavelets1D(x, "db2", 2, mode="smooth")
    with pytest.raises(ValueError):
        BoundaryWavelets1D(x, "db2", 2, mode="periodization")
    with pytest.raises(ValueError):
        BoundaryWavelets1D(np.zeros((4, 8, 8), np.float32), "db2", 1)
    assert BoundaryWavelets1D(R1.make_input((2, 80), np.float32), "db4", 9).levels == 3  # clamped as Wavelets(ndim=1): ilog2(80 / 7)
    assert BoundaryWavelets1D(R1.make_input((7, 64), np.float32), "db4", 3).levels == 3   # the rows do not count: 7 rows of 64 samples
    assert BoundaryWavelets1D(x, "db2", 0).levels == 1
    one = BoundaryWavelets1D(np.arange(64, dtype=np.float64), "db2", 2)  # a 1-D array is one row
    assert one.shape == (1, 64) and one.coeff_shape(0) == (1, 18)


@pytest.mark.parametrize("dt", DTYPES)
def test_device_tensors_and_zero_copy_views(dt):
    import torch
    x = R1.make_input((5, 77), dt)
    t = torch.as_tensor(x, device="cuda")
    W = BoundaryWavelets1D(t, "db2", 2, "reflect")
    H = BoundaryWavelets1D(x, "db2", 2, "reflect")
    assert W.dtype == np.dtype(dt) and W.shape == (5, 77) and W.mode == "reflect"
    W.forward()
    H.forward()
    assert all(_same_bits(a, b) for a, b in zip(W.coeffs, H.coeffs))
    v = W.coeff_view(1)
    assert v.ptr == W.coeff_int_ptr(1) and v.shape == W.coeff_shape(1) and v.ptr % 256 == 0
    assert W.image_view().ptr == W.image_int_ptr() and _same_bits(W.image_view().numpy(), x)
    W.sync()
    tv = torch.as_tensor(v, device="cuda")
    assert tv.data_ptr() == v.ptr and np.array_equal(tv.cpu().numpy(), W.get_coeff(1))
    tv.zero_()  # a write through the view lands in the band
    torch.cuda.synchronize()
    assert not W.get_coeff(1).any()
    W.set_coeff(torch.as_tensor(H.get_coeff(1), device="cuda"), 1)
    assert _same_bits(W.get_coeff(1), H.get_coeff(1)) and W.state == W_FORWARD
    W.set_image(torch.as_tensor(x[::-1].copy(), device="cuda"))
    assert np.array_equal(W.get_image(), x[::-1]) and W.state == W_INIT
    with pytest.raises(TypeError):
        BoundaryWavelets1D(t, "db2", 2, dtype=np.float64 if dt == np.float32 else np.float32)


# ---- the point of the feature -----------------------------------------------------------------------------------------------------------
def _soft(v, beta):
    return np.copysign(np.maximum(np.abs(v) - beta, 0.0), v)


@pytest.mark.parametrize("dt", DTYPES)
def test_a_step_between_the_ends_of_a_row_does_not_wrap_around(dt):
    """Rows of 64 samples, 0 on their first half and 100 on their second: a step between the first and the last sample of the row.
    db4 L2, soft-thresholded at beta = 5 and inverted.  Periodised, the transform sees a second edge between the last sample and the
    first, and the threshold rings around it: sample 0 moves.  With `symmetric` sample 0 stays where the float64 reference puts it
    (its input, 0) within the forward bound relative to the row's maximum."""
    beta = 5.0
    x = np.zeros((4, 64), dt)
    x[:, 32:] = 100.0
    W = BoundaryWavelets1D(x, "db4", 2, "symmetric")
    W.forward()
    W.soft_threshold(beta)
    W.inverse()
    got = W.get_image()
    bands = R1.wavedec(x, "db4", 2, "symmetric", np.float64)
    want = R1.waverec([bands[0]] + [_soft(b, beta) for b in bands[1:]], 64, "db4", np.float64)
    assert np.abs(want[:, 0]).max() <= 1e-10  # the reference: sample 0 does not feel the edge
    sym = np.abs(got[:, 0].astype(np.float64) - x[:, 0]).max()
    e_all = band_err(got, want)
    P = Wavelets(x, "db4", 2, ndim=1)
    P.forward()
    P.soft_threshold(beta)
    P.inverse()
    per = np.abs(P.get_image()[:, 0].astype(np.float64) - x[:, 0]).max()
    print("%s: sample 0 moves by %.3e with symmetric, by %.3e periodised; whole batch against the reference %.3e" % (np.dtype(dt).name, sym, per, e_all))
    assert sym / 100.0 <= FWD[np.dtype(dt)] and e_all <= RT[np.dtype(dt)]
    assert per > 100 * sym
