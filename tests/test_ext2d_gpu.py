"""BoundaryWavelets2D (the 2-D DWT with signal-extension boundary modes) on the GPU against tests/refext.py, the float64 numpy
reference (pinned on the CPU in tests/test_refext_cpu.py).

Metric: tests/helpers.band_err per band (max |got - ref| / max |ref| of that band).  Bounds: 1e-5 (float32) and 1e-12 (float64) for
every band; 10x those for a round trip back to the image.  The reference alone round-trips every bank of the cases to below a tenth of
the float64 round-trip bound (sym8: 8.7e-13, everything else below 2e-15; tests/test_refext_cpu.py), so no bank has a looser one; its
float32 evaluation stays within a quarter of the float32 bounds on every input used here.

The 7 x 7 db4 case lies below the level clamp of the class (ilog2(7 / 7) = 0 levels: W_CREATION_ERROR, as for Wavelets), so it runs
through the level drivers, which take any line of at least hlen - 1 samples.

The "ramp" input is a wrapped ramp, ((3x + 5y) mod 17) - 8: along every border it is a ramp (where symmetric, reflect and constant
differ), but its detail bands are not small.  A plain or bilinear ramp cannot be held to a per-band bound: under the mirror modes its
detail bands are zero up to rounding (D of x + 2y analytically; those of (x + 1)(y + 2) / 8 reach 7e-3 on an image that reaches 500),
so the band-normalised error of ANY float32 evaluation is far above 1e-5 there (the reference's own: up to 4.5e-3 on 61 x 67 db4).
"""
import ctypes as C
import functools

import numpy as np
import pytest

import pdwt_amd
from pdwt_amd import BoundaryWavelets2D, DeviceArray, Wavelets
from pdwt_amd import _native as nat
from pdwt_amd.wavelets import W_CREATION_ERROR, W_FORWARD, W_INIT, W_INVERSE
from tests import refext as R
from tests.helpers import band_err
from tests.refstats import MAD_SCALE, ref_betas, ref_stats, ref_threshold

pytestmark = pytest.mark.gpu

FWD = {np.dtype(np.float32): 1e-5, np.dtype(np.float64): 1e-12}
RT = {k: 10 * v for k, v in FWD.items()}
SUM_TOL = 1e-10  # sums accumulated in double (tests/test_bandstats_gpu.py)
DTYPES = [np.float32, np.float64]
RUNS = [(shape, wname, levels, mode) for shape, wname, levels, modes in R.CASES for mode in modes]
CLASS_RUNS = [r for r in RUNS if r[0] != (7, 7)]
_ids = ["%dx%d-%s-L%d-%s" % (r[0] + r[1:]) for r in RUNS]


def _input(shape, dt, kind="uniform"):
    if kind == "uniform":
        return np.random.RandomState(1).uniform(-100, 100, shape).astype(dt)
    if kind == "impulse":
        x = np.zeros(shape, dt)
        x[0, 0], x[-1, -1], x[0, -1], x[-1, 0] = 100.0, -50.0, 25.0, -75.0
        return x
    assert kind == "ramp"
    yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
    return ((3 * xx + 5 * yy) % 17 - 8.0).astype(dt)


@functools.lru_cache(maxsize=None)
def _ref(shape, wname, levels, mode, dtname, kind="uniform"):
    """(image in the dtype under test, float64 reference bands of it): computed once per case and shared; callers do not modify them"""
    x = _input(shape, np.dtype(dtname), kind)
    bands = R.wavedec2(x, wname, levels, mode, np.float64)
    for b in bands:
        b.setflags(write=False)
    x.setflags(write=False)
    return x, bands


def _check_bands(got, ref, bound, what):
    assert len(got) == len(ref), (what, len(got), len(ref))
    L = (len(ref) - 1) // 3
    errs = []
    for k, (g, r) in enumerate(zip(got, ref)):
        assert g.shape == r.shape, (what, k, g.shape, r.shape)
        errs.append(band_err(g, r))
    print("%s: A%d %.3e" % (what, L, errs[0]) + "".join(" | level %d H %.3e V %.3e D %.3e" % ((l,) + tuple(errs[3 * l - 2:3 * l + 1])) for l in range(1, L + 1)))
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


# ---- one level through the drivers (also the shapes below the clamp of the class) ---------------------------------------------------
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


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("mode", R.MODES)
def test_one_level_of_7x7_db4_through_the_level_drivers(mode, dt):
    """the halo of n - 1 samples: every window position outside the image folds once, to the far end of the line"""
    shape = (7, 7)
    x, ref = _ref(shape, "db4", 1, mode, np.dtype(dt).name)
    L, sfx, f, h = _bank("db4", dt)
    hr, hc = ref[0].shape
    assert (hr, hc) == (7, 7)
    with _Dev() as D:
        src = D.put(x)
        b = [D.put(np.full((hr, hc), np.nan, dt)) for _ in range(4)]
        assert getattr(L, "pdwt_ext2d_forward_level_" + sfx)(src, b[0], b[1], b[2], b[3], 7, 7, R.MODES.index(mode), C.byref(f)) == 0
        got = [D.get(p, (hr, hc), dt) for p in b]
        _check_bands(got, ref, FWD[np.dtype(dt)], "7x7 db4 %s %s" % (mode, np.dtype(dt).name))
        dst = D.put(np.full(shape, np.nan, dt))
        assert getattr(L, "pdwt_ext2d_inverse_level_" + sfx)(dst, b[0], b[1], b[2], b[3], 7, 7, C.byref(f)) == 0
        e = band_err(D.get(dst, shape, dt), x)
        print("round trip %.3e" % e)
        assert e <= RT[np.dtype(dt)], e
        assert _same_bits(D.get(src, shape, dt), x) and all(_same_bits(D.get(p, (hr, hc), dt), g) for p, g in zip(b, got))


# ---- forward and round trip of the class --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape,wname,levels,mode", CLASS_RUNS, ids=[i for i, r in zip(_ids, RUNS) if r[0] != (7, 7)])
def test_forward_every_band_and_round_trip(shape, wname, levels, mode, dt):
    x, ref = _ref(shape, wname, levels, mode, np.dtype(dt).name)
    W = BoundaryWavelets2D(x, wname, levels, mode)
    assert W.state == W_INIT and W.dtype == np.dtype(dt) and W.levels == levels and W.mode == mode and W.nbands == 3 * levels + 1
    F = W.info.hlen
    assert [W.coeff_shape(k) for k in range(W.nbands)] == R.band_shapes(shape, F, levels)
    W.forward()
    assert W.state == W_FORWARD
    got = W.coeffs
    _check_bands(got, ref, FWD[np.dtype(dt)], "%s %s L%d %s %s" % (shape, wname, levels, mode, np.dtype(dt).name))
    assert _same_bits(W.get_image(), x)  # forward() leaves the image bit-unchanged
    W.set_image(np.zeros(shape, dt))  # the reconstruction must come from the bands, not from what the image still held
    assert W.state == W_INIT
    W.inverse()
    assert W.state == W_INVERSE
    e = band_err(W.get_image(), x)
    print("round trip %.3e" % e)
    assert e <= RT[np.dtype(dt)], e
    assert all(_same_bits(a, b) for a, b in zip(_raw_bands(W), got))  # inverse() leaves the bands bit-unchanged


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("kind", ["impulse", "ramp"])
@pytest.mark.parametrize("shape,wname,levels", [((61, 67), "db4", 2), ((33, 47), "haar", 3)])
def test_corner_impulses_and_ramp(shape, wname, levels, kind, mode, dt):
    """corner impulses: everything near a corner comes through the extension of both axes; the (wrapped) ramp: the modes differ along
    every border"""
    x, ref = _ref(shape, wname, levels, mode, np.dtype(dt).name, kind)
    W = BoundaryWavelets2D(x, wname, levels, mode)
    W.forward()
    _check_bands(W.coeffs, ref, FWD[np.dtype(dt)], "%s %s %s %s %s" % (shape, wname, kind, mode, np.dtype(dt).name))
    W.inverse()
    assert band_err(W.get_image(), x) <= RT[np.dtype(dt)]


def test_the_modes_differ_on_the_ramp_and_only_near_the_border():
    """what the ramp is for: the five modes give different bands, and they differ only where a window leaves the image"""
    shape, wname = (61, 67), "db4"
    got = {}
    for mode in R.MODES:
        W = BoundaryWavelets2D(_input(shape, np.float64, "ramp"), wname, 1, mode)
        W.forward()
        got[mode] = W.coeffs
    F = 8
    lo, hi_r, hi_c = (F - 2) // 2, (shape[0] - 2) // 2 + 1, (shape[1] - 2) // 2 + 1  # positions whose window 2i + 1 - k lies inside 0 .. n-1
    for a in range(5):
        for b in range(a + 1, 5):
            ga, gb = got[R.MODES[a]], got[R.MODES[b]]
            assert any(not np.array_equal(u, v) for u, v in zip(ga, gb)), (R.MODES[a], R.MODES[b])
            for u, v in zip(ga, gb):
                assert np.array_equal(u[lo:hi_r, lo:hi_c], v[lo:hi_r, lo:hi_c])


# ---- the inverse alone ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape,wname,levels", [((61, 67), "db4", 2), ((33, 47), "haar", 3), ((104, 200), "db2", 2), ((96, 80), "db20", 1)])
def test_inverse_from_bands_written_with_set_coeff(shape, wname, levels, dt):
    """random bands (not the transform of any image), against the reference inverse: tests the inverse without the forward"""
    F, _ = R.bank(wname)
    rs = np.random.RandomState(9)
    bands = [rs.uniform(-100, 100, s).astype(dt) for s in R.band_shapes(shape, F, levels)]
    want = R.waverec2(bands, shape, wname, np.float64)
    W = BoundaryWavelets2D(np.zeros(shape, dt), wname, levels, "symmetric")
    assert W.levels == levels
    for k, b in enumerate(bands):
        W.set_coeff(b, k)
    assert W.state == W_INIT and all(_same_bits(a, b) for a, b in zip(W.coeffs, bands))
    W.inverse()
    e = band_err(W.get_image(), want)
    print("%s %s L%d %s: inverse of random bands %.3e" % (shape, wname, levels, np.dtype(dt).name, e))
    assert e <= FWD[np.dtype(dt)], e
    assert all(_same_bits(a, b) for a, b in zip(_raw_bands(W), bands))


# ---- thresholds, norms, statistics ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("kind,app", [("soft", 0), ("hard", 0), ("soft", 1), ("hard", 1)])
def test_thresholds_touch_exactly_the_bands_they_should(kind, app, dt):
    x = _input((61, 67), dt)
    W = BoundaryWavelets2D(x, "db4", 2, "symmetric")
    W.forward()
    before = W.coeffs
    getattr(W, kind + "_threshold")(30.0, do_thresh_appcoeffs=app)
    after = W.coeffs
    for k, (b, a) in enumerate(zip(before, after)):
        if k == 0 and not app:
            assert _same_bits(a, b)  # the approximation only when asked
        else:
            assert _same_bits(a, ref_threshold(b, 30.0, kind)) and not _same_bits(a, b), k
    want = sum(np.abs(a.astype(np.float64)).sum() for a in after)
    assert abs(W.norm1() - want) <= SUM_TOL * want
    W.threshold_bands([-1.0, 5.0, -1.0, 7.0, -1.0, -1.0, 0.0], kind)
    for k, (b, a) in enumerate(zip(after, W.coeffs)):
        assert _same_bits(a, ref_threshold(b, [-1.0, 5.0, -1.0, 7.0, -1.0, -1.0, 0.0][k], kind)), k


@pytest.mark.parametrize("dt", DTYPES)
def test_norm1_statistics_sigma_and_denoise_on_the_reference_bands(dt):
    """the reference's bands written with set_coeff, so that the statistics are those of tests/refstats.py on known data"""
    shape, wname, levels = (64, 96), "sym8", 2
    rs = np.random.RandomState(7)
    x = (rs.standard_normal(shape) * 3 + rs.uniform(-1, 1, shape).cumsum(axis=-1)).astype(dt)
    bands = [b.astype(dt) for b in R.wavedec2(x, wname, levels, "symmetric", np.float64)]
    stats = [ref_stats(b) for b in bands]

    def fresh():
        W = BoundaryWavelets2D(x, wname, levels, "symmetric")
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
    sigma = stats[3]["median_abs"] / MAD_SCALE  # the finest diagonal band: D1
    assert W.estimate_sigma() == sigma
    for method in ("visu", "bayes"):
        for kind in ("soft", "hard"):
            for given in (None, 0.8):
                W = fresh()
                r = W.denoise(method, sigma=given, kind=kind)
                s_used = sigma if given is None else given
                assert r["sigma"] == s_used
                betas = r["betas"]
                assert betas.dtype == np.dtype(dt) and betas.shape == (7,) and betas[0] == -1
                wantb = ref_betas(stats, s_used, method, float(shape[0] * shape[1]))
                rel = np.abs(betas[1:].astype(np.float64) - wantb[1:]) / np.abs(wantb[1:])
                assert rel.max() <= (1e-6 if dt == np.float32 else 1e-10), (method, kind, rel.max())
                for k, (b, a) in enumerate(zip(bands, W.coeffs)):
                    assert _same_bits(a, ref_threshold(b, betas[k], kind)), (method, kind, k)
                assert W.state == W_FORWARD


# ---- state machine and errors ----------------------------------------------------------------------------------------------------------
def test_state_machine_refusals_leave_the_data_alone():
    x = _input((64, 64), np.float32)
    W = BoundaryWavelets2D(x, "db2", 3)
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
        W.coeff_shape(10)
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
    x = _input((64, 64), np.float32)
    assert BoundaryWavelets2D(x, "nosuchwavelet", 2).state == W_CREATION_ERROR
    assert BoundaryWavelets2D(x, "db2", 2, mode=5).state == W_CREATION_ERROR
    for shape in ((6, 64), (7, 7)):  # ilog2(6 / 7) = ilog2(7 / 7) = 0 levels
        W = BoundaryWavelets2D(_input(shape, np.float32), "db4", 2)
        assert W.state == W_CREATION_ERROR and W.nbands == 0
        W.forward()
        W.inverse()
        assert W.state == W_CREATION_ERROR
        for call in (lambda: W.get_coeff(0), lambda: W.get_image(), lambda: W.set_image(np.zeros(shape, np.float32)), lambda: W.norm1()):
            with pytest.raises((RuntimeError, IndexError)):
                call()
    with pytest.raises(ValueError):
        BoundaryWavelets2D(x, "db2", 2, mode="smooth")
    with pytest.raises(ValueError):
        BoundaryWavelets2D(x, "db2", 2, mode="periodization")
    with pytest.raises(ValueError):
        BoundaryWavelets2D(np.zeros((4, 8, 8), np.float32), "db2", 1)
    assert BoundaryWavelets2D(_input((96, 80), np.float32), "db4", 9).levels == 3  # clamped as Wavelets
    assert BoundaryWavelets2D(x, "db2", 0).levels == 1


@pytest.mark.parametrize("dt", DTYPES)
def test_device_tensors_and_zero_copy_views(dt):
    import torch
    x = _input((61, 67), dt)
    t = torch.as_tensor(x, device="cuda")
    W = BoundaryWavelets2D(t, "db2", 2, "reflect")
    H = BoundaryWavelets2D(x, "db2", 2, "reflect")
    assert W.dtype == np.dtype(dt) and W.shape == (61, 67) and W.mode == "reflect"
    W.forward()
    H.forward()
    assert all(_same_bits(a, b) for a, b in zip(W.coeffs, H.coeffs))
    v = W.coeff_view(3)
    assert v.ptr == W.coeff_int_ptr(3) and v.shape == W.coeff_shape(3) and v.ptr % 256 == 0
    assert W.image_view().ptr == W.image_int_ptr() and _same_bits(W.image_view().numpy(), x)
    W.sync()
    tv = torch.as_tensor(v, device="cuda")
    assert tv.data_ptr() == v.ptr and np.array_equal(tv.cpu().numpy(), W.get_coeff(3))
    tv.zero_()  # a write through the view lands in the band
    torch.cuda.synchronize()
    assert not W.get_coeff(3).any()
    W.set_coeff(torch.as_tensor(H.get_coeff(3), device="cuda"), 3)
    assert _same_bits(W.get_coeff(3), H.get_coeff(3)) and W.state == W_FORWARD
    W.set_image(torch.as_tensor(x[::-1].copy(), device="cuda"))
    assert np.array_equal(W.get_image(), x[::-1]) and W.state == W_INIT
    with pytest.raises(TypeError):
        BoundaryWavelets2D(t, "db2", 2, dtype=np.float64 if dt == np.float32 else np.float32)


# ---- the point of the feature -----------------------------------------------------------------------------------------------------------
def _soft(v, beta):
    return np.copysign(np.maximum(np.abs(v) - beta, 0.0), v)


@pytest.mark.parametrize("dt", DTYPES)
def test_a_step_edge_does_not_ghost_onto_the_opposite_border(dt):
    """A 64 x 64 image, 0 on its left half and 100 on its right half, soft-thresholded at beta = 5 with db4 L2.  Periodised, the
    transform sees a second edge between the last column and the first, and the threshold rings around it: the reference alone (the
    oracle's periodised transform, float64) moves column 0 by more than 1.  With `symmetric` column 0 of the result is 0 as before,
    within the forward bound (relative to the image's maximum) of the float64 reference's result."""
    beta = 5.0
    x = np.zeros((64, 64), dt)
    x[:, 32:] = 100.0
    W = BoundaryWavelets2D(x, "db4", 2, "symmetric")
    W.forward()
    W.soft_threshold(beta)
    W.inverse()
    got = W.get_image()
    bands = R.wavedec2(x, "db4", 2, "symmetric", np.float64)
    want = R.waverec2([bands[0]] + [_soft(b, beta) for b in bands[1:]], (64, 64), "db4", np.float64)
    assert np.abs(want[:, 0]).max() <= 1e-10  # the reference: column 0 does not feel the edge
    e_col = np.abs(got[:, 0].astype(np.float64) - want[:, 0]).max() / np.abs(want).max()
    e_all = band_err(got, want)
    print("%s: column 0 err %.3e, image err %.3e, max |column 0| %.3e" % (np.dtype(dt).name, e_col, e_all, np.abs(got[:, 0]).max()))
    assert e_col <= FWD[np.dtype(dt)] and e_all <= RT[np.dtype(dt)]
    # the periodised transform of the same image: the reference alone shows the ghost
    from oracle import oracle as orc
    O = orc.OracleWavelets(x.astype(np.float64), "db4", 2)
    O.forward()
    O.soft_threshold(beta)
    O.inverse()
    ghost = np.abs(O.get_image()[:, 0]).max()
    print("periodised reference: max |column 0| %.3f" % ghost)
    assert ghost >= 1.0
    P = Wavelets(x, "db4", 2)
    P.forward()
    P.soft_threshold(beta)
    P.inverse()
    assert np.abs(P.get_image()[:, 0]).max() >= 1.0
