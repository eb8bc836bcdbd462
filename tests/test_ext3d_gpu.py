"""BoundaryWavelets3D (the 3-D DWT of volumes with signal-extension boundary modes) on the GPU against tests/refext3d.py, the float64
numpy reference (pinned on the CPU in tests/test_refext3d_cpu.py).

Metric: tests/helpers.band_err per band (max |got - ref| / max |ref| of that band).  Bounds: those of tests/test_ext2d_gpu.py, 1e-5
(float32) and 1e-12 (float64) for every band and 10x those for a round trip back to the volume: the third pass adds one more rounding
of the same size, and the reference's own float32 evaluation sits 15x or more below the float32 bound on every input used here (at
most 6.7e-7; tests/test_refext3d_cpu.py).  The reference alone round-trips every bank of the cases to a fifth of the float64
round-trip bound or better (sym8 1.4e-12, everything else below 2e-15), so no bank has a looser one.

The 7 x 7 x 7 db4 and 40 x 48 x 40 db20 cases lie below the level clamp of the class (ilog2(7 / 7) = ilog2(40 / 39) = 0 levels:
W_CREATION_ERROR, as for Wavelets3D), so they run through the level drivers, which take any axis of at least hlen - 1 samples.

Inputs: uniform(-100, 100) with seed 1, impulses on the eight corners, and the wrapped ramp ((3x + 5y + 7z) mod 17) - 8 (along every
face it is a ramp, where symmetric, reflect and constant differ, but its detail bands are not small: see tests/test_ext2d_gpu.py).
"""
import ctypes as C
import functools

import numpy as np
import pytest

import pdwt_amd
from pdwt_amd import BoundaryWavelets3D, DeviceArray, Wavelets3D
from pdwt_amd import _native as nat
from pdwt_amd.wavelets import W_CREATION_ERROR, W_FORWARD, W_INIT, W_INVERSE
from tests import refext3d as R3
from tests.bank_matrix import ALL72
from tests.helpers import band_err
from tests.refstats import MAD_SCALE, ref_betas, ref_stats, ref_threshold

pytestmark = pytest.mark.gpu

FWD = {np.dtype(np.float32): 1e-5, np.dtype(np.float64): 1e-12}
RT = {k: 10 * v for k, v in FWD.items()}
SUM_TOL = 1e-10  # sums accumulated in double (tests/test_bandstats_gpu.py)
DTYPES = [np.float32, np.float64]
KINDS = ["uniform", "impulse", "ramp"]
RUNS = [(shape, wname, levels, mode) for shape, wname, levels, modes in R3.CASES for mode in modes]
CLASS_RUNS = [r for r in RUNS if r[0] not in R3.DRIVER_CASES]
DRIVER_RUNS = [r for r in RUNS if r[0] in R3.DRIVER_CASES]


def _id(r):
    return "%dx%dx%d-%s-L%d-%s" % (r[0] + r[1:])


@functools.lru_cache(maxsize=None)
def _ref(shape, wname, levels, mode, dtname, kind="uniform"):
    """(volume in the dtype under test, float64 reference bands of it): computed once per case and shared; callers do not modify them"""
    x = R3.make_input(shape, np.dtype(dtname), kind)
    bands = R3.wavedec3(x, wname, levels, mode, np.float64)
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
    print("%s: worst band %d %.3e" % (what, int(np.argmax(errs)), max(errs)))
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


def _one_level_through_the_drivers(x, ref, wname, mode, dt, what):
    """forward into NaN-filled bands, the checks of a level, the inverse of those bands into a NaN-filled volume; ref: the eight float64
    bands in R3.LEVEL_KEYS order.  Returns (largest band error, the bands, the volume the inverse gave)."""
    dt = np.dtype(dt)
    shape = x.shape
    L, sfx, f, h = _bank(wname, dt)
    bshape = tuple((n + h - 1) // 2 for n in shape)
    assert ref[0].shape == bshape
    ntmp = L.pdwt_ext3d_tmp_elems(*shape, h)
    assert ntmp >= 4 * shape[0] * bshape[1] * bshape[2]
    with _Dev() as D:
        src = D.put(x)
        b = [D.put(np.full(bshape, np.nan, dt)) for _ in range(8)]
        tmp = D.put(np.full(ntmp, np.nan, dt))
        tab = (C.c_void_p * 8)(*b)
        assert getattr(L, "pdwt_ext3d_forward_level_" + sfx)(src, tab, *shape, R3.MODES.index(mode), C.byref(f), tmp) == 0
        got = [D.get(p, bshape, dt) for p in b]
        e = _check_bands(got, ref, FWD[dt], what)
        dst = D.put(np.full(shape, np.nan, dt))
        assert getattr(L, "pdwt_ext3d_inverse_level_" + sfx)(dst, tab, *shape, C.byref(f), tmp) == 0
        back = D.get(dst, shape, dt)
        assert _same_bits(D.get(src, shape, dt), x) and all(_same_bits(D.get(p, bshape, dt), g) for p, g in zip(b, got))
    return e, got, back


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape,wname,levels,mode", DRIVER_RUNS, ids=[_id(r) for r in DRIVER_RUNS])
def test_one_level_through_the_level_drivers(shape, wname, levels, mode, kind, dt):
    """7^3 db4: the halo of n - 1 samples, every window position outside the volume folds once on all three axes; 40 x 48 x 40 db20: 40
    taps, the LDS opt-in of the x-y kernels, a 70-plane register window"""
    assert levels == 1
    x, ref = _ref(shape, wname, 1, mode, np.dtype(dt).name, kind)
    what = "%s %s %s %s %s" % (shape, wname, mode, kind, np.dtype(dt).name)
    _, _, back = _one_level_through_the_drivers(x, ref, wname, mode, dt, what)
    e = band_err(back, x)
    print("round trip %.3e" % e)
    assert e <= RT[np.dtype(dt)], e


@pytest.mark.parametrize("wname", ALL72)
def test_every_bank_through_the_level_drivers(wname):
    """the (hlen - 1) x hlen x (hlen + 3) volume: every filter length of the four kernels, the folded line on z.  The forward against
    the reference's bands; the inverse against the reference's inverse OF THE BANDS THE DEVICE GAVE, within the bound of a level: a round
    trip to the input would also measure how well the bank itself reconstructs, which the table's sym banks do only to about 1e-11 on
    these volumes (the float64 reference alone: sym3 2.5e-11, sym20 6.4e-11)."""
    h, taps = R3.bank(wname)
    shape = (h - 1, h, h + 3)
    worst = {}
    for dt in DTYPES:
        dt = np.dtype(dt)
        for mode in ("symmetric", "zero"):
            x, ref = _ref(shape, wname, 1, mode, dt.name)
            e, got, back = _one_level_through_the_drivers(x, ref, wname, mode, dt, "%s %s %s %s" % (wname, shape, mode, dt.name))
            ei = band_err(back, R3.idwt3({k: g.astype(np.float64) for k, g in zip(R3.LEVEL_KEYS, got)}, shape, taps))
            assert ei <= FWD[dt], (mode, dt, ei)
            worst[dt.name] = max(worst.get(dt.name, 0.0), e, ei)
    print("%s (%d taps): %s" % (wname, h, worst))


# ---- forward and round trip of the class --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape,wname,levels,mode", CLASS_RUNS, ids=[_id(r) for r in CLASS_RUNS])
def test_forward_every_band_and_round_trip(shape, wname, levels, mode, kind, dt):
    """every case of the table with each of the three inputs, in both precisions"""
    x, ref = _ref(shape, wname, levels, mode, np.dtype(dt).name, kind)
    W = BoundaryWavelets3D(x, wname, levels, mode)
    assert W.state == W_INIT and W.dtype == np.dtype(dt) and W.levels == levels and W.mode == mode and W.nbands == 7 * levels + 1
    F = W.info.hlen
    assert [W.coeff_shape(k) for k in range(W.nbands)] == R3.band_shapes(shape, F, levels)
    assert W.band_index(1, "ddd") == 7 * levels and W.band_index(levels, "aad") == 1
    W.forward()
    assert W.state == W_FORWARD
    got = W.coeffs
    _check_bands(got, ref, FWD[np.dtype(dt)], "%s %s L%d %s %s %s" % (shape, wname, levels, mode, kind, np.dtype(dt).name))
    assert _same_bits(W.get_image(), x)  # forward() leaves the volume bit-unchanged
    W.set_image(np.zeros(shape, dt))  # the reconstruction must come from the bands, not from what the volume still held
    assert W.state == W_INIT
    W.inverse()
    assert W.state == W_INVERSE
    e = band_err(W.get_image(), x)
    print("round trip %.3e" % e)
    assert e <= RT[np.dtype(dt)], e
    assert all(_same_bits(a, b) for a, b in zip(_raw_bands(W), got))  # inverse() leaves the bands bit-unchanged


def test_the_modes_differ_on_the_ramp_and_only_near_the_faces():
    shape, wname, F = (16, 16, 16), "db2", 4
    got = {}
    for mode in R3.MODES:
        W = BoundaryWavelets3D(R3.make_input(shape, np.float64, "ramp"), wname, 1, mode)
        W.forward()
        got[mode] = W.coeffs
    lo, hi = (F - 2) // 2, (shape[0] - 2) // 2 + 1  # positions whose window 2i + 1 - k lies inside 0 .. n-1
    for a in range(5):
        for b in range(a + 1, 5):
            ga, gb = got[R3.MODES[a]], got[R3.MODES[b]]
            assert any(not np.array_equal(u, v) for u, v in zip(ga, gb)), (R3.MODES[a], R3.MODES[b])
            for u, v in zip(ga, gb):
                assert np.array_equal(u[lo:hi, lo:hi, lo:hi], v[lo:hi, lo:hi, lo:hi])


# ---- the inverse alone ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape,wname,levels", [c[:3] for c in R3.CASES if c[0] not in R3.DRIVER_CASES],
                         ids=["%dx%dx%d-%s" % (c[0] + (c[1],)) for c in R3.CASES if c[0] not in R3.DRIVER_CASES])
def test_inverse_from_bands_written_with_set_coeff(shape, wname, levels, dt):
    """random bands (not the transform of any volume), against the reference inverse: tests the inverse without the forward"""
    F, _ = R3.bank(wname)
    rs = np.random.RandomState(9)
    bands = [rs.uniform(-100, 100, s).astype(dt) for s in R3.band_shapes(shape, F, levels)]
    want = R3.waverec3(bands, shape, wname, np.float64)
    W = BoundaryWavelets3D(np.zeros(shape, dt), wname, levels, "symmetric")
    assert W.levels == levels
    for k, b in enumerate(bands):
        W.set_coeff(b, k)
    assert W.state == W_INIT and all(_same_bits(a, b) for a, b in zip(W.coeffs, bands))
    W.inverse()
    e = band_err(W.get_image(), want)
    print("%s %s L%d %s: inverse of random bands %.3e" % (shape, wname, levels, np.dtype(dt).name, e))
    assert e <= FWD[np.dtype(dt)], e
    assert all(_same_bits(a, b) for a, b in zip(_raw_bands(W), bands))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape,wname", [((7, 7, 7), "db4"), ((40, 48, 40), "db20")])
def test_inverse_level_driver_from_random_bands(shape, wname, dt):
    dt = np.dtype(dt)
    L, sfx, f, h = _bank(wname, dt)
    bshape = tuple((n + h - 1) // 2 for n in shape)
    rs = np.random.RandomState(9)
    bands = [rs.uniform(-100, 100, bshape).astype(dt) for _ in range(8)]
    _, taps = R3.bank(wname)
    want = R3.idwt3({k: b.astype(np.float64) for k, b in zip(R3.LEVEL_KEYS, bands)}, shape, taps)
    with _Dev() as D:
        b = [D.put(v) for v in bands]
        tmp = D.put(np.full(L.pdwt_ext3d_tmp_elems(*shape, h), np.nan, dt))
        dst = D.put(np.full(shape, np.nan, dt))
        assert getattr(L, "pdwt_ext3d_inverse_level_" + sfx)(dst, (C.c_void_p * 8)(*b), *shape, C.byref(f), tmp) == 0
        e = band_err(D.get(dst, shape, dt), want)
        assert all(_same_bits(D.get(p, bshape, dt), v) for p, v in zip(b, bands))
    print("%s %s %s: inverse level of random bands %.3e" % (shape, wname, dt.name, e))
    assert e <= FWD[dt], e


# ---- thresholds, norms, statistics ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("kind,app", [("soft", 0), ("hard", 0), ("soft", 1), ("hard", 1)])
def test_thresholds_touch_exactly_the_bands_they_should(kind, app, dt):
    x = R3.make_input((40, 24, 24), dt)
    W = BoundaryWavelets3D(x, "db2", 2, "symmetric")
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
    betas = [-1.0, 5.0, -1.0, 7.0, -1.0, -1.0, 0.0, 2.0, -1.0, 11.0, -1.0, 0.5, -1.0, -1.0, 3.0]
    W.threshold_bands(betas, kind)
    for k, (b, a) in enumerate(zip(after, W.coeffs)):
        assert _same_bits(a, ref_threshold(b, betas[k], kind)), k


@pytest.mark.parametrize("dt", DTYPES)
def test_norm1_statistics_sigma_and_denoise_on_the_reference_bands(dt):
    """the reference's bands written with set_coeff, so that the statistics are those of tests/refstats.py on known data"""
    shape, wname, levels = (30, 32, 36), "db4", 2
    rs = np.random.RandomState(7)
    x = (rs.standard_normal(shape) * 3 + rs.uniform(-1, 1, shape).cumsum(axis=-1)).astype(dt)
    bands = [b.astype(dt) for b in R3.wavedec3(x, wname, levels, "symmetric", np.float64)]
    stats = [ref_stats(b) for b in bands]

    def fresh():
        W = BoundaryWavelets3D(x, wname, levels, "symmetric")
        W.forward()
        for k, b in enumerate(bands):
            W.set_coeff(b, k)
        assert W.state == W_FORWARD
        return W

    W = fresh()
    assert W.nbands == 15
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
    finest = W.band_index(1, "ddd")
    assert finest == 14
    sigma = stats[finest]["median_abs"] / MAD_SCALE  # the finest diagonal band: ddd of level 1
    assert W.estimate_sigma() == sigma
    for method in ("visu", "bayes"):
        for kind in ("soft", "hard"):
            for given in (None, 0.8):
                W = fresh()
                r = W.denoise(method, sigma=given, kind=kind)
                s_used = sigma if given is None else given
                assert r["sigma"] == s_used
                betas = r["betas"]
                assert betas.dtype == np.dtype(dt) and betas.shape == (15,) and betas[0] == -1
                wantb = ref_betas(stats, s_used, method, float(shape[0] * shape[1] * shape[2]))
                rel = np.abs(betas[1:].astype(np.float64) - wantb[1:]) / np.abs(wantb[1:])
                assert rel.max() <= (1e-6 if dt == np.float32 else 1e-10), (method, kind, rel.max())
                for k, (b, a) in enumerate(zip(bands, W.coeffs)):
                    assert _same_bits(a, ref_threshold(b, betas[k], kind)), (method, kind, k)
                assert W.state == W_FORWARD


# ---- state machine and errors ----------------------------------------------------------------------------------------------------------
def test_state_machine_refusals_leave_the_data_alone():
    x = R3.make_input((16, 16, 16), np.float32)
    W = BoundaryWavelets3D(x, "db2", 2)
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
        W.coeff_shape(15)
    with pytest.raises(IndexError):
        W.coeff_view(-1)
    with pytest.raises(IndexError):
        W.band_index(3, "ddd")
    with pytest.raises(ValueError):
        W.threshold_bands([1.0] * (W.nbands - 1))
    with pytest.raises(ValueError):
        W.denoise("sure")
    with pytest.raises(ValueError):
        W.set_coeff(np.zeros((3, 3, 3), np.float32), 1)
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
    x = R3.make_input((16, 16, 16), np.float32)
    assert BoundaryWavelets3D(x, "nosuchwavelet", 2).state == W_CREATION_ERROR
    assert BoundaryWavelets3D(x, "db2", 2, mode=5).state == W_CREATION_ERROR
    for shape in ((6, 64, 64), (7, 7, 7), (16, 16, 6)):  # ilog2(6 / 7) = ilog2(7 / 7) = 0 levels
        W = BoundaryWavelets3D(R3.make_input(shape, np.float32), "db4", 2)
        assert W.state == W_CREATION_ERROR and W.nbands == 0
        W.forward()
        W.inverse()
        assert W.state == W_CREATION_ERROR
        for call in (lambda: W.get_coeff(0), lambda: W.get_image(), lambda: W.set_image(np.zeros(shape, np.float32)), lambda: W.norm1()):
            with pytest.raises((RuntimeError, IndexError)):
                call()
    with pytest.raises(ValueError):
        BoundaryWavelets3D(x, "db2", 2, mode="smooth")
    with pytest.raises(ValueError):
        BoundaryWavelets3D(x, "db2", 2, mode="periodization")
    with pytest.raises(ValueError):
        BoundaryWavelets3D(np.zeros((8, 8), np.float32), "db2", 1)
    assert BoundaryWavelets3D(R3.make_input((30, 32, 36), np.float32), "db4", 9).levels == 2  # clamped as Wavelets3D: ilog2(30 / 7)
    assert BoundaryWavelets3D(x, "db2", 0).levels == 1


@pytest.mark.parametrize("dt", DTYPES)
def test_device_tensors_and_zero_copy_views(dt):
    import torch
    shape = (9, 33, 47)
    x = R3.make_input(shape, dt)
    t = torch.as_tensor(x, device="cuda")
    W = BoundaryWavelets3D(t, "db2", 1, "reflect")
    H = BoundaryWavelets3D(x, "db2", 1, "reflect")
    assert W.dtype == np.dtype(dt) and W.shape == shape and W.mode == "reflect"
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
        BoundaryWavelets3D(t, "db2", 1, dtype=np.float64 if dt == np.float32 else np.float32)


# ---- the point of the feature -----------------------------------------------------------------------------------------------------------
def _soft(v, beta):
    return np.copysign(np.maximum(np.abs(v) - beta, 0.0), v)


@pytest.mark.parametrize("dt", DTYPES)
def test_a_step_along_z_does_not_ghost_onto_the_first_plane(dt):
    """A 64 x 32 x 32 volume, 0 for z < 32 and 100 for z >= 32, soft-thresholded at beta = 5 with db4 L2.  Periodised, the transform sees
    a second step between the last plane and the first, and the threshold rings around it: Wavelets3D moves plane 0 by more than 1 (the
    float64 references: 3.11).  With `symmetric` plane 0 of the result is exactly 0 -- every coefficient it is built from is a sum of
    zeros -- and the last plane stays within the round-trip bound of 100."""
    beta = 5.0
    x = np.zeros((64, 32, 32), dt)
    x[32:] = 100.0
    W = BoundaryWavelets3D(x, "db4", 2, "symmetric")
    assert W.levels == 2
    W.forward()
    W.soft_threshold(beta)
    W.inverse()
    got = W.get_image()
    bands = R3.wavedec3(x, "db4", 2, "symmetric", np.float64)
    want = R3.waverec3([bands[0]] + [_soft(b, beta) for b in bands[1:]], x.shape, "db4", np.float64)
    assert np.abs(want[0]).max() == 0.0  # the reference: plane 0 does not feel the step
    e_last = np.abs(got[-1].astype(np.float64) - 100.0).max() / 100.0
    print("%s: max |plane 0| %.3e, last plane off 100 by %.3e (relative), volume err %.3e" % (np.dtype(dt).name, np.abs(got[0]).max(), e_last, band_err(got, want)))
    assert np.abs(got[0]).max() == 0.0
    assert e_last <= RT[np.dtype(dt)], e_last
    P = Wavelets3D(x, "db4", 2)
    P.forward()
    P.soft_threshold(beta)
    P.inverse()
    ghost = np.abs(P.get_image()[0]).max()
    print("periodised: max |plane 0| %.3f" % ghost)
    assert ghost > 1.0
