"""BoundaryImageBatch (the batched 2-D DWT with signal-extension boundary modes, dwt_ext2db.hip) on the GPU against tests/refext.py, the
float64 numpy reference applied per image, and, bit for bit, against a loop over BoundaryWavelets2D instances and against the level
drivers chained by hand.

Metric and bounds: those of tests/test_ext2d_gpu.py -- tests/helpers.band_err per band of every image, 1e-5 (float32) and 1e-12 (float64)
for a band and for the inverse of random bands, 10x those for a round trip back to the image (sym8 round trips sit at the bank's own
8.7e-13 in float64).  Inputs: seeded standard-normal images plus the wrapped ramp ((3x + 5y) mod 17) - 8 of that file (a plain ramp has
zero detail bands under the mirror modes and cannot carry a band-normalised bound).

Every case asserts the `fused` value the plan predicts, so both kernel forms are tested: the one-launch kernels (below and above the
64 KiB LDS opt-in) and the per-level tile kernels."""
import ctypes as C
import functools

import numpy as np
import pytest

import pdwt_amd
from pdwt_amd import BoundaryImageBatch, BoundaryWavelets2D, DeviceArray
from pdwt_amd import _native as nat
from pdwt_amd.wavelets import W_CREATION_ERROR, W_FORWARD, W_INIT, W_INVERSE
from tests import refext as R
from tests.helpers import TOL, band_err
from tests.refstats import MAD_SCALE, ref_betas, ref_stats, ref_threshold

pytestmark = pytest.mark.gpu

FWD = {np.dtype(np.float32): 1e-5, np.dtype(np.float64): 1e-12}
RT = {k: 10 * v for k, v in FWD.items()}
SUM_TOL = TOL[np.dtype(np.float64)]  # sums accumulated in double (tests/test_batch_stats_gpu.py)
DTYPES = [np.float32, np.float64]
ALL = R.MODES

# (B, Nr, Nc, bank, levels, modes, fused in float32, fused in float64)
CASES = [
    (3, 37, 51, "db3", 2, ALL, True, True),
    (2, 9, 7, "haar", 2, ALL, True, True),
    (5, 64, 64, "db4", 3, ("symmetric",), True, True),
    (2, 128, 128, "db4", 3, ("reflect",), True, False),   # float32 fused above the opt-in; float64 per level
    (2, 61, 67, "sym8", 2, ("constant",), True, True),
    (2, 78, 80, "db20", 1, ("periodic",), True, True),
    (2, 160, 200, "db4", 3, ("symmetric",), False, False),  # per level
    (2, 156, 160, "db20", 2, ("zero",), False, False),      # per level, 40 taps
]
RUNS = [c[:5] + (m,) + c[6:] for c in CASES for m in c[5]]
IDS = ["%dx%dx%d-%s-L%d-%s" % r[:6] for r in RUNS]


def _images(B, Nr, Nc, dt):
    """standard-normal images plus the wrapped ramp of tests/test_ext2d_gpu.py"""
    yy, xx = np.mgrid[0:Nr, 0:Nc]
    return (np.random.RandomState(B * 1000 + Nr).standard_normal((B, Nr, Nc)) + ((3 * xx + 5 * yy) % 17 - 8.0)).astype(dt)


@functools.lru_cache(maxsize=None)
def _ref(B, Nr, Nc, wname, levels, mode, dtname):
    """(the batch in the dtype under test, per image the float64 reference bands): computed once per case and shared, read-only"""
    x = _images(B, Nr, Nc, np.dtype(dtname))
    x.setflags(write=False)
    refs = [R.wavedec2(x[b], wname, levels, mode, np.float64) for b in range(B)]
    for bands in refs:
        for a in bands:
            a.setflags(write=False)
    return x, refs


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _raw_bands(W):
    """every band stack read straight from device memory, whatever the state"""
    W.sync()
    return [DeviceArray(W, W.coeff_int_ptr(k), W.coeff_shape(k), W.dtype).numpy() for k in range(W.nbands)]


def _plan(Nr, Nc, wname, levels, dt):
    F, _ = R.bank(wname)
    return bool(pdwt_amd.hip().pdwt_ext2db_fused(Nr, Nc, F, levels, np.dtype(dt).itemsize))


def _expect_fused(run, dt):
    B, Nr, Nc, wname, levels, mode, f32, f64 = run
    want = f32 if np.dtype(dt) == np.float32 else f64
    assert _plan(Nr, Nc, wname, levels, dt) == want, "the plan is not on the documented side"
    return want


# ---- forward, round trip, the twins -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("run", RUNS, ids=IDS)
def test_forward_round_trip_and_the_per_image_class(run, dt):
    B, Nr, Nc, wname, levels, mode = run[:6]
    x, refs = _ref(B, Nr, Nc, wname, levels, mode, np.dtype(dt).name)
    W = BoundaryImageBatch(x, wname, levels, mode)
    assert W.levels == levels and W.nbands == 3 * levels + 1 and W.shape == (B, Nr, Nc) and len(W) == B and W.mode == mode
    assert W.fused == _expect_fused(run, dt)
    W.forward()
    assert W.state == W_FORWARD
    got = W.coeffs
    worst = 0.0
    for k, g in enumerate(got):
        assert g.shape == (B,) + refs[0][k].shape == W.coeff_shape(k), k
        for b in range(B):
            e = band_err(g[b], refs[b][k])
            worst = max(worst, e)
            assert e <= FWD[np.dtype(dt)], ("band", k, "image", b, e)
    assert _same_bits(W.get_image(), x)  # forward() leaves the images alone
    W.inverse()
    assert W.state == W_INVERSE
    back = W.get_image()
    e = max(band_err(back[b], x[b]) for b in range(B))
    print("%s %s fused=%s: worst band %.3e, round trip %.3e" % (IDS[RUNS.index(run)], np.dtype(dt).name, W.fused, worst, e))
    assert e <= RT[np.dtype(dt)], e
    assert all(_same_bits(a, g) for a, g in zip(_raw_bands(W), got))  # inverse() leaves the bands alone
    # a loop over BoundaryWavelets2D instances: the same bits, bands and reconstruction
    for b in range(B):
        T = BoundaryWavelets2D(x[b], wname, levels, mode)
        T.forward()
        for k, t in enumerate(T.coeffs):
            assert np.array_equal(got[k][b], t), ("band", k, "image", b)
        T.inverse()
        assert np.array_equal(back[b], T.get_image()), b


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("case", CASES, ids=["%dx%dx%d-%s-L%d" % c[:5] for c in CASES])
def test_inverse_alone_from_random_bands(case, dt):
    """random bands (not the transform of any image) written with set_coeff, against the reference inverse and the per-image class"""
    B, Nr, Nc, wname, levels = case[:5]
    F, _ = R.bank(wname)
    rs = np.random.RandomState(9)
    bands = [rs.standard_normal((B,) + s).astype(dt) for s in R.band_shapes((Nr, Nc), F, levels)]
    W = BoundaryImageBatch(np.zeros((B, Nr, Nc), dt), wname, levels, "symmetric")
    assert W.levels == levels and W.fused == _expect_fused(case[:5] + ("symmetric",) + case[6:], dt)
    for k, a in enumerate(bands):
        W.set_coeff(a, k)
    assert W.state == W_INIT and all(_same_bits(a, g) for a, g in zip(W.coeffs, bands))
    W.inverse()
    got = W.get_image()
    for b in range(B):
        want = R.waverec2([a[b] for a in bands], (Nr, Nc), wname, np.float64)
        e = band_err(got[b], want)
        assert e <= FWD[np.dtype(dt)], (b, e)
        T = BoundaryWavelets2D(np.zeros((Nr, Nc), dt), wname, levels, "symmetric")
        for k, a in enumerate(bands):
            T.set_coeff(a[b], k)
        T.inverse()
        assert np.array_equal(got[b], T.get_image()), b
    assert all(_same_bits(a, g) for a, g in zip(_raw_bands(W), bands))


# ---- the fused class against the level drivers chained by hand ----------------------------------------------------------------------------
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


FUSED_RUNS = [(r, dt) for r in RUNS for dt in DTYPES if (r[6] if dt == np.float32 else r[7]) and r[5] in ("symmetric", "reflect", "constant", "periodic", "zero")]


@pytest.mark.parametrize("run,dt", FUSED_RUNS, ids=["%s-%s" % (IDS[RUNS.index(r)], np.dtype(d).name) for r, d in FUSED_RUNS])
def test_fused_class_equals_the_level_drivers_chained_by_hand(run, dt):
    B, Nr, Nc, wname, levels, mode = run[:6]
    x, _ = _ref(B, Nr, Nc, wname, levels, mode, np.dtype(dt).name)
    W = BoundaryImageBatch(x, wname, levels, mode)
    assert W.fused
    W.forward()
    got = W.coeffs
    W.inverse()
    back = W.get_image()
    L, sfx, f, h = _bank(wname, dt)
    shapes = R.level_shapes((Nr, Nc), h, levels)
    fwd, inv = getattr(L, "pdwt_ext2db_forward_level_" + sfx), getattr(L, "pdwt_ext2db_inverse_level_" + sfx)
    with _Dev() as D:
        src = D.put(x)
        approx, det = [src], []
        for l in range(1, levels + 1):
            hr, hc = shapes[l]
            q = [D.put(np.full((B, hr, hc), np.nan, dt)) for _ in range(4)]
            assert fwd(approx[-1], q[0], q[1], q[2], q[3], B, shapes[l - 1][0], shapes[l - 1][1], R.MODES.index(mode), C.byref(f)) == 0
            approx.append(q[0])
            det.append(q[1:])
        assert np.array_equal(D.get(approx[levels], (B,) + shapes[levels], dt), got[0])
        for l in range(1, levels + 1):
            for j in range(3):
                assert np.array_equal(D.get(det[l - 1][j], (B,) + shapes[l], dt), got[3 * (l - 1) + 1 + j]), (l, j)
        cur = approx[levels]
        for l in range(levels, 0, -1):
            out = D.put(np.full((B,) + shapes[l - 1], np.nan, dt))
            assert inv(out, cur, det[l - 1][0], det[l - 1][1], det[l - 1][2], B, shapes[l - 1][0], shapes[l - 1][1], C.byref(f)) == 0
            cur = out
        assert np.array_equal(D.get(cur, (B, Nr, Nc), dt), back)


# ---- the batch is B independent images ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape,wname,levels", [((1, 37, 51), "db3", 2), ((1, 160, 200), "db4", 3)], ids=["fused", "levels"])
def test_a_batch_of_one_is_the_2d_class(shape, wname, levels, dt):
    x = _images(*shape, dt)
    W, T = BoundaryImageBatch(x, wname, levels, "reflect"), BoundaryWavelets2D(x[0], wname, levels, "reflect")
    W.forward()
    T.forward()
    for a, t in zip(W.coeffs, T.coeffs):
        assert np.array_equal(a[0], t)
    W.inverse()
    T.inverse()
    assert np.array_equal(W.get_image()[0], T.get_image())


@pytest.mark.parametrize("shape,wname,levels", [((4, 37, 51), "db3", 2), ((3, 160, 200), "db4", 2)], ids=["fused", "levels"])
def test_replacing_one_image_changes_only_its_slices(shape, wname, levels):
    x = _images(*shape, np.float32)
    W = BoundaryImageBatch(x, wname, levels, "symmetric")
    W.forward()
    first = W.coeffs
    y = x.copy()
    y[2] = _images(1, shape[1], shape[2], np.float32)[0][::-1]
    W.set_image(y)
    assert W.state == W_INIT
    W.forward()
    for k, (a, c) in enumerate(zip(first, W.coeffs)):
        for b in range(shape[0]):
            assert _same_bits(a[b], c[b]) == (b != 2), (k, b)


# ---- thresholds, norms, statistics --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("kind,app", [("soft", 0), ("hard", 1)])
def test_uniform_thresholds_and_the_pooled_norm(kind, app, dt):
    x = _images(3, 61, 67, dt)
    W = BoundaryImageBatch(x, "db4", 2, "symmetric")
    W.forward()
    before = W.coeffs
    getattr(W, kind + "_threshold")(1.5, do_thresh_appcoeffs=app)
    after = W.coeffs
    for k, (b, a) in enumerate(zip(before, after)):
        if k == 0 and not app:
            assert _same_bits(a, b)
        else:
            assert _same_bits(a, ref_threshold(b, 1.5, kind)) and not _same_bits(a, b), k
    want = sum(np.abs(a.astype(np.float64)).sum() for a in after)
    assert abs(W.pooled_norm1() - want) <= SUM_TOL * want
    per = W.norm1()
    assert per.shape == (3,) and abs(per.sum() - want) <= SUM_TOL * want
    # the pooled statistics see a stack as one band: D1 of all images together
    assert W.pooled_estimate_sigma() == ref_stats(after[3])["median_abs"] / MAD_SCALE
    assert W.band_stats(3)["n"] == after[3].size and len(W.pooled_all_band_stats()) == W.nbands


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape,wname,levels", [((4, 61, 67), "db4", 2), ((3, 160, 200), "db2", 2)], ids=["fused", "levels"])
def test_per_image_statistics_sigma_thresholds_and_denoise(shape, wname, levels, dt):
    B, Nr, Nc = shape
    rs = np.random.RandomState(7)
    x = (rs.standard_normal(shape) * np.arange(1, B + 1)[:, None, None] + rs.uniform(-1, 1, shape).cumsum(axis=-1)).astype(dt)

    def fresh():
        W = BoundaryImageBatch(x, wname, levels, "symmetric")
        W.forward()
        return W

    W = fresh()
    nb = W.nbands
    bands = W.coeffs
    stats = [[ref_stats(a[b]) for a in bands] for b in range(B)]
    for with_median in (False, True):
        st = W.all_band_stats(with_median=with_median)
        for key in ("n", "sum_abs", "sum_sq", "max_abs", "median_abs"):
            assert st[key].shape == (B, nb) and st[key].dtype == np.float64
        for b in range(B):
            for k in range(nb):
                s = stats[b][k]
                assert st["n"][b, k] == s["n"] and st["max_abs"][b, k] == s["max_abs"], (b, k)
                assert abs(st["sum_abs"][b, k] - s["sum_abs"]) <= SUM_TOL * s["sum_abs"] and abs(st["sum_sq"][b, k] - s["sum_sq"]) <= SUM_TOL * s["sum_sq"]
                if with_median:
                    assert st["median_abs"][b, k] == s["median_abs"], (b, k)
                else:
                    assert np.isnan(st["median_abs"][b, k])
    sigma = W.estimate_sigma()
    norm = W.norm1()
    twins = []
    for b in range(B):
        assert sigma[b] == stats[b][3]["median_abs"] / MAD_SCALE, b
        want = sum(s["sum_abs"] for s in stats[b])
        assert abs(norm[b] - want) <= SUM_TOL * want, b
        T = BoundaryWavelets2D(x[b], wname, levels, "symmetric")
        T.forward()
        assert sigma[b] == T.estimate_sigma()
        twins.append(T)
    assert (np.diff(sigma) > 0).all()  # every image its own noise level
    # threshold_bands: per image and broadcast, negative betas leave a band alone
    betas = rs.uniform(0.0, 2.0, (B, nb))
    betas[rs.uniform(size=betas.shape) < 0.3] = -1.0
    betas[:, 0], betas[:, 1] = -0.5, 0.0
    for kind in ("soft", "hard"):
        for form in (betas, betas[1]):
            W = fresh()
            W.threshold_bands(form, kind)
            full = np.broadcast_to(form, (B, nb)).astype(dt)
            for k, (old, new) in enumerate(zip(bands, W.coeffs)):
                for b in range(B):
                    assert _same_bits(new[b], ref_threshold(old[b], full[b, k], kind)), (kind, b, k)
            assert W.state == W_FORWARD
    # denoise: per-image sigma, the rule of bandstats_host.hpp
    tol = 1e-6 if dt == np.float32 else 1e-10
    for method in ("visu", "bayes"):
        for kind in ("soft", "hard"):
            for given in (None, 0.8, np.linspace(0.5, 1.5, B)):
                W = fresh()
                r = W.denoise(method, sigma=given, kind=kind)
                bt = r["betas"]
                assert bt.dtype == np.dtype(dt) and bt.shape == (B, nb) and (bt[:, 0] == -1).all()
                after = W.coeffs
                for b in range(B):
                    s_used = sigma[b] if given is None else float(np.broadcast_to(given, (B,))[b])
                    assert r["sigma"][b] == s_used
                    want = ref_betas(stats[b], s_used, method, float(Nr * Nc))
                    rel = np.abs(bt[b, 1:].astype(np.float64) - want[1:]) / np.abs(want[1:])
                    assert rel.max() <= tol, (method, b, rel.max())
                    for k in range(nb):
                        assert _same_bits(after[k][b], ref_threshold(bands[k][b], bt[b, k], kind)), (method, kind, b, k)
                    if method == "visu" and kind == "soft":  # VisuShrink betas equal those of the per-image class bit for bit
                        T = BoundaryWavelets2D(x[b], wname, levels, "symmetric")
                        T.forward()
                        t = T.denoise("visu", sigma=None if given is None else s_used, kind=kind)
                        assert _same_bits(t["betas"], bt[b]) and t["sigma"] == r["sigma"][b]
                assert W.state == W_FORWARD


# ---- state machine and errors -------------------------------------------------------------------------------------------------------------
def test_state_machine_refusals_leave_the_data_alone():
    x = _images(3, 64, 64, np.float32)
    W = BoundaryImageBatch(x, "db2", 3)
    assert W.mode == "symmetric" and W.fused

    def all_refuse(stats_only):
        calls = [lambda: W.band_stats(1), lambda: W.all_band_stats(), lambda: W.estimate_sigma(), lambda: W.threshold_bands([1.0] * W.nbands),
                 lambda: W.denoise("bayes"), lambda: W.denoise("visu", sigma=1.0), lambda: W.pooled_all_band_stats(), lambda: W.pooled_estimate_sigma(),
                 lambda: W.pooled_threshold_bands([1.0] * W.nbands), lambda: W.pooled_denoise("bayes")]
        if not stats_only:
            calls += [lambda: W.get_coeff(0), lambda: W.coeffs, lambda: W.soft_threshold(1.0), lambda: W.hard_threshold(1.0), lambda: W.norm1(),
                      lambda: W.pooled_norm1()]
        for call in calls:
            with pytest.raises(RuntimeError):
                call()

    all_refuse(stats_only=True)  # before forward(): the statistics need the coefficients of a forward()
    assert W.norm1().shape == (3,)  # (readable: zeros)
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
        W.threshold_bands(np.ones((2, W.nbands)))
    with pytest.raises(ValueError):
        W.denoise("sure")
    with pytest.raises(ValueError):
        W.denoise("visu", sigma=[1.0, 2.0])
    with pytest.raises(ValueError):
        W.denoise("visu", sigma=-1.0)
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
    assert W.state == W_FORWARD and (W.estimate_sigma() >= 0).all()


def test_creation_errors_and_bad_arguments():
    x = _images(2, 64, 64, np.float32)
    assert BoundaryImageBatch(x, "nosuchwavelet", 2).state == W_CREATION_ERROR
    assert BoundaryImageBatch(x, "db2", 2, mode=5).state == W_CREATION_ERROR
    for shape in ((2, 6, 64), (2, 7, 7)):  # ilog2(6 / 7) = ilog2(7 / 7) = 0 levels
        W = BoundaryImageBatch(np.zeros(shape, np.float32), "db4", 2)
        assert W.state == W_CREATION_ERROR and W.nbands == 0 and not W.fused
        W.forward()
        W.inverse()
        assert W.state == W_CREATION_ERROR
        for call in (lambda: W.get_coeff(0), lambda: W.get_image(), lambda: W.set_image(np.zeros(shape, np.float32)), lambda: W.norm1(),
                     lambda: W.pooled_norm1(), lambda: W.all_band_stats(), lambda: W.estimate_sigma(), lambda: W.denoise("visu")):
            with pytest.raises((RuntimeError, IndexError)):
                call()
    with pytest.raises(ValueError):
        BoundaryImageBatch(x, "db2", 2, mode="smooth")
    with pytest.raises(ValueError):
        BoundaryImageBatch(x[0], "db2", 1)
    assert BoundaryImageBatch(_images(2, 96, 80, np.float32), "db4", 9).levels == 3  # clamped as BoundaryWavelets2D
    assert BoundaryImageBatch(x, "db2", 0).levels == 1


@pytest.mark.parametrize("dt", DTYPES)
def test_device_tensors_and_zero_copy_views(dt):
    import torch
    x = _images(3, 61, 67, dt)
    t = torch.as_tensor(x, device="cuda")
    W = BoundaryImageBatch(t, "db2", 2, "reflect")
    H = BoundaryImageBatch(x, "db2", 2, "reflect")
    assert W.dtype == np.dtype(dt) and W.shape == (3, 61, 67) and W.mode == "reflect"
    W.forward()
    H.forward()
    assert all(_same_bits(a, b) for a, b in zip(W.coeffs, H.coeffs))
    v = W.coeff_view(3)
    assert v.ptr == W.coeff_int_ptr(3) and v.shape == W.coeff_shape(3) == (3, 32, 35) and v.ptr % 256 == 0
    assert W.image_view().ptr == W.image_int_ptr() and _same_bits(W.image_view().numpy(), x)
    W.sync()
    tv = torch.as_tensor(v, device="cuda")
    assert tv.data_ptr() == v.ptr and np.array_equal(tv.cpu().numpy(), W.get_coeff(3))
    tv[1].zero_()  # a write through the view lands in the slice of image 1
    torch.cuda.synchronize()
    c = W.get_coeff(3)
    assert not c[1].any() and _same_bits(c[0], H.get_coeff(3)[0]) and _same_bits(c[2], H.get_coeff(3)[2])
    W.set_coeff(torch.as_tensor(H.get_coeff(3), device="cuda"), 3)
    assert _same_bits(W.get_coeff(3), H.get_coeff(3)) and W.state == W_FORWARD
    W.set_image(torch.as_tensor(x[::-1].copy(), device="cuda"))
    assert np.array_equal(W.get_image(), x[::-1]) and W.state == W_INIT
    with pytest.raises(TypeError):
        BoundaryImageBatch(t, "db2", 2, dtype=np.float64 if dt == np.float32 else np.float32)
