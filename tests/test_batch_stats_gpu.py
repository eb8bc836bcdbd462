"""GPU tests of the batched band statistics and noise-adaptive thresholds of ImageBatch (bandbatch.hip; all_band_stats /
estimate_sigma / threshold_bands / denoise / norm1 of WaveletsImages) against (a) the numpy restatement of tests/refstats.py on
the downloaded bands, with the tolerances of test_bandstats_gpu.py: n, max and median EQUAL, sums to 1e-10 relative; (b) the
single-image path on a twin ``Wavelets`` per image: median, max and sigma bit for bit, VisuShrink betas bit for bit."""
import numpy as np
import pytest

import pdwt_amd
from tests.helpers import TOL
from tests.refstats import MAD_SCALE, ref_betas, ref_stats, ref_threshold

pytestmark = pytest.mark.gpu

SUM_TOL = TOL[np.dtype(np.float64)]
DTYPES = [np.float32, np.float64]
KEYS = ("n", "sum_abs", "sum_sq", "max_abs", "median_abs")


def _rel(a, b):
    if np.isinf(b) or np.isinf(a):
        return 0.0 if a == b else np.inf
    return abs(a - b) / (abs(b) if b != 0 else 1.0)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _bits(x):
    return np.float64(x).tobytes()


def _check_band(got, band, with_median, what):
    ref = ref_stats(band)
    assert got["n"] == ref["n"], what
    assert got["max_abs"] == ref["max_abs"], what
    if with_median:
        assert got["median_abs"] == ref["median_abs"] and not np.signbit(got["median_abs"]), (what, got["median_abs"], ref["median_abs"])
    else:
        assert np.isnan(got["median_abs"]), what
    ra, rq = _rel(got["sum_abs"], ref["sum_abs"]), _rel(got["sum_sq"], ref["sum_sq"])
    assert ra <= SUM_TOL and rq <= SUM_TOL, (what, ra, rq)
    return max(ra, rq)


def _images(B, Nr, Nc, dtype, seed=7):
    rs = np.random.RandomState(seed)
    return (rs.standard_normal((B, Nr, Nc)) * 3 + rs.uniform(-1, 1, (B, Nr, Nc)).cumsum(axis=-1)).astype(dtype)


def _twin(x, wname, L, swt):
    T = pdwt_amd.Wavelets(x, wname, L, do_swt=swt)
    T.forward()
    return T


def _at(st, b, k):
    return {key: float(st[key][b, k]) for key in KEYS}


# (B, Nr, Nc, wname, levels, do_swt)
CASES = [(64, 512, 512, "db4", 3, 0), (3, 250, 371, "haar", 3, 0), (5, 256, 384, "db7", 2, 0), (4, 192, 320, "db4", 2, 1),
         (3, 2048, 2048, "db4", 2, 0), (1, 128, 128, "db2", 2, 0)]
IDS = ["%dx%dx%d-%s-L%d%s" % (c[0], c[1], c[2], c[3], c[4], "-swt" if c[5] else "") for c in CASES]


# ---- 1. the statistics: numpy, the single-image path, two runs -----------------------------------------------------
@pytest.mark.parametrize("with_median", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_statistics_against_numpy_and_the_single_image_path(case, dtype, with_median):
    B, Nr, Nc, wname, L, swt = case
    x = _images(B, Nr, Nc, dtype)
    batch = pdwt_amd.ImageBatch(x, wname, L, do_swt=swt)
    batch.forward()
    nb = batch.nbands
    assert nb == 3 * L + 1 == batch[0].nbands
    st = batch.all_band_stats(with_median=with_median)
    again = batch.all_band_stats(with_median=with_median)
    assert sorted(st) == sorted(KEYS)
    for key in KEYS:
        assert st[key].shape == (B, nb) and st[key].dtype == np.float64
        assert st[key].tobytes() == again[key].tobytes(), key  # two runs, identical bits
    sigma = batch.estimate_sigma()
    norm = batch.norm1()
    assert sigma.shape == norm.shape == (B,) and sigma.dtype == norm.dtype == np.float64
    worst = 0.0
    for b in range(B):
        bands = batch[b].coeffs
        T = _twin(x[b], wname, L, swt)
        for k in range(nb):
            got = _at(st, b, k)
            worst = max(worst, _check_band(got, bands[k], with_median, "image %d band %d" % (b, k)))
            one = T.band_stats(k, with_median=with_median)
            assert _bits(got["max_abs"]) == _bits(one["max_abs"]), (b, k)
            if with_median:
                assert _bits(got["median_abs"]) == _bits(one["median_abs"]), (b, k)
        assert sigma[b] == T.estimate_sigma(), b
        assert sigma[b] == ref_stats(bands[3])["median_abs"] / MAD_SCALE, b
        want = T.norm1_f64()
        assert abs(norm[b] - want) <= SUM_TOL * abs(want), (b, norm[b], want)
    print("batched=%s worst relative error of a sum %.2e" % (batch.batched, worst))


# ---- 2. every image has its own sigma ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_every_image_estimates_its_own_sigma(dtype):
    B, N = 6, 256
    g = np.mgrid[0:N, 0:N] / N
    clean = np.sin(6 * g[0]) * np.cos(4 * g[1]) + 0.5 * (g[0] > 0.5)
    rs = np.random.RandomState(3)
    x = np.stack([clean + (b + 1) * rs.standard_normal((N, N)) for b in range(B)]).astype(dtype)
    batch = pdwt_amd.ImageBatch(x, "db4", 3)
    batch.forward()
    sigma = batch.estimate_sigma()
    twins = [_twin(x[b], "db4", 3, 0) for b in range(B)]
    for b in range(B):
        assert sigma[b] == twins[b].estimate_sigma()
        assert abs(sigma[b] / (b + 1) - 1) <= 0.05, (b, sigma[b])
    assert (np.diff(sigma) > 0).all()
    for method in ("visu", "bayes"):
        fresh = pdwt_amd.ImageBatch(x, "db4", 3)
        fresh.forward()
        r = fresh.denoise(method)
        assert _same_bits(r["sigma"], sigma)
        assert r["betas"].shape == (B, fresh.nbands) and r["betas"].dtype == np.dtype(dtype)
        for b in range(1, B):
            assert (r["betas"][b, 1:] != r["betas"][b - 1, 1:]).all(), (method, b)


# ---- 3. threshold_bands ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["per_image", "broadcast"])
@pytest.mark.parametrize("kind", ["soft", "hard"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", [(5, 192, 160, "db4", 3, 0), (3, 96, 128, "db2", 2, 1), (2, 2048, 1024, "db4", 1, 0)], ids=["dwt", "swt", "large"])
def test_threshold_bands_against_numpy(case, dtype, kind, form):
    B, Nr, Nc, wname, L, swt = case
    batch = pdwt_amd.ImageBatch(_images(B, Nr, Nc, dtype, seed=11), wname, L, do_swt=swt)
    batch.forward()
    nb = batch.nbands
    before = [batch[b].coeffs for b in range(B)]
    rs = np.random.RandomState(12)
    betas = rs.uniform(0.0, 3.0, (B, nb) if form == "per_image" else (nb,))
    betas[rs.uniform(size=betas.shape) < 0.3] = -1.0
    betas[..., 0], betas[..., 1] = -0.5, 0.0
    batch.threshold_bands(betas, kind)
    full = np.broadcast_to(betas, (B, nb)).astype(dtype)
    assert (full < 0).any() and (full > 0).any()
    for b in range(B):
        assert batch[b].state == pdwt_amd.W_FORWARD
        for k, (old, new) in enumerate(zip(before[b], batch[b].coeffs)):
            assert _same_bits(new, ref_threshold(old, full[b, k], kind)), (b, k, full[b, k])
            if full[b, k] < 0:
                assert _same_bits(new, old), (b, k)


# ---- 4. denoise --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", [None, 0.8, "array"])
@pytest.mark.parametrize("kind", ["soft", "hard"])
@pytest.mark.parametrize("method", ["visu", "bayes"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", [(6, 256, 256, "db4", 3, 0), (3, 128, 96, "db2", 2, 1), (3, 250, 371, "haar", 3, 0)], ids=["dwt", "swt", "odd"])
def test_denoise_betas_bands_and_reconstruction(case, dtype, method, kind, sigma):
    B, Nr, Nc, wname, L, swt = case
    x = _images(B, Nr, Nc, dtype, seed=5)
    batch = pdwt_amd.ImageBatch(x, wname, L, do_swt=swt)
    batch.forward()
    nb = batch.nbands
    before = [batch[b].coeffs for b in range(B)]
    stats = [[ref_stats(c) for c in before[b]] for b in range(B)]
    given = np.linspace(0.5, 1.5, B) if isinstance(sigma, str) else sigma
    r = batch.denoise(method, sigma=given, kind=kind)
    betas = r["betas"]
    assert betas.dtype == np.dtype(dtype) and betas.shape == (B, nb) and (betas[:, 0] == -1).all()
    tol = 1e-6 if dtype == np.float32 else 1e-10
    for b in range(B):
        want_sigma = stats[b][3]["median_abs"] / MAD_SCALE if given is None else float(np.broadcast_to(given, (B,))[b])
        assert r["sigma"][b] == want_sigma, b
        want = ref_betas(stats[b], want_sigma, method, float(Nr * Nc))
        rel = np.abs(betas[b, 1:].astype(np.float64) - want[1:]) / np.abs(want[1:])
        assert rel.max() <= tol, (b, rel.max())
        after = batch[b].coeffs  # the view of image b sees the thresholded coefficients
        for k in range(nb):
            assert _same_bits(after[k], ref_threshold(before[b][k], betas[b, k], kind)), (b, k)
        assert _same_bits(after[0], before[b][0])
        assert batch[b].state == pdwt_amd.W_FORWARD
    # the twins: VisuShrink betas bit for bit; the reconstructions bit for bit (BayesShrink: the twin takes the batch's betas, its own
    # sums are added in another order)
    twins = [_twin(x[b], wname, L, swt) for b in range(B)]
    for b, T in enumerate(twins):
        if method == "visu":
            t = T.denoise("visu", sigma=None if given is None else float(np.broadcast_to(given, (B,))[b]), kind=kind)
            assert _same_bits(t["betas"], betas[b]), b
            assert t["sigma"] == r["sigma"][b]
        else:
            T.threshold_bands(betas[b], kind)
        T.inverse()
    batch.inverse()
    rec = batch.get_images()
    for b, T in enumerate(twins):
        assert _same_bits(rec[b], T.get_image()), b


@pytest.mark.parametrize("method", ["visu", "bayes"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_constant_image_in_the_batch(dtype, method):
    x = _images(4, 128, 128, dtype, seed=9)
    x[2] = 3.0
    batch = pdwt_amd.ImageBatch(x, "haar", 3)
    batch.forward()
    before = [batch[b].coeffs for b in range(4)]
    r = batch.denoise(method)
    assert r["sigma"][2] == 0.0 and np.isfinite(r["betas"]).all() and (r["betas"][2, 1:] == 0).all()
    for old, new in zip(before[2], batch[2].coeffs):
        assert _same_bits(old, new)
    for b in (0, 1, 3):  # the other images: as if they were alone
        T = _twin(x[b], "haar", 3, 0)
        assert r["sigma"][b] == T.estimate_sigma() > 0
        if method == "visu":
            assert _same_bits(T.denoise("visu")["betas"], r["betas"][b])
        for k, (old, new) in enumerate(zip(before[b], batch[b].coeffs)):
            assert _same_bits(new, ref_threshold(old, r["betas"][b, k], "soft")), (b, k)


# ---- 4b. more (image, band) pairs than one group holds -----------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_batch_larger_than_one_group(dtype):
    B, N, L = 900, 32, 3  # 900 x 10 pairs: the group of 8192 pairs (819 images) and a second one of 81 images
    rs = np.random.RandomState(21)
    x = (rs.standard_normal((B, N, N)) * np.linspace(0.5, 4.0, B)[:, None, None]).astype(dtype)
    batch = pdwt_amd.ImageBatch(x, "haar", L)
    batch.forward()
    nb = batch.nbands
    assert B * nb > 8192
    st = batch.all_band_stats(with_median=True)
    sigma = batch.estimate_sigma()
    norm = batch.norm1()
    before = [batch[b].coeffs for b in range(B)]
    for b in range(B):
        for k in range(nb):
            _check_band(_at(st, b, k), before[b][k], True, "image %d band %d" % (b, k))
        assert sigma[b] == ref_stats(before[b][3])["median_abs"] / MAD_SCALE, b
        want = float(sum(np.abs(c).astype(np.float64).sum() for c in before[b]))
        assert abs(norm[b] - want) <= SUM_TOL * want, b
    for b in (0, 818, 819, 820, 899):  # both sides of the group boundary against the single-image path on the same coefficients
        assert sigma[b] == batch[b].estimate_sigma(), b
    betas = rs.uniform(0.0, 2.0, (B, nb))
    betas[rs.uniform(size=betas.shape) < 0.3] = -1.0
    batch.threshold_bands(betas, "soft")
    full = betas.astype(dtype)
    for b in range(B):
        for k, (old, new) in enumerate(zip(before[b], batch[b].coeffs)):
            assert _same_bits(new, ref_threshold(old, full[b, k], "soft")), (b, k)
    fresh = pdwt_amd.ImageBatch(x, "haar", L)
    fresh.forward()
    r = fresh.denoise("visu")
    assert _same_bits(r["sigma"], sigma)
    for b in (0, 818, 819, 899):
        T = _twin(x[b], "haar", L, 0)
        assert _same_bits(T.denoise("visu")["betas"], r["betas"][b]), b
        for k, c in enumerate(fresh[b].coeffs):
            assert _same_bits(c, T.get_coeff(k)), (b, k)


# ---- 5. hard inputs in one member only ---------------------------------------------------------------------------------
def _hard_inputs(n, dtype):
    rs = np.random.RandomState(n)
    tiny = 1e-40 if dtype == np.float32 else 1e-310
    z = np.zeros(n, dtype)
    signed = np.zeros(n, dtype)
    signed[::7] = -0.0
    sparse = np.where(rs.uniform(size=n) < 0.9, 0.0, rs.standard_normal(n)).astype(dtype)
    one_inf = rs.standard_normal(n).astype(dtype)
    one_inf[n // 3] = -np.inf
    with np.errstate(under="ignore"):
        den = (rs.standard_normal(n) * tiny).astype(dtype)
    return {"zeros": z, "signed zeros": signed, "sparse": sparse, "denormal": den, "inf": one_inf, "equal": np.full(n, -0.75, dtype)}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(256, 256), (130, 126), (2048, 2048)])  # (the last: a band of 2^20 elements, selected in rounds)
def test_hard_inputs_in_one_member_only(shape, dtype):
    B, hit = 3, 1
    batch = pdwt_amd.ImageBatch(_images(B, shape[0], shape[1], dtype, seed=1), "db2", 1)
    batch.forward()
    base = batch.all_band_stats(with_median=True)
    sig0 = batch.estimate_sigma()
    bshape = batch[hit].band_shape(3)
    n = bshape[0] * bshape[1]
    for name, v in _hard_inputs(n, dtype).items():
        batch[hit].set_coeff(v.reshape(bshape), 3)  # (the band does not move: the pointer table stays valid)
        band = batch[hit].get_coeff(3)
        assert _same_bits(band, v.reshape(bshape)), name
        st = batch.all_band_stats(with_median=True)
        got = _at(st, hit, 3)
        _check_band(got, band, True, "%s n=%d" % (name, n))
        if name in ("zeros", "signed zeros"):
            assert got["median_abs"] == 0.0 and not np.signbit(got["median_abs"]) and got["max_abs"] == 0.0
        if name == "inf":
            assert np.isfinite(got["median_abs"]) and got["max_abs"] == np.inf
        if name == "equal":
            assert got["median_abs"] == 0.75 == got["max_abs"]
        sig = batch.estimate_sigma()
        assert sig[hit] == got["median_abs"] / MAD_SCALE
        for key in KEYS:  # every other (image, band) keeps its bits
            mask = np.ones(st[key].shape, bool)
            mask[hit, 3] = False
            assert st[key][mask].tobytes() == base[key][mask].tobytes(), (name, key)
        assert sig[0] == sig0[0] and sig[2] == sig0[2]
        r = batch.denoise("bayes") if name == "zeros" else None
        if r is not None:  # a member whose finest band is all zero: sigma 0, finite betas; the batch goes on
            assert r["sigma"][hit] == 0.0 and np.isfinite(r["betas"]).all()
            batch = pdwt_amd.ImageBatch(_images(B, shape[0], shape[1], dtype, seed=1), "db2", 1)
            batch.forward()


# ---- 6. state machine and errors ---------------------------------------------------------------------------------------
def _calls(batch):
    nb = batch.nbands
    return (lambda: batch.all_band_stats(), lambda: batch.all_band_stats(with_median=True), lambda: batch.estimate_sigma(),
            lambda: batch.threshold_bands([1.0] * nb), lambda: batch.denoise("bayes"), lambda: batch.denoise("visu", sigma=1.0),
            lambda: batch.norm1())


def _all_refuse(batch):
    for call in _calls(batch):
        with pytest.raises(RuntimeError):
            call()


@pytest.mark.parametrize("dtype", DTYPES)
def test_state_machine_and_errors(dtype):
    B = 3
    x = _images(B, 96, 64, dtype, seed=2)
    batch = pdwt_amd.ImageBatch(x, "db2", 2)
    _all_refuse(batch)  # before forward()
    batch.forward()
    nb = batch.nbands
    before = [batch[b].coeffs for b in range(B)]
    with pytest.raises(ValueError):
        batch.threshold_bands([1.0] * (nb - 1))
    with pytest.raises(ValueError):
        batch.threshold_bands(np.ones((B + 1, nb)))
    with pytest.raises(ValueError):
        batch.threshold_bands([1.0] * nb, kind="firm")
    with pytest.raises(ValueError):
        batch.denoise("sure")
    with pytest.raises(ValueError):
        batch.denoise("bayes", kind="garrote")
    with pytest.raises(ValueError):
        batch.denoise("bayes", sigma=-2.0)
    with pytest.raises(ValueError):
        batch.denoise("bayes", sigma=[1.0] * (B + 1))
    for b in range(B):  # a refused call launched nothing
        for old, new in zip(before[b], batch[b].coeffs):
            assert _same_bits(old, new)
    for call in _calls(batch):
        call()
    assert all(batch[b].state == pdwt_amd.W_FORWARD for b in range(B))
    mid = [batch[b].coeffs for b in range(B)]
    batch[1].inverse()  # one member inverted: the batch calls refuse and touch nothing
    _all_refuse(batch)
    for b in (0, 2):
        assert batch[b].state == pdwt_amd.W_FORWARD
        for old, new in zip(mid[b], batch[b].coeffs):
            assert _same_bits(old, new)
    batch.inverse()
    img = batch.get_images()
    _all_refuse(batch)  # after inverse()
    assert _same_bits(batch.get_images(), img)
    batch.forward()
    assert (batch.estimate_sigma() >= 0).all()
