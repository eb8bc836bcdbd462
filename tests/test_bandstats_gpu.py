"""GPU tests of the band statistics and the noise-adaptive thresholds (bandstats.hip; band_stats / all_band_stats / estimate_sigma /
threshold_bands / denoise of Wavelets, Wavelets3D and StationaryWavelets3D) against the numpy restatement of tests/refstats.py on the
bands downloaded with get_coeff.  median_abs, max_abs and n must be EQUAL (selection and max do no arithmetic); sum_abs and sum_sq
agree to 1e-10 relative (tests/helpers.py TOL of float64: the accumulation is in double for both dtypes)."""
import numpy as np
import pytest

import pdwt_amd
from tests.helpers import TOL
from tests.refstats import MAD_SCALE, ref_betas, ref_stats, ref_threshold

pytestmark = pytest.mark.gpu

SUM_TOL = TOL[np.dtype(np.float64)]
DTYPES = [np.float32, np.float64]


def _rel(a, b):
    if np.isinf(b) or np.isinf(a):
        return 0.0 if a == b else np.inf
    return abs(a - b) / (abs(b) if b != 0 else 1.0)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _check_band(got, band, with_median=True, what=""):
    ref = ref_stats(band)
    print("%s n=%d median %r / %r max %r / %r sum_abs rel %.2e sum_sq rel %.2e"
          % (what, ref["n"], got["median_abs"], ref["median_abs"], got["max_abs"], ref["max_abs"],
             _rel(got["sum_abs"], ref["sum_abs"]), _rel(got["sum_sq"], ref["sum_sq"])))
    assert got["n"] == ref["n"], what
    assert got["max_abs"] == ref["max_abs"], what
    if with_median:
        assert got["median_abs"] == ref["median_abs"] and not np.signbit(got["median_abs"]), what
    else:
        assert np.isnan(got["median_abs"]), what
    assert _rel(got["sum_abs"], ref["sum_abs"]) <= SUM_TOL, what
    assert _rel(got["sum_sq"], ref["sum_sq"]) <= SUM_TOL, what


def _make(case, dtype):
    rs = np.random.RandomState(7)
    kind, shape, wname, L = case[:4]
    kw = case[4] if len(case) > 4 else {}
    x = (rs.standard_normal(shape) * 3 + rs.uniform(-1, 1, shape).cumsum(axis=-1)).astype(dtype)
    if kind == "2d":
        return pdwt_amd.Wavelets(x, wname, L, **kw)
    if kind == "3d":
        return pdwt_amd.Wavelets3D(x, wname, L)
    return pdwt_amd.StationaryWavelets3D(x, wname, L)


CASES = [
    ("2d", (512, 512), "db4", 3), ("2d", (63, 65), "db4", 2), ("2d", (512, 512), "haar", 3),
    ("2d", (64, 64), "db2", 2, dict(do_swt=1)), ("2d", (96, 80), "db3", 2, dict(do_separable=0)),
    ("2d", (5, 256), "sym8", 4, dict(ndim=1)),
    ("3d", (40, 48, 56), "db2", 2), ("3d", (33, 35, 37), "db2", 2), ("swt3d", (32, 32, 32), "db2", 2),
]


# ---- 1. exactness of the statistics --------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-%s-%s-L%d%s" % (c[0], "x".join(map(str, c[1])), c[2], c[3], "".join("-" + k for k in (c[4] if len(c) > 4 else {}))))
def test_statistics_of_every_band_are_exact(case, dtype):
    W = _make(case, dtype)
    assert W.info.nlevels == case[3]
    W.forward()
    bands = W.coeffs
    every = W.all_band_stats(with_median=True)
    plain = W.all_band_stats()
    assert len(every) == len(bands) == W.nbands
    for k, b in enumerate(bands):
        one = W.band_stats(k)
        _check_band(one, b, what="band %d" % k)
        for key in one:  # all_band_stats equals band_stats bit for bit
            assert np.float64(one[key]).tobytes() == np.float64(every[k][key]).tobytes(), (k, key)
            if key != "median_abs":
                assert np.float64(one[key]).tobytes() == np.float64(plain[k][key]).tobytes(), (k, key)
        assert np.isnan(plain[k]["median_abs"])
        _check_band(W.band_stats(k, with_median=False), b, with_median=False, what="band %d, no median" % k)
    assert W.estimate_sigma() == ref_stats(bands[_finest(W)])["median_abs"] / MAD_SCALE


# ---- 2. selection on hard inputs -----------------------------------------------------------------------------
def _hard_inputs(n, dtype):
    rs = np.random.RandomState(n)
    tiny = 1e-40 if dtype == np.float32 else 1e-310
    z = np.zeros(n, dtype)
    z[::7] = -0.0
    sparse = np.where(rs.uniform(size=n) < 0.9, 0.0, rs.standard_normal(n)).astype(dtype)
    infs = rs.standard_normal(n).astype(dtype)
    idx = rs.permutation(n)[:max(2, n // 100)] if n >= 4 else np.arange(0)
    infs[idx[::2]] = np.inf
    infs[idx[1::2]] = -np.inf
    with np.errstate(under="ignore"):
        den = (rs.standard_normal(n) * tiny).astype(dtype)
    inc = (np.arange(n, dtype=np.float64) * 1.25 + 0.5).astype(dtype) * np.where(np.arange(n) % 2, -1, 1).astype(dtype)
    return {"equal": np.full(n, -0.75, dtype), "zeros": z, "sparse": sparse, "denormal": den, "inf": infs, "increasing": inc}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,ndim", [((256, 256), 2), ((130, 126), 2), ((1, 34), 1), ((1, 36), 1), ((3, 2050), 1)])
def test_selection_on_hard_inputs(shape, ndim, dtype):
    W = pdwt_amd.Wavelets(np.random.RandomState(1).standard_normal(shape).astype(dtype), "db2", 1, ndim=ndim)
    W.forward()
    fin = 3 if ndim == 2 else 1
    bshape = W.band_shape(fin)
    n = bshape[0] * bshape[1]
    if shape == (1, 34):
        assert n == 17
    if shape == (1, 36):
        assert n == 18
    for name, v in _hard_inputs(n, dtype).items():
        W.set_coeff(v.reshape(bshape), fin)
        band = W.get_coeff(fin)
        assert _same_bits(band, v.reshape(bshape)), name
        got = W.band_stats(fin)
        _check_band(got, band, what="%s n=%d" % (name, n))
        if name == "zeros":
            assert got["median_abs"] == 0.0 and not np.signbit(got["median_abs"])
        if name == "inf" and n >= 4:
            assert np.isfinite(got["median_abs"]) and got["max_abs"] == np.inf
        if name == "equal":
            assert got["median_abs"] == 0.75 == got["max_abs"]
        assert W.estimate_sigma() == got["median_abs"] / MAD_SCALE


# ---- 3. full size, determinism -------------------------------------------------------------------------------
def test_full_size_4096_float32_db4_l3():
    x = np.random.RandomState(3).uniform(0, 255, (4096, 4096)).astype(np.float32)
    W = pdwt_amd.Wavelets(x, "db4", 3)
    W.forward()
    d1 = W.get_coeff(3)
    ref = ref_stats(d1)
    s1 = W.estimate_sigma()
    assert s1 == ref["median_abs"] / MAD_SCALE
    a, b = W.all_band_stats(with_median=True), W.all_band_stats(with_median=True)
    assert a == b and W.estimate_sigma() == s1  # two runs, identical bits
    _check_band(a[3], d1, what="4096^2 D1")
    W.soft_threshold(20.0)  # mostly zeros now
    _check_band(W.band_stats(3), W.get_coeff(3), what="4096^2 D1 after soft_threshold")


def test_full_size_8192_float64_db20_l6():
    x = np.random.RandomState(4).standard_normal((8192, 8192))
    W = pdwt_amd.Wavelets(x, "db20", 6)
    assert W.info.nlevels == 6
    W.forward()
    del x
    d1 = W.get_coeff(3)
    a, b = W.band_stats(3), W.band_stats(3)
    assert a == b
    _check_band(a, d1, what="8192^2 f64 D1")


# ---- 4. threshold_bands --------------------------------------------------------------------------------------
THRESH_CASES = [("2d", (192, 160), "db4", 3), ("2d", (4, 512), "sym8", 3, dict(ndim=1)), ("3d", (40, 48, 56), "db2", 2),
                ("swt3d", (32, 32, 32), "db2", 2)]


@pytest.mark.parametrize("kind", ["soft", "hard"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", THRESH_CASES, ids=lambda c: c[0] + "-" + "x".join(map(str, c[1])))
def test_threshold_bands_against_numpy_and_the_uniform_threshold(case, dtype, kind):
    W, T = _make(case, dtype), _make(case, dtype)
    W.forward()
    T.forward()
    before = W.coeffs
    rs = np.random.RandomState(11)
    betas = rs.uniform(0.0, 3.0, W.nbands)
    betas[rs.uniform(size=W.nbands) < 0.3] = -1.0
    betas[0], betas[1] = -0.5, 0.0
    W.threshold_bands(betas, kind)
    assert W.state == pdwt_amd.W_FORWARD
    b_t = betas.astype(dtype)
    for k, (b, a) in enumerate(zip(before, W.coeffs)):
        assert _same_bits(a, ref_threshold(b, b_t[k], kind)), (k, betas[k])
        if betas[k] < 0:
            assert _same_bits(a, b), k
    # all betas equal, band 0 left alone: the existing uniform threshold on a twin
    W2 = _make(case, dtype)
    W2.forward()
    W2.threshold_bands([-1.0] + [1.25] * (W2.nbands - 1), kind)
    (T.soft_threshold if kind == "soft" else T.hard_threshold)(1.25)
    for k, (a, t) in enumerate(zip(W2.coeffs, T.coeffs)):
        assert _same_bits(a, t), k


@pytest.mark.parametrize("dtype", DTYPES)
def test_threshold_bands_drops_the_cached_norm(dtype):
    x = np.random.RandomState(5).standard_normal((256, 256)).astype(dtype)
    W = pdwt_amd.Wavelets(x, "db4", 3)
    W.set_norm_cache(1)
    W.forward()
    W.soft_threshold(0.1)
    cached = W.norm1_f64()
    W.threshold_bands([-1.0] + [0.7] * (W.nbands - 1))
    fresh = float(sum(np.abs(b).astype(np.float64).sum() for b in W.coeffs))
    got = W.norm1_f64()
    assert got != cached and abs(got - fresh) <= SUM_TOL * fresh
    W.denoise("visu", sigma=0.2)
    fresh2 = float(sum(np.abs(b).astype(np.float64).sum() for b in W.coeffs))
    assert abs(W.norm1_f64() - fresh2) <= SUM_TOL * fresh2 and fresh2 < fresh


# ---- 5. denoise ----------------------------------------------------------------------------------------------
def _samples(W):
    if isinstance(W, pdwt_amd.Wavelets3D):
        return float(np.prod(W.shape))
    return float(W.shape[1] if W.info.ndims == 1 else W.shape[0] * W.shape[1])


def _finest(W):
    if isinstance(W, pdwt_amd.Wavelets3D):
        return 7 * W.levels
    return 1 if W.info.ndims == 1 else 3


@pytest.mark.parametrize("sigma", [None, 0.8])
@pytest.mark.parametrize("kind", ["soft", "hard"])
@pytest.mark.parametrize("method", ["visu", "bayes"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", THRESH_CASES, ids=lambda c: c[0] + "-" + "x".join(map(str, c[1])))
def test_denoise_betas_and_bands(case, dtype, method, kind, sigma):
    W = _make(case, dtype)
    W.forward()
    before = W.coeffs
    stats = [ref_stats(b) for b in before]
    r = W.denoise(method, sigma=sigma, kind=kind)
    want_sigma = stats[_finest(W)]["median_abs"] / MAD_SCALE if sigma is None else sigma
    assert r["sigma"] == want_sigma
    betas = r["betas"]
    assert betas.dtype == np.dtype(dtype) and betas.shape == (W.nbands,) and betas[0] == -1
    want = ref_betas(stats, want_sigma, method, _samples(W))
    tol = 1e-6 if dtype == np.float32 else 1e-10
    rel = np.abs(betas[1:].astype(np.float64) - want[1:]) / np.abs(want[1:])
    print("denoise betas: max rel err %.3e" % rel.max())
    assert rel.max() <= tol
    for k, (b, a) in enumerate(zip(before, W.coeffs)):
        assert _same_bits(a, ref_threshold(b, betas[k], kind)), k
        if method == "bayes" and k > 0 and stats[k]["sum_sq"] / stats[k]["n"] <= want_sigma ** 2:
            assert not a.any(), k
    assert _same_bits(W.coeffs[0], before[0])


@pytest.mark.parametrize("kind", ["soft", "hard"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_bayes_zeroes_a_band_below_the_noise(dtype, kind):
    x = np.random.RandomState(6).standard_normal((128, 128)).astype(dtype)
    W = pdwt_amd.Wavelets(x, "db4", 2)
    W.forward()
    stats = [ref_stats(b) for b in W.coeffs]
    r = W.denoise("bayes", sigma=5.0, kind=kind)  # every detail band of unit-variance noise has ms < 25
    for k in range(1, W.nbands):
        assert r["betas"][k] == dtype(stats[k]["max_abs"]) and not W.get_coeff(k).any(), k


@pytest.mark.parametrize("method", ["visu", "bayes"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_constant_image_gives_sigma_zero_and_unchanged_bands(dtype, method):
    W = pdwt_amd.Wavelets(np.full((128, 128), 3.0, dtype), "haar", 3)
    W.forward()
    before = W.coeffs
    assert W.estimate_sigma() == 0.0
    r = W.denoise(method)
    assert r["sigma"] == 0.0 and np.isfinite(r["betas"]).all() and (r["betas"][1:] == 0).all() and r["betas"][0] == -1
    for b, a in zip(before, W.coeffs):
        assert _same_bits(a, b)


# ---- 6. it denoises ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", [0.05, 0.2])
@pytest.mark.parametrize("method", ["visu", "bayes"])
@pytest.mark.parametrize("wname", ["db4", "sym8", "haar"])
def test_it_denoises(wname, method, sigma):
    g = np.mgrid[0:512, 0:512] / 512
    x, y = g[0], g[1]
    clean = np.sin(6 * x) * np.cos(4 * y) + 0.5 * (x > 0.5) + 0.7 * ((x - 0.3) ** 2 + (y - 0.6) ** 2 < 0.04)
    noisy = clean + sigma * np.random.default_rng(1).standard_normal(clean.shape)
    W = pdwt_amd.Wavelets(noisy, wname, 3)
    assert W.dtype == np.float64 and W.info.nlevels == 3
    W.forward()
    r = W.denoise(method)
    W.inverse()
    den = W.get_image()
    ratio = np.mean((noisy - clean) ** 2) / np.mean((den - clean) ** 2)
    print("%s %s sigma %.2f: sigma_hat %.5f (%.2f %%), mse ratio %.2f" % (wname, method, sigma, r["sigma"], 100 * (r["sigma"] / sigma - 1), ratio))
    assert abs(r["sigma"] / sigma - 1) <= 0.05
    assert ratio >= 2


# ---- 7. state machine and errors -----------------------------------------------------------------------------
def _instances():
    rs = np.random.RandomState(2)
    return [pdwt_amd.Wavelets(rs.standard_normal((64, 64)).astype(np.float32), "db2", 2),
            pdwt_amd.Wavelets3D(rs.standard_normal((16, 16, 16)), "db2", 1),
            pdwt_amd.StationaryWavelets3D(rs.standard_normal((16, 16, 16)).astype(np.float32), "db2", 1)]


def _all_refuse(W):
    for call in (lambda: W.band_stats(1), lambda: W.all_band_stats(), lambda: W.estimate_sigma(),
                 lambda: W.threshold_bands([1.0] * W.nbands), lambda: W.denoise("bayes"), lambda: W.denoise("visu", sigma=1.0)):
        with pytest.raises(RuntimeError):
            call()


def test_state_machine_and_errors():
    for W in _instances():
        _all_refuse(W)  # before forward()
        W.forward()
        before = W.coeffs
        with pytest.raises(IndexError):
            W.band_stats(W.nbands)
        with pytest.raises(IndexError):
            W.band_stats(-1)
        with pytest.raises(ValueError):
            W.threshold_bands([1.0] * (W.nbands - 1))
        with pytest.raises(ValueError):
            W.threshold_bands([1.0] * W.nbands, kind="firm")
        with pytest.raises(ValueError):
            W.denoise("sure")
        with pytest.raises(ValueError):
            W.denoise("bayes", kind="garrote")
        with pytest.raises(ValueError):
            W.denoise("bayes", sigma=-2.0)
        for b, a in zip(before, W.coeffs):  # a refused call launched nothing
            assert _same_bits(a, b)
        assert W.band_stats(1)["n"] == before[1].size
        W.denoise("bayes")
        assert W.state == pdwt_amd.W_FORWARD
        W.band_stats(1)  # still valid after a threshold
        W.inverse()
        img = W.get_image()
        _all_refuse(W)  # after inverse()
        assert _same_bits(W.get_image(), img)
        W.set_image(img)
        _all_refuse(W)  # a new image: coefficients not computed
        W.forward()
        assert W.estimate_sigma() >= 0
