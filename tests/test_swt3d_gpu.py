"""GPU parity of the 3-D stationary transform (pdwt_amd.StationaryWavelets3D, swt3d.hip).  The expected values compose the numpy
a-trous level of tests/test_swt3d_cpu.py (pinned there against the oracle's 1-D SWT) along x, y and z, level by level on the
aaa band -- no 3-D code of the library is involved."""
import ctypes as C

import numpy as np
import pytest

import pdwt_amd
from pdwt_amd import W_CREATION_ERROR, W_FORWARD, W_INVERSE
from pdwt_amd.wavelets3d import BAND_KEYS
from oracle import oracle as orc
from tests.helpers import band_err
from tests.test_swt3d_cpu import atrous_ana, atrous_syn, bank

pytestmark = pytest.mark.gpu

TOL3 = {np.dtype(np.float32): 1e-5, np.dtype(np.float64): 1e-12}


# ---- the composition --------------------------------------------------------------------------------------
def ref_forward(vol, wname, L):
    """[A_L, then levels L .. 1 in BAND_KEYS order]: the a-trous level along x (axis 2), y (1), z (0) at spacing 2^(lev-1)"""
    F = bank(wname, vol.dtype)
    per_level = []
    a = vol
    for lev in range(1, L + 1):
        f = 2 ** (lev - 1)
        bands = {"": a}
        for axis in (2, 1, 0):
            nxt = {}
            for key, b in bands.items():
                nxt["a" + key], nxt["d" + key] = atrous_ana(b, axis, F, f)
            bands = nxt
        per_level.append([bands[k] for k in BAND_KEYS])
        a = bands["aaa"]
    out = [a]
    for lev in range(L, 0, -1):
        out += per_level[lev - 1]
    return out


def ref_inverse(coeffs, wname, L):
    F = bank(wname, coeffs[0].dtype)
    a = coeffs[0]
    for lev in range(L, 0, -1):
        f = 2 ** (lev - 1)
        d = dict(zip(BAND_KEYS, coeffs[1 + 7 * (L - lev):8 + 7 * (L - lev)]))
        d["aaa"] = a
        # z, then y, then x: undo the forward passes in the opposite order
        q = {k: atrous_syn(d["a" + k], d["d" + k], 0, F, f) for k in ("aa", "ad", "da", "dd")}
        r = {k: atrous_syn(q["a" + k], q["d" + k], 1, F, f) for k in ("a", "d")}
        a = atrous_syn(r["a"], r["d"], 2, F, f)
    return a


def clamp(shape, wname, levels):
    hlen = orc.filters(wname)[0]
    return min(levels, orc.ilog2(min(shape) // (hlen - 1)))


def check_forward_inverse(vol, wname, levels, ref_inv=True):
    dt = vol.dtype
    W = pdwt_amd.StationaryWavelets3D(vol, wname, levels)
    L = clamp(vol.shape, wname, levels)
    if L < 1:
        assert W.state == W_CREATION_ERROR
        return None
    assert W.levels == L and W.nbands == 7 * L + 1
    W.forward()
    assert W.state == W_FORWARD
    got, want = W.coeffs, ref_forward(vol, wname, L)
    assert len(got) == len(want)
    for k, (g, o) in enumerate(zip(got, want)):
        assert g.shape == o.shape == vol.shape, (k, g.shape, o.shape)
        assert band_err(g, o) <= TOL3[dt], (wname, vol.shape, L, k, band_err(g, o))
    W.inverse()
    assert W.state == W_INVERSE
    rec = W.get_image()
    if ref_inv:
        assert band_err(rec, ref_inverse(got, wname, L)) <= TOL3[dt] * 10, (wname, vol.shape, L)
    assert band_err(rec, vol) <= TOL3[dt] * 10, (wname, vol.shape, L)
    # the inverse leaves every band intact, bit for bit
    for k, g in enumerate(got):
        assert np.array_equal(W.coeff_view(k).numpy(), g), k
    return W


# ---- forward / inverse ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("wname", ["haar", "db2", "db4", "sym8", "coif3"])
@pytest.mark.parametrize("shape", [(64, 64, 64), (33, 47, 61), (8, 72, 100)])
def test_forward_inverse_vs_composition(shape, wname, dtype):
    rs = np.random.RandomState(sum(shape) + len(wname))
    vol = rs.uniform(-100, 100, shape).astype(dtype)
    for levels in sorted({1, clamp(shape, wname, 99), 99}):  # level 1, the clamp itself, and a request above it
        check_forward_inverse(vol, wname, levels)


@pytest.mark.parametrize("shape,wname,dtype,levels", [((37, 45, 70), "db8", np.float32, 2), ((50, 61, 35), "db8", np.float64, 9),
                                                       ((100, 97, 130), "db12", np.float32, 2), ((49, 140, 47), "db12", np.float64, 1),
                                                       ((156, 160, 158), "db20", np.float64, 2), ((81, 79, 95), "db20", np.float32, 9),
                                                       ((5, 3, 7), "haar", np.float64, 9), ((19, 130, 33), "haar", np.float32, 9)])
def test_long_banks_and_ragged_tiles(shape, wname, dtype, levels):
    # sizes that are no multiple of the tap spacing, of the x-y tile or of the z chunk, and planes smaller than one tile
    vol = np.random.RandomState(sum(shape)).uniform(-1, 1, shape).astype(dtype)
    check_forward_inverse(vol, wname, levels)


def test_clamp_to_zero_levels_is_a_creation_error():
    W = pdwt_amd.StationaryWavelets3D(np.zeros((8, 64, 64), np.float32), "db4", 2)  # ilog2(8 / 7) = 0
    assert W.state == W_CREATION_ERROR
    W.forward()  # refused, no launch
    assert W.state == W_CREATION_ERROR
    assert check_forward_inverse(np.ones((30, 64, 64)), "db20", 1) is None  # ilog2(30 / 39) = 0


def test_inverse_of_arbitrary_bands_vs_composition():
    shape, wname, L = (40, 37, 50), "db3", 2
    for dt in (np.float32, np.float64):
        W = pdwt_amd.StationaryWavelets3D(np.zeros(shape, dt), wname, L)
        assert W.levels == L
        rs = np.random.RandomState(5)
        bands = [rs.uniform(-1, 1, W.band_shape(k)).astype(dt) for k in range(W.nbands)]
        for k, b in enumerate(bands):
            W.set_coeff(b, k)
        W.inverse()
        assert band_err(W.get_image(), ref_inverse(bands, wname, L)) <= TOL3[np.dtype(dt)] * 10
        for k, b in enumerate(bands):
            assert np.array_equal(W.coeff_view(k).numpy(), b), k


def test_full_size_256_float32_db4_l3():
    vol = np.random.RandomState(6).uniform(0, 255, (256, 256, 256)).astype(np.float32)
    W = check_forward_inverse(vol, "db4", 3, ref_inv=False)
    assert W.levels == 3
    W.close()


# ---- thresholds and norm1 -----------------------------------------------------------------------------------
def _betas(beta, L, dt, app, normalize, hard):
    T = dt.type
    beta = T(beta)
    b_app = beta
    if normalize > 0 and not hard:  # beta / sqrt(2)^L, computed as the 2-D path does
        nl2 = L // 2
        b_app = T(beta / T(1 << nl2))
        if nl2 * 2 != L:
            b_app = T(np.float64(b_app) / 1.4142135623730951)
    lev_b = []
    for _ in range(L):
        if normalize > 0:
            beta = T(np.float64(beta) / 1.4142135623730951)
        lev_b.append(beta)
    return (b_app if app else None), lev_b  # lev_b[lev - 1]


def _np_thresh(bands, beta, L, dt, app, normalize, hard):
    b_app, lev_b = _betas(beta, L, dt, app, normalize, hard)
    out = [b.copy() for b in bands]

    def op(x, b):
        if hard:
            return ((np.abs(x) - b > 0).astype(dt) * x).astype(dt)
        m = np.abs(x) - b
        return np.copysign(np.where(m > 0, m, 0), x).astype(dt)
    if b_app is not None:
        out[0] = op(out[0], b_app)
    for k in range(1, len(out)):
        lev = L - (k - 1) // 7
        out[k] = op(out[k], lev_b[lev - 1])
    return out


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("app,normalize", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_thresholds_and_norm1_vs_numpy(dtype, app, normalize):
    shape, wname, L = (24, 33, 40), "db2", 3
    vol = np.random.RandomState(7).uniform(-10, 10, shape).astype(dtype)
    want = ref_forward(vol, wname, L)
    n_ref = sum(np.abs(b.astype(np.float64)).sum() for b in want)
    for hard in (False, True):
        W = pdwt_amd.StationaryWavelets3D(vol, wname, L)
        assert W.levels == L
        W.forward()
        assert abs(W.norm1_f64() - n_ref) <= 1e-6 * n_ref
        before = W.coeffs
        (W.hard_threshold if hard else W.soft_threshold)(3.0, app, normalize)
        # elementwise: bit-identical to numpy on the same bands
        for k, (g, o) in enumerate(zip(W.coeffs, _np_thresh(before, 3.0, L, np.dtype(dtype), app, normalize, hard))):
            assert np.array_equal(g, o), (hard, k)
        n_got = sum(np.abs(b.astype(np.float64)).sum() for b in W.coeffs)
        assert abs(W.norm1_f64() - n_got) <= 1e-9 * max(n_got, 1.0)
        assert abs(float(W.norm1()) - n_got) <= 1e-6 * max(n_got, 1.0)


# ---- state machine, zero copy, refusals ----------------------------------------------------------------------
def test_state_machine():
    vol = np.random.RandomState(8).randn(32, 32, 32).astype(np.float32)
    W = pdwt_amd.StationaryWavelets3D(vol, "db2", 2)
    W.inverse()  # before forward: the inverse of the (zero) coefficients
    assert W.state == W_INVERSE
    assert np.array_equal(W.get_image(), np.zeros_like(vol))
    W.set_image(vol)
    W.forward()
    W.inverse()
    assert W.state == W_INVERSE
    before = W.coeff_view(1).numpy()
    W.soft_threshold(1e9)  # after inverse: refused, the bands stay as they are
    assert np.array_equal(W.coeff_view(1).numpy(), before)
    with pytest.raises(RuntimeError):
        W.get_coeff(0)  # refused after inverse
    img = W.get_image()
    W.inverse()  # a second inverse is refused
    assert np.array_equal(W.get_image(), img)
    W.forward()  # a new forward makes the coefficients valid again
    assert W.state == W_FORWARD and W.get_coeff(0).shape == (32, 32, 32)
    assert W.band_index(2, "aad") == 1 and W.band_index(1, "ddd") == 14


def test_zero_copy_torch_input_and_views():
    torch = pytest.importorskip("torch")
    vol = np.random.RandomState(9).randn(20, 36, 44)
    for dt in (np.float32, np.float64):
        v = vol.astype(dt)
        t = torch.from_numpy(v).to("cuda")
        Wt, Wn = pdwt_amd.StationaryWavelets3D(t, "sym4", 2), pdwt_amd.StationaryWavelets3D(v, "sym4", 2)
        assert Wt.dtype == np.dtype(dt)
        Wt.forward()
        Wn.forward()
        for a, b in zip(Wt.coeffs, Wn.coeffs):
            assert np.array_equal(a, b)
        Wt.sync()
        band = torch.as_tensor(Wt.coeff_view(3), device="cuda")
        assert np.array_equal(band.cpu().numpy(), Wn.get_coeff(3))
        assert np.array_equal(torch.as_tensor(Wt.image_view(), device="cuda").cpu().numpy(), v)
        Wt.set_image(t * 2)
        assert np.array_equal(Wt.get_image(), v * 2)
        Wt.set_coeff(t, 0)
        assert np.array_equal(Wt.get_coeff(0), v)


def test_out_of_scope_modes_are_refused():
    vol = np.zeros((16, 16, 16), np.float32)
    for kw in ({"do_separable": 0}, {"do_cycle_spinning": 1}):
        with pytest.raises(ValueError):
            pdwt_amd.StationaryWavelets3D(vol, "haar", 1, **kw)
    with pytest.raises(ValueError):
        pdwt_amd.StationaryWavelets3D(np.zeros((16, 16), np.float32), "haar", 1)
    W = pdwt_amd.StationaryWavelets3D(vol, "haar", 1)
    W.forward()
    for m in (W.group_soft_threshold, W.shrink, W.proj_linf):
        with pytest.raises(ValueError):
            m(1.0)
    with pytest.raises(ValueError):
        W.set_filters_forward("x", [1.0, 1.0], [1.0, -1.0])
    assert pdwt_amd.StationaryWavelets3D(vol, "nosuch", 1).state == W_CREATION_ERROR
    # the decimated class keeps refusing SWT
    with pytest.raises(ValueError):
        pdwt_amd.Wavelets3D(vol, "haar", 1, do_swt=1)
    # the C-ABI refuses a bank whose length is not the geometry's
    H = pdwt_amd.hip()
    info = pdwt_amd.Info3D(16, 16, 16, 1, 4)
    f = pdwt_amd._native.Filters32()
    assert H.pdwt_compute_filters_separable_f32(b"haar", 1, C.byref(f)) == 2
    c = H.pdwt_create_coeffs_buffer_swt3d_f32(info)
    tmp = H.pdwt_malloc(H.pdwt_tmp_elems_swt3d(info) * 4)
    assert c and tmp
    try:
        assert H.pdwt_forward3d_swt_f32(W.image_int_ptr(), c, tmp, info, C.byref(f)) < 0
        assert H.pdwt_inverse3d_swt_f32(W.image_int_ptr(), c, tmp, info, C.byref(f)) < 0
    finally:
        H.pdwt_free_coeffs_buffer_swt3d_f32(c, info)
        H.pdwt_free(tmp)
