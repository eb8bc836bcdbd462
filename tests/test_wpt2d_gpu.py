"""WaveletPackets2D on the GPU against tests/refwpt.py (the oracle's one-level transform applied to every node again, in the precision
under test).

Metric: tests/helpers.band_err per NODE (max |got - ref| / max |ref| of that node).  Bounds: 1e-5 (float32) and 1e-12 (float64) for
every node of every depth; 10x those for the round trip of a basis back to the image.  (The CPU reference alone stays within 5.4e-7 /
1e-15 on the round trips below, sym8 in float64 excepted: 1.15e-12, the table's sym banks do not reconstruct exactly.)  On the
uniform(-100, 100) inputs the smallest node maximum of a depth is at least 0.18 of the largest (asserted below), so the per-node
normalisation hides nothing.

The reference here is the oracle in the precision under test, and the banks are few (2, 4, 6, 8 and 16 taps).  The comparison with a
float64 statement of the tree, for all 72 banks and every instantiated filter length, is tests/test_newer_all_banks_gpu.py.
"""
import functools

import numpy as np
import pytest

import pdwt_amd
from pdwt_amd import DeviceArray, Wavelets, WaveletPackets2D
from pdwt_amd.wavelets import W_CREATION_ERROR, W_FORWARD, W_INIT, W_INVERSE, W_THRESHOLD
from tests import refwpt as R
from tests.helpers import band_err
from tests.refstats import ref_stats

pytestmark = pytest.mark.gpu

FWD = {np.dtype(np.float32): 1e-5, np.dtype(np.float64): 1e-12}
RT = {k: 10 * v for k, v in FWD.items()}
SUM_TOL = 1e-10  # sums accumulated in double (tests/test_bandstats_gpu.py)
DTYPES = [np.float32, np.float64]
CASES = [((64, 64), "db2", 3), ((33, 47), "haar", 3), ((96, 80), "db4", 9), ((40, 72), "coif1", 2), ((61, 67), "db2", 3), ((64, 96), "sym8", 2),
         ((48, 48), "bior2.2", 2)]


def _uniform(shape, dt):
    return np.random.RandomState(1).uniform(-100, 100, shape).astype(dt)


@functools.lru_cache(maxsize=None)
def _ref(shape, wname, levels, dtname, kind="uniform"):
    """(image, reference tree): computed once per case and shared; callers do not modify them"""
    dt = np.dtype(dtname)
    if kind == "uniform":
        x = _uniform(shape, dt)
    elif kind == "impulse":
        x = np.zeros(shape, dt)
        x[0, 0], x[-1, -1] = 100.0, -50.0
    elif kind == "ramp":
        yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
        x = (xx + 2.0 * yy - 7.0).astype(dt)
    else:
        x = _structured().astype(dt)
    # (depth 7 has 16384 nodes of one sample: the numpy restatement of the Haar tree, pinned to the oracle bit for bit on the CPU)
    tr = R.haar_tree(x, levels) if (wname == "haar" and levels >= 6) else R.tree(x, wname, levels)
    for t in tr:
        t.setflags(write=False)
    x.setflags(write=False)
    return x, tr


def _structured():
    yy, xx = np.mgrid[0:128, 0:128].astype(np.float64)
    return (50 * np.sin(2 * np.pi * 37 * xx / 128) + 0.2 * (xx + yy) + 30 * (np.hypot(xx - 40, yy - 70) < 20)
            + 2 * np.random.RandomState(5).randn(128, 128))


def _level_err(got, ref):
    """the largest band_err over the nodes of one depth (vectorised: depth 7 has 16384 nodes)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    den = np.abs(ref).reshape(ref.shape[0], -1).max(axis=1)
    num = np.abs(got - ref).reshape(ref.shape[0], -1).max(axis=1)
    return float((num / np.where(den > 0, den, 1.0)).max())


def _raw_level(W, depth):
    """all nodes of a depth read straight from device memory, whatever the state"""
    W.sync()
    return DeviceArray(W, W.node_int_ptr((depth, 0)), (4 ** depth,) + W.node_shape(depth), W.dtype).numpy()


def _check_tree(W, tr, bound, what):
    assert W.levels == len(tr) - 1, (what, W.levels)
    for d in range(W.levels + 1):
        assert W.node_shape(d) == tr[d].shape[1:], (what, d)
        e = _level_err(W.get_level(d), tr[d])
        print("%s depth %d: %d nodes, err %.3e" % (what, d, 4 ** d, e))
        assert e <= bound, (what, d, e)


# ---- forward and round trip ---------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape,wname,asked", CASES, ids=["%dx%d-%s" % (c[0] + (c[1],)) for c in CASES])
def test_forward_every_node_and_round_trip(shape, wname, asked, dt):
    x, tr = _ref(shape, wname, asked, np.dtype(dt).name)
    for t in tr[1:]:  # the normalisation hides nothing: no node of a depth is small against the others
        mx = np.abs(t).reshape(t.shape[0], -1).max(axis=1)
        assert mx.min() >= 0.18 * mx.max(), (wname, mx.min() / mx.max())
    W = WaveletPackets2D(x, wname, asked)
    assert W.state == W_INIT and W.dtype == np.dtype(dt)
    W.forward()
    assert W.state == W_FORWARD
    _check_tree(W, tr, FWD[np.dtype(dt)], "%s %s %s" % (shape, wname, np.dtype(dt).name))
    assert np.array_equal(W.get_image(), x)  # forward() leaves the image intact
    L = W.levels
    assert W.basis == [(L, i) for i in range(4 ** L)]
    for path in ("a", "d", "hv"[:L], "d" * L):
        d, i = R.index_of(path)
        assert np.array_equal(W.get_node(path), W.get_level(d)[i]) and np.array_equal(W.get_node((d, i)), W.get_node(path))
    W.inverse()
    assert W.state == W_INVERSE
    e = band_err(W.get_image(), x)
    print("round trip %.3e" % e)
    assert e <= RT[np.dtype(dt)], e


# ---- geometry that a tile kernel gets wrong -------------------------------------------------------------
@pytest.mark.parametrize("shape,wname,asked,dt,kind", [
    ((256, 320), "db4", 4, np.float32, "uniform"),   # several tiles per node at depth 0 / 1, 64 nodes of 32x40, 256 of 16x20
    ((256, 320), "db4", 4, np.float64, "uniform"),
    ((128, 128), "haar", 7, np.float32, "uniform"),  # leaf nodes of 1x1, 16384 of them
    ((130, 70), "db8", 3, np.float64, "uniform"),    # clamps to 2; nodes smaller than one tile, ragged tile ends
    ((130, 70), "db8", 3, np.float32, "uniform"),
    ((72, 40), "db4", 2, np.float32, "impulse"),     # the corners: everything there comes through the periodic halo
    ((72, 40), "db4", 2, np.float64, "impulse"),
    ((72, 40), "db4", 2, np.float32, "ramp"),
    ((45, 51), "haar", 3, np.float64, "ramp"),       # odd at every depth: the clamped butterfly
])
def test_geometry(shape, wname, asked, dt, kind):
    x, tr = _ref(shape, wname, asked, np.dtype(dt).name, kind)
    W = WaveletPackets2D(x, wname, asked)
    W.forward()
    _check_tree(W, tr, FWD[np.dtype(dt)], "%s %s %s %s" % (shape, wname, np.dtype(dt).name, kind))
    W.inverse()
    assert band_err(W.get_image(), x) <= RT[np.dtype(dt)]


def test_levels_clamp_to_seven():
    x = _uniform((256, 256), np.float32)
    W = WaveletPackets2D(x, "haar", 9)
    assert W.levels == 7 and W.node_shape(7) == (2, 2)
    with pytest.raises(IndexError):
        W.node_shape(8)
    W.forward()
    assert W.get_level(7).shape == (16384, 2, 2)
    W.inverse()
    assert band_err(W.get_image(), x) <= RT[np.dtype(np.float32)]
    assert WaveletPackets2D(_uniform((96, 80), np.float32), "db4", 9).levels == 3


# ---- against the existing transform ------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("shape,wname,L", [((64, 64), "db2", 3), ((33, 47), "haar", 3), ((61, 67), "db2", 3), ((64, 96), "sym8", 2)])
def test_all_a_path_is_the_ordinary_transform(shape, wname, L, dt):
    x = _uniform(shape, dt)
    P = WaveletPackets2D(x, wname, L)
    W = Wavelets(x, wname, L)
    P.forward()
    W.forward()
    assert P.levels == W.info.nlevels == L
    bands, bound = W.coeffs, FWD[np.dtype(dt)]  # [A_L, H1, V1, D1, ..., H_L, V_L, D_L]
    assert band_err(P.get_node("a" * L), bands[0]) <= bound
    for k in range(1, L + 1):
        for q, letter in enumerate("hvd"):
            assert band_err(P.get_node("a" * (k - 1) + letter), bands[3 * (k - 1) + 1 + q]) <= bound, (k, letter)


# ---- costs, best basis, partial basis ------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("wname,counts", [("db2", (0, 1, 6, 24)), ("db4", (0, 1, 6, 24)), ("haar", (0, 2, 4, 16))])
def test_costs_best_basis_and_inverse_from_it(wname, counts, dt):
    x, tr = _ref((128, 128), wname, 3, np.dtype(dt).name, "structured")
    W = WaveletPackets2D(x, wname, 3)
    for kind in ("l1", "shannon"):
        W.set_image(x)  # a fresh tree per cost: inverse() below ends the previous one
        W.forward()
        ref = R.node_costs(tr, kind)
        got = W.node_costs(kind)
        assert len(got) == 4 and all(g.dtype == np.float64 and g.shape == r.shape for g, r in zip(got, ref))
        rel = max(float((np.abs(g - r) / np.abs(r)).max()) for g, r in zip(got, ref))
        print("%s %s %s: node costs rel %.3e" % (wname, np.dtype(dt).name, kind, rel))
        assert rel <= 1e-9, (kind, rel)
        again = W.node_costs(kind)
        assert all(np.array_equal(a, g) for a, g in zip(again, got))  # fixed order of combination: the same bits
        want, margin = R.best_basis(ref)
        assert margin >= 1e-3  # (2e-3 measured: rounding cannot flip a decision)
        assert tuple(sum(1 for d, _ in want if d == k) for k in range(4)) == counts
        basis = W.best_basis(kind)
        assert basis == want == W.basis
        before = {d: _raw_level(W, d) for d in range(1, 4)}
        W.inverse()
        e = band_err(W.get_image(), x)
        print("%s %s %s: inverse from the best basis %.3e" % (wname, np.dtype(dt).name, kind, e))
        assert e <= RT[np.dtype(dt)], (kind, e)
        after = {d: _raw_level(W, d) for d in range(1, 4)}
        for d, i in want:  # inverse() writes parents only: the nodes of the basis keep their bits
            assert np.array_equal(before[d][i], after[d][i]), (kind, d, i)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("wname", ["db2", "db4", "haar"])
def test_hand_made_basis_with_a_zeroed_node(wname, dt):
    x, tr = _ref((128, 128), wname, 3, np.dtype(dt).name, "structured")
    names = ["a", "ha", "hh", "hv", "hd", "v", "d"]
    W = WaveletPackets2D(x, wname, 3)
    W.forward()
    W.set_basis(names)
    assert W.basis == sorted(R.index_of(n) for n in names)
    W.set_node("v", np.zeros(W.node_shape(1), dt))
    assert W.state == W_THRESHOLD
    nodes = {R.index_of(n): np.array(tr[len(n)][R.index_of(n)[1]]) for n in names}
    nodes[(1, 2)][...] = 0
    want = R.inverse(nodes, (128, 128), wname, 3)
    before = {n: W.node_view(n).numpy() for n in names}
    assert not before["v"].any()
    W.inverse()
    assert band_err(W.get_image(), want) <= FWD[np.dtype(dt)]
    for n in names:
        assert np.array_equal(W.node_view(n).numpy(), before[n]), n


# ---- thresholds, norms, statistics -----------------------------------------------------------------------
def _thresh(v, beta, kind):
    b = v.dtype.type(beta)
    if kind == "soft":
        return np.copysign(np.maximum(np.abs(v) - b, v.dtype.type(0)), v)
    return np.where(np.abs(v) > b, v, v.dtype.type(0))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("kind,app", [("soft", 0), ("hard", 0), ("soft", 1)])
def test_thresholds_touch_exactly_the_basis(kind, app, dt):
    x = _structured().astype(dt)
    names = ["a", "ha", "hh", "hv", "hd", "v", "daa", "dah", "dav", "dad", "dh", "dv", "dd"]
    W = WaveletPackets2D(x, "db2", 3)
    W.forward()
    W.set_basis(names)
    before = {d: _raw_level(W, d) for d in range(0, 4)}
    getattr(W, kind + "_threshold")(4.0, do_thresh_appcoeffs=app)
    assert W.state == W_THRESHOLD
    after = {d: _raw_level(W, d) for d in range(0, 4)}
    basis = set(W.basis)
    assert basis == {R.index_of(n) for n in names}
    for d in range(0, 4):
        for i in range(4 ** d):
            b, a = before[d][i], after[d][i]
            if (d, i) in basis and (i != 0 or app):
                want = _thresh(b, 4.0, kind)
                assert not np.array_equal(a, b), (d, i)
                assert np.allclose(a, want, rtol=1e-6 if dt == np.float32 else 1e-14, atol=0), (d, i)
            else:
                assert np.array_equal(a, b), (d, i)  # outside the basis, or the all-"a" node: the same bits
    # norm1 over the basis, after the threshold
    want = sum(np.abs(after[d][i].astype(np.float64)).sum() for d, i in basis)
    assert abs(W.norm1() - want) <= SUM_TOL * want


@pytest.mark.parametrize("dt", DTYPES)
def test_norm1_node_stats_and_sigma(dt):
    x = _structured().astype(dt)
    W = WaveletPackets2D(x, "db4", 3)
    W.forward()
    lev = {d: W.get_level(d).astype(np.float64) for d in range(0, 4)}
    want = np.abs(lev[3]).sum()
    assert abs(W.norm1() - want) <= SUM_TOL * want
    W.best_basis("l1")
    want = sum(np.abs(lev[d][i]).sum() for d, i in W.basis)
    assert abs(W.norm1() - want) <= SUM_TOL * want
    for d in range(0, 4):
        s = W.node_stats(d)
        flat = lev[d].reshape(4 ** d, -1)
        assert np.all(np.abs(s["sum_abs"] - np.abs(flat).sum(axis=1)) <= SUM_TOL * np.abs(flat).sum(axis=1))
        assert np.all(np.abs(s["sum_sq"] - (flat * flat).sum(axis=1)) <= SUM_TOL * (flat * flat).sum(axis=1))
        assert np.array_equal(s["max_abs"], np.abs(flat).max(axis=1))
    # selection does no arithmetic: equal to the mean of the two middle order statistics of the node as downloaded, in its own dtype
    node_d = W.get_node("d")
    assert node_d.dtype == np.dtype(dt)
    sig = ref_stats(node_d)["median_abs"] / 0.6744897501960817
    assert W.estimate_sigma() == sig, (W.estimate_sigma(), sig)
    assert 1.0 < sig < 4.0  # the image carries noise of sigma 2


# ---- state machine and errors -----------------------------------------------------------------------------
def test_state_machine_refusals_leave_the_data_alone():
    x = _uniform((64, 64), np.float32)
    W = WaveletPackets2D(x, "db2", 3)
    W.forward()
    W.inverse()
    assert W.state == W_INVERSE
    snap = {d: _raw_level(W, d) for d in range(0, 4)}
    for call in (lambda: W.get_node("a"), lambda: W.get_level(1), lambda: W.soft_threshold(1.0), lambda: W.hard_threshold(1.0),
                 lambda: W.best_basis("l1"), lambda: W.node_costs("l1"), lambda: W.norm1(), lambda: W.node_stats(1), lambda: W.estimate_sigma()):
        with pytest.raises(RuntimeError):
            call()
    with pytest.raises(RuntimeError):  # the parents hold reconstructions: no node may be replaced either
        W.set_node("a", np.zeros(W.node_shape(1), np.float32))
    W.inverse()  # refused with a warning
    assert W.state == W_INVERSE
    assert all(np.array_equal(snap[d], _raw_level(W, d)) for d in range(0, 4))
    # after a threshold / set_node the tree is no longer one transform
    W.set_image(x)
    assert W.state == W_INIT
    with pytest.raises(RuntimeError):  # no forward() yet
        W.set_node("a", np.zeros(W.node_shape(1), np.float32))
    assert W.state == W_INIT
    W.forward()
    W.soft_threshold(1.0)
    assert W.state == W_THRESHOLD
    snap = {d: _raw_level(W, d) for d in range(0, 4)}
    basis = W.basis
    with pytest.raises(RuntimeError):
        W.best_basis("shannon")
    with pytest.raises(RuntimeError):
        W.set_basis(["a", "h", "v", "d"])
    assert W.basis == basis and all(np.array_equal(snap[d], _raw_level(W, d)) for d in range(0, 4))
    W.inverse()  # thresholded coefficients may of course be inverted
    assert W.state == W_INVERSE


def test_set_basis_errors_and_bad_arguments():
    W = WaveletPackets2D(_uniform((64, 64), np.float32), "db2", 2)
    W.forward()
    for bad in (["a", "h", "v"], ["a", "h", "v", "d", "ah"], ["a", "a", "h", "v", "d"], ["aaa"], [(1, 4)], ["ax"]):
        with pytest.raises(ValueError):
            W.set_basis(bad)
    assert W.basis == [(2, i) for i in range(16)]
    W.set_basis([""])
    assert W.basis == [(0, 0)]
    W.inverse()  # nothing to synthesise
    assert np.array_equal(W.get_image(), _uniform((64, 64), np.float32))
    with pytest.raises(ValueError):
        W.node_costs("l2")
    with pytest.raises(ValueError):
        W.best_basis("entropy")
    with pytest.raises(IndexError):
        W.node_view("aaa")
    with pytest.raises(ValueError):
        WaveletPackets2D(np.zeros((4, 8, 8), np.float32), "db2", 1)


def test_creation_errors():
    assert WaveletPackets2D(_uniform((64, 64), np.float32), "nosuchwavelet", 2).state == W_CREATION_ERROR
    W = WaveletPackets2D(_uniform((6, 64), np.float32), "db4", 2)  # ilog2(6 / 7) = 0 levels
    assert W.state == W_CREATION_ERROR
    W.forward()
    W.inverse()
    assert W.state == W_CREATION_ERROR
    with pytest.raises(RuntimeError):
        W.get_node("a")


@pytest.mark.parametrize("dt", DTYPES)
def test_device_tensors_and_zero_copy_views(dt):
    import torch
    x = _uniform((61, 67), dt)
    t = torch.as_tensor(x, device="cuda")
    W = WaveletPackets2D(t, "db2", 2)
    H = WaveletPackets2D(x, "db2", 2)
    assert W.dtype == np.dtype(dt) and W.shape == (61, 67)
    W.forward()
    H.forward()
    assert all(np.array_equal(W.get_level(d), H.get_level(d)) for d in range(3))
    v = W.node_view("hd")
    assert v.ptr == W.node_int_ptr("hd") == W.node_int_ptr((2, 7)) and v.shape == W.node_shape(2)
    assert v.ptr == W.node_int_ptr((2, 0)) + 7 * v.shape[0] * v.shape[1] * np.dtype(dt).itemsize
    W.sync()
    tv = torch.as_tensor(v, device="cuda")
    assert tv.data_ptr() == v.ptr and np.array_equal(tv.cpu().numpy(), W.get_node("hd"))
    tv.zero_()  # a write through the view lands in the node
    torch.cuda.synchronize()
    assert not W.get_node("hd").any()
    W.set_node("hd", torch.as_tensor(H.get_node("hd"), device="cuda"))
    assert np.array_equal(W.get_node("hd"), H.get_node("hd")) and W.state == W_THRESHOLD
    W.set_image(torch.as_tensor(x[::-1].copy(), device="cuda"))
    assert np.array_equal(W.get_image(), x[::-1])
    with pytest.raises(TypeError):
        WaveletPackets2D(t, "db2", 2, dtype=np.float64 if dt == np.float32 else np.float32)
