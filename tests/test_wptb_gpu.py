"""WaveletPacketBatch on the GPU: every node of every depth of every image against tests/refwpt.py (the oracle's one-level transform applied
to every node again, in the precision under test), the fused form against the per-depth form and against a loop over WaveletPackets2D bit
for bit, the chunks of the per-depth form, one basis for the batch, costs, thresholds, statistics, the state machine and device tensors.

Metric: per image and depth, max |got - ref| over the depth / max |ref| over the depth.  Bounds: those of tests/test_wpt2d_gpu.py -- 1e-5
(float32) and 1e-12 (float64) for the nodes, 10x for a round trip.  Every case asserts which form the plan (pdwt_wptb_fused) picks.
A run of one (case, precision, form) is computed once and shared by the tests that need it; nobody modifies it.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import pdwt_amd
from pdwt_amd import DeviceArray, WaveletPacketBatch, WaveletPackets2D
from pdwt_amd.wavelets import W_CREATION_ERROR, W_FORWARD, W_INIT, W_INVERSE, W_THRESHOLD
from tests import refwpt as R
from tests.helpers import band_err
from tests.refstats import MAD_SCALE, ref_stats, ref_threshold
from tests.test_wptb_cpu import largest_fused_square

pytestmark = pytest.mark.gpu

FWD = {np.dtype(np.float32): 1e-5, np.dtype(np.float64): 1e-12}
RT = {k: 10 * v for k, v in FWD.items()}
SUM_TOL = 1e-10  # sums accumulated in double
DTYPES = [np.float32, np.float64]
N32 = largest_fused_square(8, 4)  # the largest db4 L3 float32 square the plan fuses
# (B, Nr, Nc), bank, asked depth, fused in float32, fused in float64
CASES = {
    "odd": ((3, 37, 51), "db3", 2, 1, 1),             # odd at every depth
    "haar-odd": ((2, 9, 7), "haar", 2, 1, 1),         # 1-wide nodes, the clamped butterfly
    "haar-1x1": ((2, 8, 8), "haar", 3, 1, 1),         # 1 x 1 nodes
    "64": ((5, 64, 64), "db4", 3, 1, 1),              # float32 below the 64 KiB opt-in, float64 above
    "128": ((2, 128, 128), "db4", 3, 1, 0),           # float32 above the opt-in, float64 per depth
    "sym8": ((2, 61, 67), "sym8", 2, 1, 1),
    "db20": ((2, 78, 80), "db20", 1, 1, 1),           # looped taps
    "160x200": ((2, 160, 200), "db4", 3, 0, 0),       # per depth
    "one": ((1, 37, 51), "db3", 2, 1, 1),             # B = 1
    "budget-in": ((2, N32, N32), "db4", 3, 1, 0),     # the two squares either side of the budget
    "budget-out": ((2, N32 + 1, N32 + 1), "db4", 3, 0, 0),
}
FUSED_CASES = [(n, dt) for n in CASES for k, dt in enumerate(DTYPES) if CASES[n][3 + k]]


def _images(shape, dt, seed=1):
    return np.random.RandomState(seed).uniform(-100, 100, shape).astype(dt)


@functools.lru_cache(maxsize=None)
def _ref(name, dtname):
    """(images, [reference tree of image b]): computed once per case and shared"""
    shape, wname, asked = CASES[name][:3]
    x = _images(shape, np.dtype(dtname))
    trees = [R.tree(x[b], wname, asked) for b in range(shape[0])]
    x.setflags(write=False)
    return x, trees


@functools.lru_cache(maxsize=None)
def _run(name, dtname, allow_fused):
    """(fused, [depth 0 .. L as (B, 4^l, nr, nc)], reconstruction from the default basis) of one form"""
    x = _ref(name, dtname)[0]
    W = WaveletPacketBatch(x, CASES[name][1], CASES[name][2], allow_fused=allow_fused)
    assert W.state == W_INIT and W.dtype == np.dtype(dtname) and W.shape == x.shape
    W.forward()
    assert W.state == W_FORWARD
    levels = [W.get_level(d) for d in range(W.levels + 1)]
    assert np.array_equal(W.get_image(), x)  # forward() leaves the images intact
    W.inverse()
    assert W.state == W_INVERSE
    rec = W.get_image()
    for a in levels + [rec]:
        a.setflags(write=False)
    return W.fused, levels, rec


def _depth_err(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.abs(got - ref).max() / np.abs(ref).max())


def _raw_level(W, depth):
    """a whole depth read straight from device memory, whatever the state"""
    W.sync()
    return W.level_view(depth).numpy()


# ---- accuracy ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name", list(CASES))
def test_every_node_of_every_image_and_the_round_trip(name, dt):
    dt = np.dtype(dt)
    shape, wname, asked, f32, f64 = CASES[name]
    want_fused = bool(f32 if dt == np.float32 else f64)
    hlen = R.hlen_of(wname)
    L = R.clamp_levels(shape[1:], wname, asked)
    assert pdwt_amd.hip().pdwt_wptb_fused(shape[1], shape[2], hlen, L, dt.itemsize) == int(want_fused)
    x, trees = _ref(name, dt.name)
    fused, levels, rec = _run(name, dt.name, True)
    assert fused == want_fused and len(levels) == L + 1
    for d in range(L + 1):
        assert levels[d].shape == (shape[0], 4 ** d) + trees[0][d].shape[1:]
        for b in range(shape[0]):
            e = _depth_err(levels[d][b], trees[b][d])
            print("%s %s image %d depth %d: %.3e" % (name, dt.name, b, d, e))
            assert e <= FWD[dt], (name, b, d, e)
    e = band_err(rec, x)
    print("%s %s round trip: %.3e" % (name, dt.name, e))
    assert e <= RT[dt], e


# ---- bit identity -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dt", FUSED_CASES, ids=["%s-%s" % (n, np.dtype(d).name) for n, d in FUSED_CASES])
def test_fused_per_depth_and_a_loop_over_single_images_give_the_same_bits(name, dt):
    dt = np.dtype(dt)
    x = _ref(name, dt.name)[0]
    fused, levels, rec = _run(name, dt.name, True)
    pfused, plevels, prec = _run(name, dt.name, False)
    assert fused and not pfused
    for d in range(len(levels)):
        assert np.array_equal(levels[d], plevels[d]), (name, d)
    assert np.array_equal(rec, prec)
    for b in range(x.shape[0]):
        S = WaveletPackets2D(x[b], CASES[name][1], CASES[name][2])
        S.forward()
        for d in range(len(levels)):
            assert np.array_equal(S.get_level(d), levels[d][b]), (name, b, d)
        S.inverse()
        assert np.array_equal(S.get_image(), rec[b]), (name, b)


# ---- chunks of the per-depth form ---------------------------------------------------------------------------------------------------------
def test_per_depth_form_in_two_chunks():
    """5 x 128 x 128 Haar, 7 depths: 5 * 4096 = 20480 parents at the last step, so a chunk of 16384 (four images) and one of 4096"""
    x = _images((5, 128, 128), np.float32, seed=9)
    F = WaveletPacketBatch(x, "haar", 7)
    P = WaveletPacketBatch(x, "haar", 7, allow_fused=False)
    assert F.fused and not P.fused and F.levels == P.levels == 7
    F.forward()
    P.forward()
    ref = R.haar_tree(x[0], 7)
    for d in range(8):
        lf = F.get_level(d)
        assert lf.shape == (5, 4 ** d, 128 >> d, 128 >> d)
        assert np.array_equal(lf, P.get_level(d)), d
        assert _depth_err(lf[0], ref[d]) <= FWD[np.dtype(np.float32)], d
    F.inverse()  # the default basis: every parent of every depth, the last step in two chunks
    P.inverse()
    assert np.array_equal(F.get_image(), P.get_image()) and band_err(F.get_image(), x) <= RT[np.dtype(np.float32)]
    for W in (F, P):
        W.set_image(x)
        W.forward()
    # a basis that follows "daaaaa" down to depth 7: one parent per image to synthesise at every depth 1 .. 6, so the per-depth inverse runs
    # chunk-relative lists, at depth 6 over two chunks (the second takes a prefix of the list)
    names = ["a", "h", "v"] + ["d" + "a" * 5 + q for q in "ahvd"] + ["d" + "a" * k + q for k in range(5) for q in "hvd"]
    F.set_basis(names)
    P.set_basis(names)
    F.inverse()
    P.inverse()
    assert np.array_equal(F.get_image(), P.get_image())
    assert band_err(F.get_image(), x) <= RT[np.dtype(np.float32)]


# ---- one basis for the batch ----------------------------------------------------------------------------------------------------------------
def _patches(dt):
    """three 64 x 64 patches of a structured image with noise of sigma 2 (seed 5: the best-basis decisions below have margins of 1.3e-3 (l1)
    and 2.6e-3 (shannon) in tests/refwpt.py, in both precisions, so rounding cannot flip one)"""
    yy, xx = np.mgrid[0:128, 0:128].astype(np.float64)
    img = (50 * np.sin(2 * np.pi * 37 * xx / 128) + 0.2 * (xx + yy) + 30 * (np.hypot(xx - 40, yy - 70) < 20) + 2 * np.random.RandomState(5).randn(128, 128))
    return np.ascontiguousarray(np.stack([img[:64, :64], img[64:, :64], img[32:96, 64:]])).astype(dt)


@functools.lru_cache(maxsize=None)
def _patch_ref(dtname):
    x = _patches(np.dtype(dtname))
    trees = [R.tree(x[b], "db4", 3) for b in range(3)]
    x.setflags(write=False)
    return x, trees


def _summed(per):
    out = []
    for d in range(len(per[0])):
        s = np.zeros_like(per[0][d])
        for p in per:  # image order
            s = s + p[d]
        out.append(s)
    return out


@pytest.mark.parametrize("allow_fused", [True, False])
@pytest.mark.parametrize("dt", DTYPES)
def test_costs_best_basis_and_inverse_from_it(dt, allow_fused):
    dt = np.dtype(dt)
    x, trees = _patch_ref(dt.name)
    W = WaveletPacketBatch(x, "db4", 3, allow_fused=allow_fused)
    assert W.fused == allow_fused
    for kind in ("l1", "shannon"):
        W.set_image(x)  # a fresh tree per cost: inverse() below ends the previous one
        W.forward()
        lev = [W.get_level(d) for d in range(4)]
        # per-image and summed costs against the float64 costs of the nodes as downloaded
        per, summed = W.node_costs(kind, per_image=True), W.node_costs(kind)
        for d in range(4):
            assert per[d].shape == (3, 4 ** d) and summed[d].shape == (4 ** d,) and per[d].dtype == np.float64
            want = np.array([[R.cost(lev[d][b, i], kind) for i in range(4 ** d)] for b in range(3)])
            assert np.all(np.abs(per[d] - want) <= SUM_TOL * np.abs(want)), (kind, d)
            assert np.array_equal(summed[d], (per[d][0] + per[d][1]) + per[d][2]), (kind, d)  # added in image order on the host
        again_p, again_s = W.node_costs(kind, per_image=True), W.node_costs(kind)
        assert all(np.array_equal(a, b) for a, b in zip(again_p + again_s, per + summed))  # two runs: the same bits
        # ONE basis for the batch: the reference's search on the summed reference costs
        want, margin = R.best_basis(_summed([R.node_costs(t, kind) for t in trees]))
        assert margin >= 1e-6, margin
        assert tuple(sum(1 for d, _ in want if d == k) for k in range(4)) == (0, 1, 9, 12)
        assert W.best_basis(kind) == want == W.basis
        before = {d: _raw_level(W, d) for d in range(1, 4)}
        W.inverse()
        e = band_err(W.get_image(), x)
        print("%s %s fused=%d: inverse from the best basis %.3e" % (dt.name, kind, allow_fused, e))
        assert e <= RT[dt], (kind, e)
        after = {d: _raw_level(W, d) for d in range(1, 4)}
        for d, i in want:  # the nodes of the basis keep their bits on either path
            assert np.array_equal(before[d][:, i], after[d][:, i]), (kind, d, i)
        if allow_fused:  # the fused inverse writes the images only
            assert all(np.array_equal(before[d], after[d]) for d in range(1, 4))


@pytest.mark.parametrize("allow_fused", [True, False])
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("wname", ["db4", "haar"])
def test_hand_made_basis_with_a_zeroed_node(wname, dt, allow_fused):
    dt = np.dtype(dt)
    x = _patches(dt)
    trees = _patch_ref(dt.name)[1] if wname == "db4" else [R.tree(x[b], wname, 3) for b in range(3)]
    names = ["a", "ha", "hh", "hv", "hd", "v", "daa", "dah", "dav", "dad", "dh", "dv", "dd"]
    W = WaveletPacketBatch(x, wname, 3, allow_fused=allow_fused)
    W.forward()
    W.set_basis(names)
    assert W.basis == sorted(R.index_of(n) for n in names)
    W.set_node("v", np.zeros((3,) + W.node_shape(1), dt))
    assert W.state == W_THRESHOLD
    # every node outside the basis is poisoned: the inverse may read the basis only
    for d in range(1, 4):
        lev = _raw_level(W, d)
        for i in range(4 ** d):
            if (d, i) not in W.basis:
                lev[:, i] = np.nan
        assert pdwt_amd.hip().pdwt_memcpy_h2d(C.c_void_p(W.level_view(d).ptr), lev.ctypes.data_as(C.c_void_p), lev.nbytes) == 0
    before = {n: W.node_view(n).numpy() for n in names}
    assert not before["v"].any() and before["ha"].shape == (3,) + W.node_shape(2)
    W.inverse()
    got = W.get_image()
    for b in range(3):
        nodes = {R.index_of(n): np.array(trees[b][len(n)][R.index_of(n)[1]]) for n in names}
        nodes[(1, 2)][...] = 0
        want = R.inverse(nodes, (64, 64), wname, 3)
        assert band_err(got[b], want) <= FWD[dt], (wname, b)
    for n in names:
        assert np.array_equal(W.node_view(n).numpy(), before[n]), n


# ---- thresholds, statistics, sigma --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("kind,app", [("soft", 0), ("hard", 0), ("soft", 1)])
def test_thresholds_touch_exactly_the_basis(kind, app, dt):
    dt = np.dtype(dt)
    x = _patches(dt)
    names = ["a", "ha", "hh", "hv", "hd", "v", "daa", "dah", "dav", "dad", "dh", "dv", "dd"]
    W = WaveletPacketBatch(x, "db2", 3)
    W.forward()
    W.set_basis(names)
    before = {d: _raw_level(W, d) for d in range(0, 4)}
    getattr(W, kind + "_threshold")(4.0, do_thresh_appcoeffs=app)
    assert W.state == W_THRESHOLD
    after = {d: _raw_level(W, d) for d in range(0, 4)}
    basis = set(W.basis)
    for d in range(0, 4):
        for i in range(4 ** d):
            b, a = before[d][:, i], after[d][:, i]
            if (d, i) in basis and (i != 0 or app):
                assert not np.array_equal(a, b), (d, i)
                # (one subtraction per element: a few ulp allow for another association of it, as tests/test_wpt2d_gpu.py does)
                assert np.allclose(a, ref_threshold(b, 4.0, kind), rtol=1e-6 if dt == np.float32 else 1e-14, atol=0), (d, i)
            else:
                assert np.array_equal(a, b), (d, i)  # outside the basis, or the all-"a" node: the same bits
    per = np.array([sum(np.abs(after[d][b, i].astype(np.float64)).sum() for d, i in basis) for b in range(3)])
    assert np.all(np.abs(W.images_norm1() - per) <= SUM_TOL * per)
    assert abs(W.norm1() - per.sum()) <= SUM_TOL * per.sum()


@pytest.mark.parametrize("dt", DTYPES)
def test_node_stats_norms_and_sigma(dt):
    dt = np.dtype(dt)
    x = _patches(dt)
    W = WaveletPacketBatch(x, "db4", 3)
    W.forward()
    lev = {d: W.get_level(d) for d in range(0, 4)}
    want = np.abs(lev[3].astype(np.float64)).sum(axis=(1, 2, 3))
    assert np.all(np.abs(W.images_norm1() - want) <= SUM_TOL * want) and abs(W.norm1() - want.sum()) <= SUM_TOL * want.sum()
    for d in range(0, 4):
        s = W.node_stats(d)
        for key in ("sum_abs", "sum_sq", "max_abs"):
            assert s[key].shape == (3, 4 ** d)
            ref = np.array([[ref_stats(lev[d][b, i])[key] for i in range(4 ** d)] for b in range(3)])
            if key == "max_abs":
                assert np.array_equal(s[key], ref)
            else:
                assert np.all(np.abs(s[key] - ref) <= SUM_TOL * ref), (d, key)
    # selection does no arithmetic: the mean of the two middle order statistics of the node(s) as downloaded, in their own dtype
    node_d = W.get_node("d")
    assert node_d.shape == (3, 32, 32) and node_d.dtype == dt
    pooled = ref_stats(node_d)["median_abs"] / MAD_SCALE
    assert W.estimate_sigma() == pooled
    per = W.images_estimate_sigma()
    assert per.shape == (3,) and all(per[b] == ref_stats(node_d[b])["median_abs"] / MAD_SCALE for b in range(3))
    assert 1.0 < pooled < 4.0 and len(set(per)) == 3  # the images carry noise of sigma 2; the pooled median is not one of theirs by chance
    assert per.min() <= pooled <= per.max()


# ---- the rest -----------------------------------------------------------------------------------------------------------------------------
def test_one_image_replaced_through_set_image():
    x = _images((3, 37, 51), np.float32)
    W = WaveletPacketBatch(x, "db3", 2)
    W.forward()
    first = [W.get_level(d) for d in range(3)]
    y = x.copy()
    y[1] = _images((37, 51), np.float32, seed=4)
    W.set_image(y)
    assert W.state == W_INIT
    W.forward()
    for d in range(1, 3):
        lev = W.get_level(d)
        assert np.array_equal(lev[0], first[d][0]) and np.array_equal(lev[2], first[d][2]) and not np.array_equal(lev[1], first[d][1])
    S = WaveletPackets2D(y[1], "db3", 2)
    S.forward()
    assert np.array_equal(S.get_level(2), W.get_level(2)[1])


@pytest.mark.parametrize("allow_fused", [True, False])
def test_images_do_not_leak_into_each_other_through_the_wrap(allow_fused):
    """corner impulses in image 1 of three: everything near a corner comes through the periodic wrap of THAT image; its neighbours stay 0"""
    x = np.zeros((3, 40, 72), np.float32)
    x[1, 0, 0], x[1, -1, -1], x[1, 0, -1] = 100.0, -50.0, 25.0
    W = WaveletPacketBatch(x, "db4", 2, allow_fused=allow_fused)
    assert W.fused == allow_fused
    W.forward()
    tr = R.tree(x[1], "db4", 2)
    for d in range(1, 3):
        lev = W.get_level(d)
        assert not lev[0].any() and not lev[2].any(), d
        assert _depth_err(lev[1], tr[d]) <= FWD[np.dtype(np.float32)]
    W.inverse()
    rec = W.get_image()
    assert not rec[0].any() and not rec[2].any() and band_err(rec[1], x[1]) <= RT[np.dtype(np.float32)]


def test_state_machine_refusals_leave_the_data_alone():
    x = _images((2, 64, 64), np.float32)
    W = WaveletPacketBatch(x, "db2", 3)
    W.forward()
    W.inverse()
    assert W.state == W_INVERSE
    snap = {d: _raw_level(W, d) for d in range(0, 4)}
    for call in (lambda: W.get_node("a"), lambda: W.get_level(1), lambda: W.soft_threshold(1.0), lambda: W.hard_threshold(1.0),
                 lambda: W.best_basis("l1"), lambda: W.node_costs("l1"), lambda: W.norm1(), lambda: W.images_norm1(), lambda: W.node_stats(1),
                 lambda: W.estimate_sigma(), lambda: W.images_estimate_sigma()):
        with pytest.raises(RuntimeError):
            call()
    with pytest.raises(RuntimeError):  # no node may be replaced either
        W.set_node("a", np.zeros((2,) + W.node_shape(1), np.float32))
    W.inverse()  # refused with a warning
    assert W.state == W_INVERSE
    assert all(np.array_equal(snap[d], _raw_level(W, d)) for d in range(0, 4))
    W.set_image(x)
    assert W.state == W_INIT
    with pytest.raises(RuntimeError):  # no forward() yet
        W.set_node("a", np.zeros((2,) + W.node_shape(1), np.float32))
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


def test_bases_bad_arguments_and_creation_errors():
    x = _images((2, 64, 64), np.float32)
    W = WaveletPacketBatch(x, "db2", 2)
    W.forward()
    for bad in (["a", "h", "v"], ["a", "h", "v", "d", "ah"], ["a", "a", "h", "v", "d"], ["aaa"], [(1, 4)], ["ax"]):
        with pytest.raises(ValueError):
            W.set_basis(bad)
    assert W.basis == [(2, i) for i in range(16)]
    W.set_basis([""])
    assert W.basis == [(0, 0)]
    W.inverse()  # nothing to synthesise
    assert np.array_equal(W.get_image(), x)
    with pytest.raises(ValueError):
        W.node_costs("l2")
    with pytest.raises(ValueError):
        W.best_basis("entropy")
    with pytest.raises(IndexError):
        W.node_view("aaa")
    with pytest.raises(ValueError):
        WaveletPacketBatch(np.zeros((8, 8), np.float32), "db2", 1)
    assert WaveletPacketBatch(x, "nosuchwavelet", 2).state == W_CREATION_ERROR
    E = WaveletPacketBatch(_images((2, 6, 64), np.float32), "db4", 2)  # ilog2(6 / 7) = 0 levels
    assert E.state == W_CREATION_ERROR and not E.fused
    E.forward()
    E.inverse()
    assert E.state == W_CREATION_ERROR
    with pytest.raises(RuntimeError):
        E.get_node("a")


@pytest.mark.parametrize("dt", DTYPES)
def test_device_tensors_and_zero_copy_views(dt):
    import torch
    x = _images((3, 61, 67), dt)
    t = torch.as_tensor(x, device="cuda")
    W = WaveletPacketBatch(t, "db2", 2)
    H = WaveletPacketBatch(x, "db2", 2)
    assert W.dtype == np.dtype(dt) and W.shape == (3, 61, 67)
    W.forward()
    H.forward()
    assert all(np.array_equal(W.get_level(d), H.get_level(d)) for d in range(3))
    v = W.node_view("hd")
    isz = np.dtype(dt).itemsize
    assert v.ptr == W.node_int_ptr("hd") == W.node_int_ptr((2, 7)) and v.shape == (3,) + W.node_shape(2) and v.pitch == W.node_pitch("hd") == 16 * 16 * 17
    assert v.ptr == W.node_int_ptr((2, 0)) + 7 * 16 * 17 * isz
    W.sync()
    assert np.array_equal(v.numpy(), W.get_node("hd"))
    tv = torch.as_tensor(v, device="cuda")  # a strided tensor over the node itself
    assert tv.data_ptr() == v.ptr and tuple(tv.stride()) == (v.pitch, 17, 1) and np.array_equal(tv.cpu().numpy(), W.get_node("hd"))
    tv.zero_()  # a write through the view lands in the node of every image, and nowhere else
    torch.cuda.synchronize()
    lev = W.get_level(2)
    assert not lev[:, 7].any() and np.array_equal(np.delete(lev, 7, axis=1), np.delete(H.get_level(2), 7, axis=1))
    W.set_node("hd", torch.as_tensor(H.get_node("hd"), device="cuda"))
    assert np.array_equal(W.get_level(2), H.get_level(2)) and W.state == W_THRESHOLD
    lv = W.level_view(1)
    assert isinstance(lv, DeviceArray) and lv.shape == (3, 4, 31, 34) and np.array_equal(lv.numpy(), W.get_level(1))
    W.set_image(torch.as_tensor(x[::-1].copy(), device="cuda"))
    assert np.array_equal(W.get_image(), x[::-1])
    with pytest.raises(TypeError):
        WaveletPacketBatch(t, "db2", 2, dtype=np.float64 if dt == np.float32 else np.float32)
