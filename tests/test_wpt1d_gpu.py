"""WaveletPackets1D on the GPU against tests/refwpt1d.py (the oracle's one-level batched 1-D transform applied to every node again, in
the precision under test).

Metric: tests/helpers.band_err per NODE, taken over all rows of that node (max |got - ref| / max |ref|).  Bounds, those of
tests/test_wpt2d_gpu.py: 1e-5 (float32) and 1e-12 (float64) for every node of every depth; 10x those for round trips.  (The float32
reference differs from the float64 one by at most 4.8e-7 on these cases, a twentieth of the bound.)  So that the per-node normalisation
hides nothing, the smallest node maximum of a depth must be at least 0.05 of the largest: asserted on the reference for the uniform
inputs (0.094 for (5, 77) haar, 0.128 for (4, 200) bior2.2, at least 0.2 elsewhere; a single row at depth 12 would fail it -- nodes of
one sample -- which is why the deep case has 64 rows).

Largest errors measured on an MI355X (one run; the GPU runs the oracle's operations in the oracle's order):
forward 0 in every case of CASES in both precisions and on both inputs; round trips at most 6.1e-7 (float32) and 1.1e-12 (float64,
sym8: the defect of the table's bank; 3.2e-15 otherwise).
"""
import ctypes as C
import functools

import numpy as np
import pytest

import pdwt_amd
from pdwt_amd import DeviceArray, Wavelets, WaveletPackets1D
from pdwt_amd import _native as nat
from pdwt_amd import wpt
from pdwt_amd.wavelets import W_CREATION_ERROR, W_FORWARD, W_INIT, W_INVERSE, W_THRESHOLD
from tests import refwpt1d as R
from tests.helpers import band_err
from tests.refstats import ref_stats

pytestmark = pytest.mark.gpu

FWD = {np.dtype(np.float32): 1e-5, np.dtype(np.float64): 1e-12}
RT = {k: 10 * v for k, v in FWD.items()}
SUM_TOL = 1e-10  # sums accumulated in double (tests/test_wpt2d_gpu.py)
DTYPES = [np.float32, np.float64]
# (Nr, Nc, bank, asked): the clamped depth and what each case exercises are listed in tests/test_wpt1d_cpu.py / DESIGN.md 3.15
CASES = [(3, 64, "db2", 4), (5, 77, "haar", 9), (300, 33, "db2", 3), (2, 1000, "sym8", 9), (7, 96, "db4", 3), (4, 200, "bior2.2", 9),
         (2, 640, "db20", 9), (2, 1031, "db3", 9), (6, 48, "coif1", 9), (64, 4096, "haar", 12)]
IDS = ["%dx%d-%s" % c[:3] for c in CASES]


def _structured(nr=6, nc=512):
    """a chirp plus two tones plus noise (seed 5) plus five spikes, a different mix per row: the tones favour deep nodes, the spikes
    shallow ones, so the best basis is of mixed depth (7 to 9 nodes; smallest decision margin of the reference 5.8e-5)"""
    t = np.arange(nc) / nc
    rs = np.random.RandomState(5)
    rows = []
    for r in range(nr):
        x = 40 * np.sin(2 * np.pi * (3 + r) * t * t * 4) + 25 * np.sin(2 * np.pi * (11 + r) * t) + 12 * np.sin(2 * np.pi * (23 + 2 * r) * t + r) + 0.5 * rs.randn(nc)
        pos = rs.choice(nc, 5, replace=False)
        x[pos] += rs.choice([-1, 1], 5) * rs.uniform(60, 120, 5)
        rows.append(x)
    return np.stack(rows)


@functools.lru_cache(maxsize=None)
def _ref(nr, nc, wname, levels, dtname, kind="uniform"):
    """(batch, reference tree): computed once per case and shared; callers do not modify them"""
    dt = np.dtype(dtname)
    if kind == "uniform":
        x = np.random.RandomState(1).uniform(-100, 100, (nr, nc)).astype(dt)
    elif kind == "ramp":  # wraps every 37 samples, another phase per row
        rr, cc = np.mgrid[0:nr, 0:nc]
        x = (((cc + 5 * rr) % 37) * 2.5 - 40.0).astype(dt)
    elif kind == "impulse":  # zero but for the two ends of ONE row of a pack
        x = np.zeros((nr, nc), dt)
        x[nr // 2, 0], x[nr // 2, -1] = 100.0, -50.0
    else:
        x = _structured(nr, nc).astype(dt)
    # (depth 12 has 4096 nodes of one sample per row: the numpy restatement of the Haar tree, pinned to the oracle bit for bit on the CPU)
    tr = R.haar_tree(x, levels) if (wname == "haar" and levels >= 8) else R.tree(x, wname, levels)
    for t in tr:
        t.setflags(write=False)
    x.setflags(write=False)
    return x, tr


def _level_err(got, ref):
    """the largest band_err over the nodes of one depth, each node over all its rows (vectorised: depth 12 has 4096 nodes)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    den = np.abs(ref).max(axis=(0, 2))
    num = np.abs(got - ref).max(axis=(0, 2))
    return float((num / np.where(den > 0, den, 1.0)).max())


def _raw_level(W, depth):
    """the whole allocation of a depth read straight from device memory, whatever the state"""
    W.sync()
    nr, n = W.node_shape(depth)
    return DeviceArray(W, W.node_int_ptr((depth, 0)), (nr, 2 ** depth, n), W.dtype).numpy()


def _check_tree(W, tr, bound, what):
    assert W.levels == len(tr) - 1, (what, W.levels)
    worst = 0.0
    for d in range(W.levels + 1):
        assert W.node_shape(d) == (tr[d].shape[0], tr[d].shape[2]), (what, d)
        e = _level_err(W.get_level(d), tr[d])
        worst = max(worst, e)
        assert e <= bound, (what, d, e)
    print("%s: %d depths, largest node err %.3e" % (what, W.levels, worst))


# ---- forward and round trip ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["uniform", "ramp"])
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("nr,nc,wname,asked", CASES, ids=IDS)
def test_forward_every_node_and_round_trip(nr, nc, wname, asked, dt, kind):
    x, tr = _ref(nr, nc, wname, asked, np.dtype(dt).name, kind)
    if kind == "uniform":  # the normalisation hides nothing: no node of a depth is small against the others
        for t in tr[1:]:
            mx = np.abs(t).max(axis=(0, 2))
            assert mx.min() >= 0.05 * mx.max(), (wname, mx.min() / mx.max())
    W = WaveletPackets1D(x, wname, asked)
    assert W.state == W_INIT and W.dtype == np.dtype(dt) and W.fused
    W.forward()
    assert W.state == W_FORWARD
    _check_tree(W, tr, FWD[np.dtype(dt)], "%dx%d %s %s %s" % (nr, nc, wname, np.dtype(dt).name, kind))
    assert np.array_equal(W.get_image(), x)  # forward() leaves the batch intact
    L = W.levels
    assert W.basis == [(L, i) for i in range(2 ** L)]
    for path in ("a", "d", "da"[:L], "d" * L, "a" * L):
        d, i = R.index_of(path)
        node = W.get_node(path)
        assert np.array_equal(node, W.get_level(d)[:, i]) and np.array_equal(W.get_node((d, i)), node)
    W.inverse()
    assert W.state == W_INVERSE
    e = band_err(W.get_image(), x)
    print("round trip %.3e" % e)
    assert e <= RT[np.dtype(dt)], e


# ---- against the existing transform ------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("nr,nc,wname,asked", [CASES[k] for k in (0, 1, 3, 5, 7)], ids=[IDS[k] for k in (0, 1, 3, 5, 7)])
def test_all_a_path_is_the_ordinary_transform(nr, nc, wname, asked, dt):
    x, _ = _ref(nr, nc, wname, asked, np.dtype(dt).name)
    P = WaveletPackets1D(x, wname, asked)
    L = P.levels
    W = Wavelets(x, wname, L, ndim=1)
    P.forward()
    W.forward()
    assert W.info.nlevels == L
    bands, bound = W.coeffs, FWD[np.dtype(dt)]  # [A_L, D_1, ..., D_L]
    assert band_err(P.get_node("a" * L), bands[0]) <= bound
    for k in range(1, L + 1):
        assert band_err(P.get_node("a" * (k - 1) + "d"), bands[k]) <= bound, k


# ---- both kernel forms give the same bits ----------------------------------------------------------------
class _Dev:
    """a device buffer of the library's allocator holding `arr` (or `n` elements of zeros)"""

    def __init__(self, arr=None, n=0, dt=np.float32):
        self.L = pdwt_amd.hip()
        host = np.ascontiguousarray(arr) if arr is not None else np.zeros(n, dt)
        self.shape, self.dtype, self.nbytes = host.shape, host.dtype, max(host.nbytes, 1)
        self.ptr = self.L.pdwt_malloc(self.nbytes)
        assert self.ptr
        assert self.L.pdwt_memcpy_h2d(self.ptr, host.ctypes.data_as(C.c_void_p), host.nbytes) == 0

    def numpy(self):
        out = np.empty(self.shape, self.dtype)
        assert self.L.pdwt_memcpy_d2h(out.ctypes.data_as(C.c_void_p), self.ptr, out.nbytes) == 0
        return out

    def free(self):
        self.L.pdwt_free(self.ptr)


def _bank(wname, dt):
    sfx, FT = ("f32", nat.Filters32) if np.dtype(dt) == np.float32 else ("f64", nat.Filters64)
    f = FT()
    h = getattr(pdwt_amd.hip(), "pdwt_compute_filters_separable_" + sfx)(wname.encode(), 0, C.byref(f))
    assert h >= 2
    f.hlen = h
    return sfx, f


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("nr,nc,wname,asked", [CASES[k] for k in (1, 2, 3, 6, 7)], ids=[IDS[k] for k in (1, 2, 3, 6, 7)])
def test_both_kernel_forms_give_the_same_bits(nr, nc, wname, asked, dt):
    x, _ = _ref(nr, nc, wname, asked, np.dtype(dt).name)
    W = WaveletPackets1D(x, wname, asked)
    assert W.fused
    W.forward()
    L, H = W.levels, pdwt_amd.hip()
    want = [W.get_level(d) for d in range(L + 1)]
    sfx, f = _bank(wname, dt)
    n = R.lengths(nc, L)
    bufs = [_Dev(x)] + [_Dev(n=nr * 2 ** d * n[d], dt=dt) for d in range(1, L + 1)]
    try:
        for d in range(L):  # the tree composed from the level entries
            assert getattr(H, "pdwt_wp1_forward_level_" + sfx)(bufs[d].ptr, bufs[d + 1].ptr, nr, 2 ** d, n[d], C.byref(f)) == 0
        H.pdwt_sync()
        for d in range(1, L + 1):
            assert np.array_equal(bufs[d].numpy().reshape(want[d].shape), want[d]), d
        for d in range(L - 1, -1, -1):  # the inverse from depth L composed from the level entries
            assert getattr(H, "pdwt_wp1_inverse_level_" + sfx)(bufs[d].ptr, bufs[d + 1].ptr, nr, 2 ** d, n[d], None, 0, C.byref(f)) == 0
        H.pdwt_sync()
        W.inverse()
        assert np.array_equal(bufs[0].numpy(), W.get_image())
    finally:
        for b in bufs:
            b.free()


# ---- both sides of the LDS budget ------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_both_sides_of_the_budget(dt):
    H, elem = pdwt_amd.hip(), np.dtype(dt).itemsize
    lo, hi = 1000, 2 ** 20
    assert H.pdwt_wp1_fused(lo, 8, 3, elem) == 1 and H.pdwt_wp1_fused(hi, 8, 3, elem) == 0
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if H.pdwt_wp1_fused(mid, 8, 3, elem) == 1 else (lo, mid)
    print("largest fused row, db4 %s, 3 levels: %d samples" % (np.dtype(dt).name, lo))
    for nc, fused in ((lo, True), (lo + 1, False)):
        x, tr = _ref(2, nc, "db4", 3, np.dtype(dt).name)
        W = WaveletPackets1D(x, "db4", 3)
        assert W.fused == fused and W.levels == 3
        W.forward()
        _check_tree(W, tr, FWD[np.dtype(dt)], "2x%d db4 %s (%s)" % (nc, np.dtype(dt).name, "fused" if fused else "per level"))
        W.inverse()
        assert band_err(W.get_image(), x) <= RT[np.dtype(dt)]


# ---- no leak between packed rows or between nodes ----------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("nr,nc,wname,asked", [(16, 33, "db2", 3), (24, 64, "db4", 3), (9, 77, "haar", 6)])
def test_no_leak_between_packed_rows(nr, nc, wname, asked, dt):
    x, tr = _ref(nr, nc, wname, asked, np.dtype(dt).name, "impulse")
    hit = nr // 2
    W = WaveletPackets1D(x, wname, asked)
    W.forward()
    for d in range(1, W.levels + 1):
        got = W.get_level(d)
        others = np.delete(got, hit, axis=0)
        assert not others.any(), d  # exactly 0 in every other row's nodes
        assert _level_err(got[hit:hit + 1], tr[d][hit:hit + 1]) <= FWD[np.dtype(dt)], d
    W.inverse()
    assert band_err(W.get_image(), x) <= RT[np.dtype(dt)]


# ---- inverse from bases, costs --------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("wname", ["db4", "haar"])
def test_costs_best_basis_and_inverse_from_it(wname, dt):
    x, tr = _ref(6, 512, wname, 4, np.dtype(dt).name, "structured")
    W = WaveletPackets1D(x, wname, 4)
    assert W.levels == 4 and W.fused
    for kind in ("l1", "shannon"):
        W.set_image(x)  # a fresh tree per cost: inverse() below ends the previous one
        W.forward()
        ref, ref_rows = R.node_costs(tr, kind), R.node_costs(tr, kind, per_row=True)
        got, got_rows = W.node_costs(kind), W.node_costs(kind, per_row=True)
        assert len(got) == 5 and all(g.dtype == np.float64 and g.shape == r.shape for g, r in zip(got, ref))
        assert all(g.shape == r.shape for g, r in zip(got_rows, ref_rows))
        rel = max(float((np.abs(g - r) / np.abs(r)).max()) for g, r in zip(got + got_rows, ref + ref_rows))
        print("%s %s %s: node costs rel %.3e" % (wname, np.dtype(dt).name, kind, rel))
        assert rel <= SUM_TOL, (kind, rel)
        again = W.node_costs(kind) + W.node_costs(kind, per_row=True)
        assert all(np.array_equal(a, g) for a, g in zip(again, got + got_rows))  # fixed order of combination: the same bits
        want, margin = R.best_basis(ref)
        print("%s %s %s: best basis of %d nodes, smallest decision margin %.3e" % (wname, np.dtype(dt).name, kind, len(want), margin))
        assert margin >= 1e-6  # double-accumulated costs (rel 1e-10) cannot flip a decision
        assert 1 < len(want) < 16 and len({d for d, _ in want}) > 1  # a basis of mixed depth
        basis = W.best_basis(kind)
        assert basis == want == W.basis
        before = {d: _raw_level(W, d) for d in range(1, 5)}
        W.inverse()
        e = band_err(W.get_image(), x)
        print("%s %s %s: inverse from the best basis %.3e" % (wname, np.dtype(dt).name, kind, e))
        assert e <= RT[np.dtype(dt)], (kind, e)
        after = {d: _raw_level(W, d) for d in range(1, 5)}
        for d in range(1, 5):  # the fused inverse writes the rows only: every depth keeps its bits, the basis nodes among them
            assert np.array_equal(before[d], after[d]), (kind, d)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("wname", ["db2", "db4", "haar"])
def test_hand_made_basis_with_a_zeroed_node(wname, dt):
    x, tr = _ref(6, 512, wname, 4, np.dtype(dt).name, "structured")
    names = ["aa", "ada", "adda", "addd", "da", "dd"]
    W = WaveletPackets1D(x, wname, 4)
    W.forward()
    W.set_basis(names)
    assert W.basis == sorted(R.index_of(n) for n in names)
    W.set_node("da", np.zeros(W.node_shape(2), dt))
    assert W.state == W_THRESHOLD
    nodes = {R.index_of(n): np.array(tr[len(n)][:, R.index_of(n)[1]]) for n in names}
    nodes[(2, 2)][...] = 0
    want = R.inverse(nodes, x.shape, wname, 4)
    before = {n: W.node_view(n).numpy() for n in names}
    assert not before["da"].any() and np.array_equal(before["dd"], tr[2][:, 3])
    W.inverse()
    assert band_err(W.get_image(), want) <= FWD[np.dtype(dt)]
    for n in names:
        assert np.array_equal(W.node_view(n).numpy(), before[n]), n


def test_inverse_per_level_path_from_a_mixed_basis():
    """rows too long for LDS: one launch per depth under the same state table; parents are written to their own storage"""
    H = pdwt_amd.hip()
    nc = 24000
    assert H.pdwt_wp1_fused(nc, 8, 3, 4) == 0
    x, tr = _ref(2, nc, "db4", 3, "float32")
    W = WaveletPackets1D(x, "db4", 3)
    assert not W.fused
    W.forward()
    names = ["aa", "ad", "d"]
    W.set_basis(names)
    nodes = {R.index_of(n): tr[len(n)][:, R.index_of(n)[1]] for n in names}
    want = R.inverse(nodes, x.shape, "db4", 3)
    before = {n: W.node_view(n).numpy() for n in names}
    W.inverse()
    assert band_err(W.get_image(), want) <= FWD[np.dtype(np.float32)]
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
    x, _ = _ref(6, 512, "db2", 4, np.dtype(dt).name, "structured")
    names = ["aaa", "aad", "ad", "daa", "dada", "dadd", "dd"]
    W = WaveletPackets1D(x, "db2", 4)
    W.forward()
    W.set_basis(names)
    before = {d: _raw_level(W, d) for d in range(0, 5)}
    getattr(W, kind + "_threshold")(4.0, do_thresh_appcoeffs=app)
    assert W.state == W_THRESHOLD
    after = {d: _raw_level(W, d) for d in range(0, 5)}
    basis = set(W.basis)
    assert basis == {R.index_of(n) for n in names}
    for d in range(0, 5):
        for i in range(2 ** d):
            b, a = before[d][:, i], after[d][:, i]
            if (d, i) in basis and (i != 0 or app):
                want = _thresh(b, 4.0, kind)
                assert not np.array_equal(a, b), (d, i)
                assert np.allclose(a, want, rtol=1e-6 if dt == np.float32 else 1e-14, atol=0), (d, i)
            else:
                assert np.array_equal(a, b), (d, i)  # outside the basis, or the all-"a" node: the same bits
    want = sum(np.abs(after[d][:, i].astype(np.float64)).sum() for d, i in basis)
    assert abs(W.norm1() - want) <= SUM_TOL * want


@pytest.mark.parametrize("dt", DTYPES)
def test_norm1_node_stats_and_sigma(dt):
    x, _ = _ref(6, 512, "db4", 4, np.dtype(dt).name, "structured")
    W = WaveletPackets1D(x, "db4", 4)
    W.forward()
    lev = {d: W.get_level(d).astype(np.float64) for d in range(0, 5)}
    want = np.abs(lev[4]).sum()
    assert abs(W.norm1() - want) <= SUM_TOL * want
    W.best_basis("l1")
    want = sum(np.abs(lev[d][:, i]).sum() for d, i in W.basis)
    assert abs(W.norm1() - want) <= SUM_TOL * want
    for d in range(0, 5):
        s = W.node_stats(d)
        flat = np.moveaxis(lev[d], 1, 0).reshape(2 ** d, -1)
        assert np.all(np.abs(s["sum_abs"] - np.abs(flat).sum(axis=1)) <= SUM_TOL * np.abs(flat).sum(axis=1))
        assert np.all(np.abs(s["sum_sq"] - (flat * flat).sum(axis=1)) <= SUM_TOL * (flat * flat).sum(axis=1))
        assert np.array_equal(s["max_abs"], np.abs(flat).max(axis=1))
    # selection does no arithmetic: equal to the mean of the two middle order statistics of the node as downloaded, in its own dtype
    node_d = W.get_node("d")
    assert node_d.dtype == np.dtype(dt)
    st = ref_stats(node_d)
    sig = st["median_abs"] / 0.6744897501960817
    assert st["median_abs"] == float(np.median(np.abs(node_d).astype(np.float64)))
    assert W.estimate_sigma() == sig, (W.estimate_sigma(), sig)


# ---- frequency order ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTYPES)
def test_frequency_order_on_the_gpu(dt):
    """get_level(order="freq") is the Gray permutation of the natural one, and a sinusoid at the centre of band r puts its energy
    maximum on rank r"""
    n, depth = 1024, 4
    nb, t = 2 ** depth, np.arange(1024)
    rows = np.stack([np.sin(2 * np.pi * (r + 0.5) / (2.0 * nb) * t + 0.3) for r in range(nb)]).astype(dt)
    for wname in ("sym8", "db4", "haar"):
        W = WaveletPackets1D(rows, wname, depth)
        W.forward()
        nat_, frq = W.get_level(depth), W.get_level(depth, order="freq")
        assert frq.shape == nat_.shape and frq.flags["C_CONTIGUOUS"]
        assert np.array_equal(frq, nat_[:, wpt.frequency_order(depth)])
        energy = (frq.astype(np.float64) ** 2).sum(axis=2)  # (row = the band the sinusoid sits in, rank)
        assert list(np.argmax(energy, axis=1)) == list(range(nb)), wname
        with pytest.raises(ValueError):
            W.get_level(depth, order="paley")


# ---- state machine and errors -----------------------------------------------------------------------------
def test_state_machine_refusals_leave_the_data_alone():
    x, _ = _ref(3, 64, "db2", 4, "float32")
    W = WaveletPackets1D(x, "db2", 3)
    W.forward()
    W.inverse()
    assert W.state == W_INVERSE
    snap = {d: _raw_level(W, d) for d in range(0, 4)}
    for call in (lambda: W.get_node("a"), lambda: W.get_level(1), lambda: W.soft_threshold(1.0), lambda: W.hard_threshold(1.0),
                 lambda: W.best_basis("l1"), lambda: W.node_costs("l1"), lambda: W.norm1(), lambda: W.node_stats(1), lambda: W.estimate_sigma()):
        with pytest.raises(RuntimeError):
            call()
    with pytest.raises(RuntimeError):  # no node may be replaced after inverse() either
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
        W.set_basis(["a", "d"])
    assert W.basis == basis and all(np.array_equal(snap[d], _raw_level(W, d)) for d in range(0, 4))
    W.inverse()  # thresholded coefficients may of course be inverted
    assert W.state == W_INVERSE


def test_set_basis_errors_and_bad_arguments():
    x, _ = _ref(3, 64, "db2", 4, "float32")
    W = WaveletPackets1D(x, "db2", 2)
    W.forward()
    for bad in (["a"], ["a", "d", "aa"], ["a", "a", "d"], ["aaa"], [(1, 2)], ["ah"]):
        with pytest.raises(ValueError):
            W.set_basis(bad)
    assert W.basis == [(2, i) for i in range(4)]
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
    with pytest.raises(IndexError):
        W.node_shape(3)
    with pytest.raises(ValueError):
        WaveletPackets1D(np.zeros((4, 8, 8), np.float32), "db2", 1)
    with pytest.raises(ValueError):
        WaveletPackets1D(np.zeros(64, np.float32), "db2", 1)


def test_creation_errors_and_clamps():
    assert WaveletPackets1D(np.zeros((4, 64), np.float32), "nosuchwavelet", 2).state == W_CREATION_ERROR
    W = WaveletPackets1D(np.zeros((64, 6), np.float32), "db4", 2)  # ilog2(6 / 7) = 0 levels, however many rows
    assert W.state == W_CREATION_ERROR and not W.fused
    W.forward()
    W.inverse()
    assert W.state == W_CREATION_ERROR
    with pytest.raises(RuntimeError):
        W.get_node("a")
    assert WaveletPackets1D(np.zeros((2, 96), np.float32), "db4", 9).levels == 3
    assert WaveletPackets1D(np.zeros((2, 96), np.float32), "db4", 0).levels == 1
    W = WaveletPackets1D(np.zeros((1, 2 ** 14), np.float32), "haar", 20)
    assert W.levels == 12 and W.node_shape(12) == (1, 4)


@pytest.mark.parametrize("dt", DTYPES)
def test_device_tensors_and_zero_copy_views(dt):
    import torch
    x, _ = _ref(7, 96, "db4", 3, np.dtype(dt).name)
    t = torch.as_tensor(np.array(x), device="cuda")
    W = WaveletPackets1D(t, "db4", 3)
    H = WaveletPackets1D(x, "db4", 3)
    assert W.dtype == np.dtype(dt) and W.shape == (7, 96)
    W.forward()
    H.forward()
    assert all(np.array_equal(W.get_level(d), H.get_level(d)) for d in range(4))
    v = W.node_view("da")
    isz = np.dtype(dt).itemsize
    assert v.ptr == W.node_int_ptr("da") == W.node_int_ptr((2, 2)) and v.shape == W.node_shape(2) == (7, 24)
    assert v.pitch == W.node_pitch("da") == 4 * 24 and v.ptr == W.node_int_ptr((2, 0)) + 2 * 24 * isz
    assert v.__cuda_array_interface__["strides"] == (4 * 24 * isz, isz)
    W.sync()
    tv = torch.as_tensor(v, device="cuda")
    assert tv.data_ptr() == v.ptr and tuple(tv.stride()) == (96, 1) and np.array_equal(tv.cpu().numpy(), W.get_node("da"))
    assert np.array_equal(v.numpy(), W.get_node("da"))
    tv.zero_()  # a write through the view lands in the node, and only there
    torch.cuda.synchronize()
    assert not W.get_node("da").any()
    assert np.array_equal(W.get_node("dd"), H.get_node("dd")) and np.array_equal(W.get_node("ad"), H.get_node("ad"))
    W.set_node("da", torch.as_tensor(H.get_node("da"), device="cuda"))
    assert np.array_equal(W.get_level(2), H.get_level(2)) and W.state == W_THRESHOLD
    W.set_image(torch.as_tensor(np.array(x[::-1]), device="cuda"))
    assert np.array_equal(W.get_image(), x[::-1])
    with pytest.raises(TypeError):
        WaveletPackets1D(t, "db4", 3, dtype=np.float64 if dt == np.float32 else np.float32)
