"""The batched 1-D wavelet packet entries of the C ABI (pdwt_wp1_forward_level_* / pdwt_wp1_inverse_level_*, the whole-transform
pdwt_wp1_forward_* / pdwt_wp1_inverse_*, pdwt_wp1_moments_* and pdwt_wp1_thresh_*) on buffers of a CALLER: every buffer guarded on
both sides and misaligned down to its element size (tests/cabi_arena.py), both precisions.  After each call: the return code, no byte
outside a payload and no byte of a read-only payload changed, every output fully overwritten (no NaN of the fill left) and the values
within the bounds of tests/test_wpt1d_gpu.py of tests/refwpt1d.py.  Every PDWT_EINVAL case touches nothing."""
import ctypes as C

import numpy as np
import pytest

import pdwt_amd
from pdwt_amd import _native as nat
from tests import refwpt1d as R
from tests.cabi_arena import Arena, Region
from tests.helpers import band_err

pytestmark = pytest.mark.gpu

FWD = {"f32": 1e-5, "f64": 1e-12}


def _setup(wname, sfx):
    L = pdwt_amd.hip()
    dt = np.dtype(np.float32 if sfx == "f32" else np.float64)
    f = (nat.Filters32 if sfx == "f32" else nat.Filters64)()
    hlen = getattr(L, "pdwt_compute_filters_separable_" + sfx)(wname.encode(), 0, C.byref(f))
    assert hlen > 0
    f.hlen = hlen
    return L, dt, f, hlen


def _node_err(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    den = np.abs(ref).max(axis=(0, 2))
    return float((np.abs(got - ref).max(axis=(0, 2)) / np.where(den > 0, den, 1.0)).max())


def _state_table(L, levels, basis):
    d, i = (C.c_int * len(basis))(*[v[0] for v in basis]), (C.c_int * len(basis))(*[v[1] for v in basis])
    out = (C.c_ubyte * 2 ** (levels + 1))()
    assert L.pdwt_wp1_state_table(levels, d, i, len(basis), out) == 0
    return np.frombuffer(out, np.uint8).copy()


@pytest.mark.parametrize("sfx", ["f32", "f64"])
@pytest.mark.parametrize("nr,nc,wname", [(5, 77, "haar"), (3, 4201, "db4")])
def test_level_entries_on_guarded_misaligned_buffers(nr, nc, wname, sfx):
    """one step from depth 1 to depth 2 (two parents per row); (3, 4201) db4: parents of 2101 samples, two tiles each way, the second partial"""
    L, dt, f, hlen = _setup(wname, sfx)
    x = np.random.RandomState(3).uniform(-100, 100, (nr, nc)).astype(dt)
    tr = R.tree(x, wname, 2)
    n1, n2 = tr[1].shape[2], tr[2].shape[2]
    nan = np.full(tr[2].shape, np.nan, dt)
    A = Arena(L, [Region("par", tr[1].size, dt, "in", 1), Region("kid", tr[2].size, dt, "out", 3), Region("list", 4, np.int32, "in", 1)],
              {"par": tr[1], "kid": nan, "list": np.array([1, 0, 0, 0], np.int32)})
    fwd, inv = getattr(L, "pdwt_wp1_forward_level_" + sfx), getattr(L, "pdwt_wp1_inverse_level_" + sfx)
    par, kid, lst = A.ptr("par"), A.ptr("kid"), A.ptr("list")
    try:
        # refusals first: nothing may be touched
        assert fwd(None, kid, nr, 2, n1, C.byref(f)) == -1 and fwd(par, None, nr, 2, n1, C.byref(f)) == -1 and fwd(par, kid, nr, 2, n1, None) == -1
        assert fwd(par, kid, 0, 2, n1, C.byref(f)) == -1 and fwd(par, kid, nr, 0, n1, C.byref(f)) == -1 and fwd(par, kid, nr, 2, 0, C.byref(f)) == -1
        assert fwd(par, kid, nr, 4097, n1, C.byref(f)) == -1 and fwd(par, kid, 1 << 16, 2, 1 << 15, C.byref(f)) == -1
        assert inv(None, kid, nr, 2, n1, None, 0, C.byref(f)) == -1 and inv(par, None, nr, 2, n1, None, 0, C.byref(f)) == -1
        assert inv(par, kid, nr, 2, n1, lst, 0, C.byref(f)) == -1 and inv(par, kid, nr, 2, n1, lst, 3, C.byref(f)) == -1
        assert inv(par, kid, nr, 2, n1, None, 0, None) == -1 and inv(par, kid, 0, 2, n1, None, 0, C.byref(f)) == -1
        A.by_name["kid"].role = "in"
        A.check("refusals %s %s" % (wname, sfx))
        A.by_name["kid"].role = "out"
        assert fwd(par, kid, nr, 2, n1, C.byref(f)) == 0
        image = A.check("forward level %s %s" % (wname, sfx))
        got = A.get(image, "kid", shape=tr[2].shape)
        assert not np.isnan(got).any()  # fully overwritten
        e = _node_err(got, tr[2])
        print("%s %s forward level: %.3e" % (wname, sfx, e))
        assert e <= FWD[sfx], e
        # inverse of parent 1 alone (the list), then of both, from the reference children into parents of NaN
        A.by_name["par"].role, A.by_name["kid"].role = "out", "in"
        A.upload("kid", tr[2])
        A.upload("par", np.full(tr[1].shape, np.nan, dt))
        assert inv(par, kid, nr, 2, n1, lst, 1, C.byref(f)) == 0
        image = A.check("inverse level, one parent %s %s" % (wname, sfx))
        got = A.get(image, "par", shape=tr[1].shape)
        assert np.isnan(got[:, 0]).all() and not np.isnan(got[:, 1]).any()  # parent 0 untouched
        assert band_err(got[:, 1], tr[1][:, 1]) <= 10 * FWD[sfx]
        assert inv(par, kid, nr, 2, n1, None, 0, C.byref(f)) == 0
        image = A.check("inverse level %s %s" % (wname, sfx))
        got = A.get(image, "par", shape=tr[1].shape)
        assert not np.isnan(got).any()
        e = _node_err(got, tr[1])
        print("%s %s inverse level: %.3e" % (wname, sfx, e))
        assert e <= 10 * FWD[sfx], e
        assert n2 == (n1 + 1) // 2
    finally:
        A.free()


@pytest.mark.parametrize("sfx", ["f32", "f64"])
@pytest.mark.parametrize("nr,nc,wname,levels,fused", [(21, 33, "db2", 3, 1), (2, 4099, "db4", 4, 1), (2, 24001, "db4", 2, 0)])
def test_whole_transform_entries_on_guarded_misaligned_buffers(nr, nc, wname, levels, fused, sfx):
    """(21, 33): packs of 16 rows, the last one partial; (2, 4099): one row per workgroup, odd at every depth; (2, 24001): the per-level loop"""
    L, dt, f, hlen = _setup(wname, sfx)
    assert L.pdwt_wp1_geometry(nc, hlen, levels, None) == levels and L.pdwt_wp1_fused(nc, hlen, levels, dt.itemsize) == fused
    assert L.pdwt_wp1_tmp_elems(nr, nc, hlen, levels, dt.itemsize) == 0
    x = np.random.RandomState(5).uniform(-100, 100, (nr, nc)).astype(dt)
    tr = R.tree(x, wname, levels)
    names = ["d%d" % k for k in range(1, levels + 1)]
    basis = [(1, 1)] + [(levels, i) for i in range(2 ** (levels - 1))] if levels > 1 else [(1, 0), (1, 1)]
    state = _state_table(L, levels, basis)
    regions = [Region("img", x.size, dt, "in", 1)] + [Region(n, tr[k + 1].size, dt, "out", k + 1) for k, n in enumerate(names)]
    regions.append(Region("state", state.size, np.uint8, "in", 3))
    payloads = dict([("img", x), ("state", state)] + [(n, np.full(tr[k + 1].size, np.nan, dt)) for k, n in enumerate(names)])
    A = Arena(L, regions, payloads)
    fwd, inv = getattr(L, "pdwt_wp1_forward_" + sfx), getattr(L, "pdwt_wp1_inverse_" + sfx)
    img, st = A.ptr("img"), A.ptr("state")
    tab = (C.c_void_p * levels)(*[A.ptr(n) for n in names])
    hole = (C.c_void_p * levels)(*([A.ptr(n) for n in names[:-1]] + [None]))
    try:
        assert fwd(None, tab, nr, nc, levels, C.byref(f)) == -1 and fwd(img, None, nr, nc, levels, C.byref(f)) == -1
        assert fwd(img, hole, nr, nc, levels, C.byref(f)) == -1 and fwd(img, tab, nr, nc, levels, None) == -1
        assert fwd(img, tab, 0, nc, levels, C.byref(f)) == -1 and fwd(img, tab, nr, nc, 0, C.byref(f)) == -1 and fwd(img, tab, nr, nc, 13, C.byref(f)) == -1
        assert fwd(img, tab, nr, hlen - 1, 1, C.byref(f)) == -1  # too short for one level
        assert inv(None, tab, nr, nc, levels, st, C.byref(f)) == -1 and inv(img, hole, nr, nc, levels, st, C.byref(f)) == -1
        assert inv(img, tab, nr, nc, levels, None, C.byref(f)) == -1 and inv(img, tab, nr, nc, levels, st, None) == -1
        assert inv(img, tab, nr, nc, 0, st, C.byref(f)) == -1
        for n in names:
            A.by_name[n].role = "in"
        A.check("refusals %s %s" % (wname, sfx))
        for n in names:
            A.by_name[n].role = "out"
        assert fwd(img, tab, nr, nc, levels, C.byref(f)) == fused  # PDWT_WP1_FUSED / PDWT_WP1_LEVELS
        image = A.check("forward %s %s" % (wname, sfx))
        for k, n in enumerate(names):
            got = A.get(image, n, shape=tr[k + 1].shape)
            assert not np.isnan(got).any(), n
            e = _node_err(got, tr[k + 1])
            print("%dx%d %s %s depth %d: %.3e" % (nr, nc, wname, sfx, k + 1, e))
            assert e <= FWD[sfx], (n, e)
        # inverse from the mixed basis: the nodes of the basis hold the reference, every other node NaN
        want = R.inverse({b: tr[b[0]][:, b[1]] for b in basis}, x.shape, wname, levels)
        for k, n in enumerate(names):
            lev = np.full(tr[k + 1].shape, np.nan, dt)
            for d, i in basis:
                if d == k + 1:
                    lev[:, i] = tr[d][:, i]
            A.upload(n, lev)
            A.by_name[n].role = "in" if fused else "inout"  # the fused path writes the rows only; per level the parents land in their depth
        A.by_name["img"].role = "out"
        A.upload("img", np.full(x.shape, np.nan, dt))
        assert inv(img, tab, nr, nc, levels, st, C.byref(f)) == fused
        image = A.check("inverse %s %s" % (wname, sfx))
        got = A.get(image, "img", shape=x.shape)
        assert not np.isnan(got).any()
        e = band_err(got, want)
        print("%dx%d %s %s inverse from a mixed basis: %.3e" % (nr, nc, wname, sfx, e))
        assert e <= FWD[sfx], e
        for d, i in basis:  # the nodes of the basis keep their bits on either path
            assert np.array_equal(A.get(image, names[d - 1], shape=tr[d].shape)[:, i], tr[d][:, i]), (d, i)
    finally:
        A.free()


@pytest.mark.parametrize("sfx", ["f32", "f64"])
def test_moments_and_threshold_on_guarded_misaligned_buffers(sfx):
    L, dt, _, _ = _setup("db2", sfx)
    nr, nodes, n = 5, 4, 37
    lev = np.random.RandomState(7).uniform(-10, 10, (nr, nodes, n)).astype(dt)
    lev[0, 1, :5] = 0  # zero terms are skipped by the entropy
    flags = np.array([0, 1, 2, 1], np.uint8)
    A = Arena(L, [Region("lev", lev.size, dt, "in", 1), Region("flags", 4, np.uint8, "in", 1)], {"lev": lev, "flags": flags})
    mom, thr = getattr(L, "pdwt_wp1_moments_" + sfx), getattr(L, "pdwt_wp1_thresh_" + sfx)
    p, fl = A.ptr("lev"), A.ptr("flags")
    out = np.full(4 * nr * nodes, np.nan)
    po = out.ctypes.data_as(C.POINTER(C.c_double))
    try:
        assert mom(None, nr * nodes, n, po) == -1 and mom(p, 0, n, po) == -1 and mom(p, nr * nodes, 0, po) == -1 and mom(p, nr * nodes, n, None) == -1
        assert thr(0, None, nr, nodes, n, fl, 1.0) == -1 and thr(0, p, nr, nodes, n, None, 1.0) == -1 and thr(2, p, nr, nodes, n, fl, 1.0) == -1
        assert thr(0, p, 0, nodes, n, fl, 1.0) == -1 and thr(0, p, nr, 0, n, fl, 1.0) == -1 and thr(0, p, nr, nodes, 0, fl, 1.0) == -1
        A.check("refusals %s" % sfx)
        assert np.isnan(out).all()
        assert mom(p, nr * nodes, n, po) == 0
        A.check("moments %s" % sfx)
        got = out.reshape(nr * nodes, 4)
        v = lev.reshape(nr * nodes, n).astype(np.float64)
        v2 = v * v
        ent = -np.where(v2 > 0, v2 * np.log(np.where(v2 > 0, v2, 1.0)), 0.0).sum(axis=1)
        for k, want in enumerate((np.abs(v).sum(axis=1), v2.sum(axis=1), np.abs(v).max(axis=1), ent)):
            assert np.all(np.abs(got[:, k] - want) <= 1e-10 * np.abs(want)), k
        assert np.array_equal(got[:, 2], np.abs(v).max(axis=1))
        again = np.empty_like(out)
        assert mom(p, nr * nodes, n, again.ctypes.data_as(C.POINTER(C.c_double))) == 0 and np.array_equal(again, out)  # the same bits
        A.by_name["lev"].role = "inout"
        for op, name in ((0, "soft"), (1, "hard")):
            A.upload("lev", lev)
            assert thr(op, p, nr, nodes, n, fl, 2.5) == 0
            image = A.check("%s threshold %s" % (name, sfx))
            got = A.get(image, "lev", shape=lev.shape)
            b = dt.type(2.5)
            want = np.copysign(np.maximum(np.abs(lev) - b, dt.type(0)), lev) if op == 0 else np.where(np.abs(lev) - b > 0, lev, dt.type(0) * lev)
            for i in range(nodes):
                assert np.array_equal(got[:, i], want[:, i] if flags[i] == 1 else lev[:, i]), (name, i)
    finally:
        A.free()
