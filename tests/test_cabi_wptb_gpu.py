"""The whole-transform entries of the batched 2-D wavelet packets (pdwt_wptb_forward_* / pdwt_wptb_inverse_*) on buffers of a CALLER:
every buffer guarded on both sides and misaligned down to its element size (tests/cabi_arena.py), both precisions, both forms (the fused
launch and the level entries looped over the forest), the inverse under a mixed state table.  After each call: the return code names the
form, no byte outside a payload and no byte of a read-only payload changed, every output fully overwritten (no NaN of the fill left) and
the values within the bounds of tests/test_wptb_gpu.py of tests/refwpt.py.  Every PDWT_EINVAL case touches nothing."""
import ctypes as C

import numpy as np
import pytest

import pdwt_amd
from pdwt_amd import _native as nat
from tests import refwpt as R
from tests.cabi_arena import Arena, Region
from tests.helpers import band_err

pytestmark = pytest.mark.gpu

FWD = {"f32": 1e-5, "f64": 1e-12}


def off(l):
    return (4 ** l - 1) // 3


def _setup(wname, sfx):
    L = pdwt_amd.hip()
    dt = np.dtype(np.float32 if sfx == "f32" else np.float64)
    f = (nat.Filters32 if sfx == "f32" else nat.Filters64)()
    hlen = getattr(L, "pdwt_compute_filters_separable_" + sfx)(wname.encode(), 0, C.byref(f))
    assert hlen > 0
    f.hlen = hlen
    return L, dt, f, hlen


def _mixed_basis(levels):
    b = [(1, 0), (1, 2), (1, 3)] + [(2, 4 + q) for q in range(4)]
    if levels >= 3:
        b.remove((2, 5))
        b += [(3, 20 + q) for q in range(4)]
    return sorted(b)


@pytest.mark.parametrize("sfx", ["f32", "f64"])
@pytest.mark.parametrize("allow_fused", [1, 0])
@pytest.mark.parametrize("B,Nr,Nc,wname,levels", [(3, 37, 51, "db3", 2), (2, 64, 64, "db4", 3), (2, 9, 7, "haar", 2)])
def test_whole_transform_entries_on_guarded_misaligned_buffers(B, Nr, Nc, wname, levels, allow_fused, sfx):
    L, dt, f, hlen = _setup(wname, sfx)
    assert L.pdwt_wptb_geometry(Nr, Nc, hlen, levels, None, None) == levels and L.pdwt_wptb_fused(Nr, Nc, hlen, levels, dt.itemsize) == 1
    fused = allow_fused  # every shape here fits the budget: the flag decides
    x = np.random.RandomState(5).uniform(-100, 100, (B, Nr, Nc)).astype(dt)
    trees = [R.tree(x[b], wname, levels) for b in range(B)]
    ref = [np.stack([t[d] for t in trees]) for d in range(levels + 1)]  # (B, 4^d, nr, nc)
    names = ["d%d" % k for k in range(1, levels + 1)]
    basis = _mixed_basis(levels)
    d_, i_ = (C.c_int * len(basis))(*[v[0] for v in basis]), (C.c_int * len(basis))(*[v[1] for v in basis])
    state = (C.c_ubyte * off(levels + 1))()
    assert L.pdwt_wptb_state_table(levels, d_, i_, len(basis), state) == 0
    nl = L.pdwt_wptb_chunk_lists(B, levels, state, None)
    assert nl == L.pdwt_wptb_tmp_elems(B, Nr, Nc, hlen, levels, dt.itemsize, 0) > 0 and L.pdwt_wptb_tmp_elems(B, Nr, Nc, hlen, levels, dt.itemsize, 1) == 0
    lists = (C.c_int * nl)()
    assert L.pdwt_wptb_chunk_lists(B, levels, state, lists) == nl
    regions = [Region("img", x.size, dt, "in", 1)] + [Region(n, ref[k + 1].size, dt, "out", k + 1) for k, n in enumerate(names)]
    regions += [Region("state", len(state), np.uint8, "in", 3), Region("lists", nl, np.int32, "in", 1)]
    payloads = dict([("img", x), ("state", np.frombuffer(state, np.uint8)), ("lists", np.frombuffer(lists, np.int32))]
                    + [(n, np.full(ref[k + 1].size, np.nan, dt)) for k, n in enumerate(names)])
    A = Arena(L, regions, payloads)
    fwd, inv = getattr(L, "pdwt_wptb_forward_" + sfx), getattr(L, "pdwt_wptb_inverse_" + sfx)
    img, st, ls = A.ptr("img"), A.ptr("state"), A.ptr("lists")
    tab = (C.c_void_p * levels)(*[A.ptr(n) for n in names])
    hole = (C.c_void_p * levels)(*([A.ptr(n) for n in names[:-1]] + [None]))
    try:
        # refusals first: nothing may be touched
        assert fwd(None, tab, B, Nr, Nc, levels, C.byref(f), allow_fused) == -1 and fwd(img, None, B, Nr, Nc, levels, C.byref(f), allow_fused) == -1
        assert fwd(img, hole, B, Nr, Nc, levels, C.byref(f), allow_fused) == -1 and fwd(img, tab, B, Nr, Nc, levels, None, allow_fused) == -1
        assert fwd(img, tab, 0, Nr, Nc, levels, C.byref(f), allow_fused) == -1 and fwd(img, tab, 65536, Nr, Nc, levels, C.byref(f), allow_fused) == -1
        assert fwd(img, tab, B, Nr, Nc, 0, C.byref(f), allow_fused) == -1 and fwd(img, tab, B, Nr, Nc, 8, C.byref(f), allow_fused) == -1
        assert inv(None, tab, B, Nr, Nc, levels, state, st, ls, C.byref(f), allow_fused) == -1
        assert inv(img, hole, B, Nr, Nc, levels, state, st, ls, C.byref(f), allow_fused) == -1
        assert inv(img, tab, B, Nr, Nc, levels, None, st, ls, C.byref(f), allow_fused) == -1
        assert inv(img, tab, B, Nr, Nc, levels, state, st, ls, None, allow_fused) == -1
        assert inv(img, tab, B, Nr, Nc, levels, state, None if fused else st, ls if fused else None, C.byref(f), allow_fused) == -1  # what this form reads
        for n in names:
            A.by_name[n].role = "in"
        A.check("refusals %s %s" % (wname, sfx))
        for n in names:
            A.by_name[n].role = "out"
        assert fwd(img, tab, B, Nr, Nc, levels, C.byref(f), allow_fused) == fused  # PDWT_WPTB_FUSED / PDWT_WPTB_LEVELS
        image = A.check("forward %s %s" % (wname, sfx))
        for k, n in enumerate(names):
            got = A.get(image, n, shape=ref[k + 1].shape)
            assert not np.isnan(got).any(), n
            e = max(band_err(got[b], ref[k + 1][b]) for b in range(B))
            print("%dx%dx%d %s %s fused=%d depth %d: %.3e" % (B, Nr, Nc, wname, sfx, fused, k + 1, e))
            assert e <= FWD[sfx], (n, e)
        # inverse from the mixed basis: the nodes of the basis hold the reference, every other node NaN
        want = np.stack([R.inverse({b: trees[k][b[0]][b[1]] for b in basis}, (Nr, Nc), wname, levels) for k in range(B)])
        for k, n in enumerate(names):
            lev = np.full(ref[k + 1].shape, np.nan, dt)
            for d, i in basis:
                if d == k + 1:
                    lev[:, i] = ref[d][:, i]
            A.upload(n, lev)
            A.by_name[n].role = "in" if fused else "inout"  # the fused form writes the images only; per depth the parents land in their depth
        A.by_name["img"].role = "out"
        A.upload("img", np.full(x.shape, np.nan, dt))
        assert inv(img, tab, B, Nr, Nc, levels, state, st, ls, C.byref(f), allow_fused) == fused
        image = A.check("inverse %s %s" % (wname, sfx))
        got = A.get(image, "img", shape=x.shape)
        assert not np.isnan(got).any()
        e = band_err(got, want)
        print("%dx%dx%d %s %s fused=%d inverse from a mixed basis: %.3e" % (B, Nr, Nc, wname, sfx, fused, e))
        assert e <= FWD[sfx], e
        for d, i in basis:  # the nodes of the basis keep their bits on either path
            assert np.array_equal(A.get(image, names[d - 1], shape=ref[d].shape)[:, i], ref[d][:, i]), (d, i)
    finally:
        A.free()
