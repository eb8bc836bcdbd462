"""The batched 1-D boundary-mode entries of the C ABI (pdwt_ext1d_forward_level_* / pdwt_ext1d_inverse_level_* and the whole-transform
pdwt_ext1d_forward_* / pdwt_ext1d_inverse_*) on buffers of a CALLER: every buffer guarded on both sides and misaligned down to its
element size (tests/cabi_arena.py), both precisions.  After each call: the return code, no byte outside a payload and no byte of a
read-only payload changed, every output fully overwritten (no NaN of the fill left) and the values within the bounds of
tests/test_ext1d_gpu.py of tests/refext1d.py.  Every PDWT_EINVAL case touches nothing."""
import ctypes as C

import numpy as np
import pytest

import pdwt_amd
from pdwt_amd import _native as nat
from tests import refext1d as R1
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


@pytest.mark.parametrize("sfx", ["f32", "f64"])
@pytest.mark.parametrize("shape,wname,mode", [((5, 77), "haar", "reflect"), ((3, 2101), "db4", "symmetric")])
def test_level_entries_on_guarded_misaligned_buffers(shape, wname, mode, sfx):
    """(3, 2101) db4: two tiles per row in either direction, the second one partial"""
    L, dt, f, hlen = _setup(wname, sfx)
    nr, nc = shape
    N = (nc + hlen - 1) // 2
    x = np.random.RandomState(3).standard_normal(shape).astype(dt)
    ref = R1.wavedec(x, wname, 1, mode, np.float64)
    nan = np.full((nr, N), np.nan, dt)
    A = Arena(L, [Region("img", x.size, dt, "in", 1), Region("a", nr * N, dt, "out", 1), Region("d", nr * N, dt, "out", 3)], {"img": x, "a": nan, "d": nan})
    fwd, inv = getattr(L, "pdwt_ext1d_forward_level_" + sfx), getattr(L, "pdwt_ext1d_inverse_level_" + sfx)
    img, a, d = A.ptr("img"), A.ptr("a"), A.ptr("d")
    try:
        # refusals first: nothing may be touched
        assert fwd(img, a, d, nr, nc, 5, C.byref(f)) == -1 and fwd(img, a, d, nr, nc, -1, C.byref(f)) == -1
        if hlen > 2:
            assert fwd(img, a, d, nr, hlen - 2, 2, C.byref(f)) == -1 and inv(img, a, d, nr, hlen - 2, C.byref(f)) == -1
        assert fwd(img, a, d, 0, nc, 2, C.byref(f)) == -1 and fwd(img, a, d, nr, 0, 2, C.byref(f)) == -1 and inv(img, a, d, 0, nc, C.byref(f)) == -1
        assert fwd(None, a, d, nr, nc, 2, C.byref(f)) == -1 and fwd(img, None, d, nr, nc, 2, C.byref(f)) == -1 and fwd(img, a, None, nr, nc, 2, C.byref(f)) == -1
        assert fwd(img, a, d, nr, nc, 2, None) == -1 and inv(None, a, d, nr, nc, C.byref(f)) == -1 and inv(img, a, None, nr, nc, C.byref(f)) == -1
        assert fwd(img, a, d, 1 << 16, 1 << 15, 2, C.byref(f)) == -1  # nr * nc = 2^31
        for n in ("a", "d"):
            A.by_name[n].role = "in"
        A.check("refusals %s %s" % (wname, sfx))
        for n in ("a", "d"):
            A.by_name[n].role = "out"
        assert fwd(img, a, d, nr, nc, R1.MODES.index(mode), C.byref(f)) == 0
        image = A.check("forward level %s %s %s" % (wname, mode, sfx))
        for k, n in enumerate(("a", "d")):
            got = A.get(image, n, shape=(nr, N))
            assert not np.isnan(got).any(), n  # fully overwritten
            e = band_err(got, ref[k])
            print("%s %s %s band %s: %.3e" % (wname, mode, sfx, n.upper(), e))
            assert e <= FWD[sfx], (n, e)
        # inverse from the reference bands into an image of NaN
        A.by_name["img"].role = "out"
        for k, n in enumerate(("a", "d")):
            A.by_name[n].role = "in"
            A.upload(n, ref[k].astype(dt))
        A.upload("img", np.full(shape, np.nan, dt))
        assert inv(img, a, d, nr, nc, C.byref(f)) == 0
        image = A.check("inverse level %s %s" % (wname, sfx))
        got = A.get(image, "img", shape=shape)
        assert not np.isnan(got).any()
        e = band_err(got, x)
        print("%s %s inverse: %.3e" % (wname, sfx, e))
        assert e <= 10 * FWD[sfx], e
    finally:
        A.free()


@pytest.mark.parametrize("sfx", ["f32", "f64"])
@pytest.mark.parametrize("shape,wname,levels,mode,fused", [((21, 33), "db2", 2, "symmetric", 1), ((2, 4099), "db4", 3, "constant", 1), ((2, 40037), "db4", 2, "symmetric", 0)])
def test_whole_transform_entries_on_guarded_misaligned_buffers(shape, wname, levels, mode, fused, sfx):
    """(21, 33): packs of 16 rows, the last one partial; (2, 4099): one row per workgroup; (2, 40037): the per-level loop through d_tmp"""
    L, dt, f, hlen = _setup(wname, sfx)
    ct = C.c_float if sfx == "f32" else C.c_double
    nr, nc = shape
    lens = R1.band_lens(nc, hlen, levels)
    assert L.pdwt_ext1d_fused(nc, hlen, levels, dt.itemsize) == fused
    ntmp = L.pdwt_ext1d_tmp_elems(nr, nc, hlen, levels, dt.itemsize)
    assert ntmp == (0 if fused else 2 * nr * ((nc + hlen - 1) // 2))
    x = np.random.RandomState(5).standard_normal(shape).astype(dt)
    ref = R1.wavedec(x, wname, levels, mode, np.float64)
    names = ["b%d" % k for k in range(levels + 1)]
    regions = [Region("img", x.size, dt, "in", 1)] + [Region(n, nr * lens[k], dt, "out", k + 1) for k, n in enumerate(names)]
    if ntmp:
        regions.append(Region("tmp", ntmp, dt, "scratch", 1))
    A = Arena(L, regions, dict([("img", x)] + [(n, np.full(nr * lens[k], np.nan, dt)) for k, n in enumerate(names)]))
    fwd, inv = getattr(L, "pdwt_ext1d_forward_" + sfx), getattr(L, "pdwt_ext1d_inverse_" + sfx)
    img, tmp = A.ptr("img"), (A.ptr("tmp") if ntmp else None)
    tab = C.cast(A.band_table(names, ct), C.POINTER(C.c_void_p))
    hole = (C.c_void_p * (levels + 1))(*([A.ptr(n) for n in names[:-1]] + [None]))
    try:
        m = R1.MODES.index(mode)
        assert fwd(img, tab, nr, nc, levels, 5, C.byref(f), tmp) == -1 and fwd(img, tab, nr, nc, 0, m, C.byref(f), tmp) == -1
        assert fwd(img, tab, nr, nc, 33, m, C.byref(f), tmp) == -1 and fwd(None, tab, nr, nc, levels, m, C.byref(f), tmp) == -1
        assert fwd(img, None, nr, nc, levels, m, C.byref(f), tmp) == -1 and fwd(img, hole, nr, nc, levels, m, C.byref(f), tmp) == -1
        assert fwd(img, tab, nr, hlen - 2, levels, m, C.byref(f), tmp) == -1 and fwd(img, tab, 0, nc, levels, m, C.byref(f), tmp) == -1
        assert inv(img, tab, nr, nc, 0, C.byref(f), tmp) == -1 and inv(None, tab, nr, nc, levels, C.byref(f), tmp) == -1
        assert inv(img, hole, nr, nc, levels, C.byref(f), tmp) == -1 and inv(img, tab, nr, nc, levels, None, tmp) == -1
        if not fused:
            assert fwd(img, tab, nr, nc, levels, m, C.byref(f), None) == -1 and inv(img, tab, nr, nc, levels, C.byref(f), None) == -1
        for n in names:
            A.by_name[n].role = "in"
        A.check("refusals %s %s" % (wname, sfx))
        for n in names:
            A.by_name[n].role = "out"
        assert fwd(img, tab, nr, nc, levels, m, C.byref(f), tmp) == fused  # PDWT_EXT1D_FUSED / PDWT_EXT1D_LEVELS
        image = A.check("forward %s %s %s" % (wname, mode, sfx))
        for k, n in enumerate(names):
            got = A.get(image, n, shape=(nr, lens[k]))
            assert not np.isnan(got).any(), n
            e = band_err(got, ref[k])
            print("%s %s %s %s band %d: %.3e" % (shape, wname, mode, sfx, k, e))
            assert e <= FWD[sfx], (n, e)
        A.by_name["img"].role = "out"
        for k, n in enumerate(names):
            A.by_name[n].role = "in"
            A.upload(n, ref[k].astype(dt))
        A.upload("img", np.full(shape, np.nan, dt))
        assert inv(img, tab, nr, nc, levels, C.byref(f), tmp) == fused
        image = A.check("inverse %s %s" % (wname, sfx))
        got = A.get(image, "img", shape=shape)
        assert not np.isnan(got).any()
        e = band_err(got, x)
        print("%s %s %s inverse: %.3e" % (shape, wname, sfx, e))
        assert e <= 10 * FWD[sfx], e
    finally:
        A.free()
