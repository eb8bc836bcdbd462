"""The drivers of the batched 2-D transform with boundary modes (pdwt_ext2db_forward_* / _inverse_* and the level drivers) on buffers of a
CALLER: every buffer guarded on both sides and misaligned down to its element size (tests/cabi_arena.py), so the 16-byte staging loads
of the fused kernels must fall back to element accesses.  After each call: the documented return code, no byte outside a payload and
no byte of a read-only payload changed, and the values within the bounds of tests/test_ext2d_gpu.py of tests/refext.py per image.
Cases: a fused shape, a per-level shape (with its scratch full of the fill pattern), and the folded 2 x 7 x 8 db4 level (n = hlen - 1:
below the level clamp of the class, reachable only through the drivers)."""
import ctypes as C

import numpy as np
import pytest

import pdwt_amd
from pdwt_amd import _native as nat
from tests import refext as R
from tests.cabi_arena import Arena, Region
from tests.helpers import band_err

pytestmark = pytest.mark.gpu

FWD = {"f32": 1e-5, "f64": 1e-12}
FUSED, LEVELS = 1, 0


def _setup(wname, sfx):
    L = pdwt_amd.hip()
    dt = np.dtype(np.float32 if sfx == "f32" else np.float64)
    f = (nat.Filters32 if sfx == "f32" else nat.Filters64)()
    hlen = getattr(L, "pdwt_compute_filters_separable_" + sfx)(wname.encode(), 0, C.byref(f))
    assert hlen > 0
    f.hlen = hlen
    return L, dt, f, hlen


def _images(B, Nr, Nc, dt):
    yy, xx = np.mgrid[0:Nr, 0:Nc]
    return (np.random.RandomState(3).standard_normal((B, Nr, Nc)) + ((3 * xx + 5 * yy) % 17 - 8.0)).astype(dt)


@pytest.mark.parametrize("sfx", ["f32", "f64"])
@pytest.mark.parametrize("B,Nr,Nc,wname,levels,mode,path", [(3, 37, 51, "db3", 2, "reflect", FUSED), (2, 160, 200, "db4", 2, "symmetric", LEVELS),
                                                            (2, 7, 8, "db4", 1, "periodic", FUSED)], ids=["fused", "levels", "folded"])
def test_whole_transform_drivers_on_guarded_misaligned_buffers(B, Nr, Nc, wname, levels, mode, path, sfx):
    L, dt, f, hlen = _setup(wname, sfx)
    assert L.pdwt_ext2db_fused(Nr, Nc, hlen, levels, dt.itemsize) == path
    ntmp = L.pdwt_ext2db_tmp_elems(B, Nr, Nc, hlen, levels, dt.itemsize)
    assert (ntmp == 0) == (path == FUSED)
    x = _images(B, Nr, Nc, dt)
    refs = [R.wavedec2(x[b], wname, levels, mode, np.float64) for b in range(B)]
    shapes = R.band_shapes((Nr, Nc), hlen, levels)
    names = ["b%d" % k for k in range(len(shapes))]
    regions = [Region("img", x.size, dt, "in", 1)] + [Region(n, B * s[0] * s[1], dt, "out", (k % 3) + 1) for k, (n, s) in enumerate(zip(names, shapes))]
    if ntmp:
        regions.append(Region("tmp", ntmp, dt, "scratch", 3))
    A = Arena(L, regions, {"img": x})
    ct = C.c_float if sfx == "f32" else C.c_double
    fwd, inv = getattr(L, "pdwt_ext2db_forward_" + sfx), getattr(L, "pdwt_ext2db_inverse_" + sfx)
    try:
        tab = C.cast(A.band_table(names, ct), C.POINTER(C.c_void_p))
        tmp = A.ptr("tmp") if ntmp else None
        # refusals first: nothing may be touched (the bands still hold the fill pattern afterwards)
        assert fwd(A.ptr("img"), tab, B, Nr, Nc, levels, 5, C.byref(f), tmp) == -1
        assert fwd(A.ptr("img"), tab, 0, Nr, Nc, levels, 2, C.byref(f), tmp) == -1 and fwd(A.ptr("img"), tab, 65536, Nr, Nc, levels, 2, C.byref(f), tmp) == -1
        assert fwd(A.ptr("img"), tab, B, Nr, Nc, 0, 2, C.byref(f), tmp) == -1 and fwd(A.ptr("img"), tab, B, hlen - 2, Nc, levels, 2, C.byref(f), tmp) == -1
        assert inv(A.ptr("img"), tab, 0, Nr, Nc, levels, C.byref(f), tmp) == -1 and inv(None, tab, B, Nr, Nc, levels, C.byref(f), tmp) == -1
        if ntmp:
            assert fwd(A.ptr("img"), tab, B, Nr, Nc, levels, 2, C.byref(f), None) == -1 and inv(A.ptr("img"), tab, B, Nr, Nc, levels, C.byref(f), None) == -1
        for n in names:
            A.by_name[n].role = "in"
        A.check("refusals %s %s" % (wname, sfx))
        for n in names:
            A.by_name[n].role = "out"
        assert fwd(A.ptr("img"), tab, B, Nr, Nc, levels, R.MODES.index(mode), C.byref(f), tmp) == path
        img = A.check("forward %s %s %s" % (wname, mode, sfx))
        for k, (n, s) in enumerate(zip(names, shapes)):
            got = A.get(img, n, shape=(B,) + s)
            for b in range(B):
                e = band_err(got[b], refs[b][k])
                assert e <= FWD[sfx], (k, b, e)
        # inverse from the reference bands into a zeroed batch
        A.by_name["img"].role = "out"
        for k, n in enumerate(names):
            A.by_name[n].role = "in"
            A.upload(n, np.stack([refs[b][k] for b in range(B)]).astype(dt))
        A.upload("img", np.zeros_like(x))
        assert inv(A.ptr("img"), tab, B, Nr, Nc, levels, C.byref(f), tmp) == path
        img = A.check("inverse %s %s" % (wname, sfx))
        got = A.get(img, "img", shape=(B, Nr, Nc))
        e = max(band_err(got[b], x[b]) for b in range(B))
        print("%s %s %s: inverse %.3e" % (wname, mode, sfx, e))
        assert e <= 10 * FWD[sfx], e
    finally:
        A.free()


@pytest.mark.parametrize("sfx", ["f32", "f64"])
@pytest.mark.parametrize("B,Nr,Nc,wname,mode", [(2, 7, 8, "db4", "symmetric"), (3, 61, 67, "db4", "constant"), (2, 33, 47, "haar", "reflect")],
                         ids=["folded", "db4", "haar"])
def test_level_drivers_on_guarded_misaligned_buffers(B, Nr, Nc, wname, mode, sfx):
    L, dt, f, hlen = _setup(wname, sfx)
    hr, hc = (Nr + hlen - 1) // 2, (Nc + hlen - 1) // 2
    x = _images(B, Nr, Nc, dt)
    refs = [R.wavedec2(x[b], wname, 1, mode, np.float64) for b in range(B)]
    names = ("a", "h", "v", "d")
    regions = [Region("img", x.size, dt, "in", 1)] + [Region(n, B * hr * hc, dt, "out", k + 1) for k, n in enumerate(names)]
    A = Arena(L, regions, {"img": x})
    fwd, inv = getattr(L, "pdwt_ext2db_forward_level_" + sfx), getattr(L, "pdwt_ext2db_inverse_level_" + sfx)
    try:
        bands = [A.ptr(n) for n in names]
        assert fwd(A.ptr("img"), *bands, B, Nr, Nc, 5, C.byref(f)) == -1 and fwd(A.ptr("img"), *bands, B, Nr, Nc, -1, C.byref(f)) == -1
        assert fwd(A.ptr("img"), *bands, 0, Nr, Nc, 2, C.byref(f)) == -1 and fwd(A.ptr("img"), *bands, 65536, Nr, Nc, 2, C.byref(f)) == -1
        if hlen > 2:
            assert fwd(A.ptr("img"), *bands, B, hlen - 2, Nc, 2, C.byref(f)) == -1 and inv(A.ptr("img"), *bands, B, Nr, hlen - 2, C.byref(f)) == -1
        assert fwd(None, *bands, B, Nr, Nc, 2, C.byref(f)) == -1
        for n in names:
            A.by_name[n].role = "in"
        A.check("refusals %s %s" % (wname, sfx))
        for n in names:
            A.by_name[n].role = "out"
        assert fwd(A.ptr("img"), *bands, B, Nr, Nc, R.MODES.index(mode), C.byref(f)) == 0
        img = A.check("forward level %s %s %s" % (wname, mode, sfx))
        for k, n in enumerate(names):
            got = A.get(img, n, shape=(B, hr, hc))
            for b in range(B):
                e = band_err(got[b], refs[b][k])
                assert e <= FWD[sfx], (n, b, e)
        A.by_name["img"].role = "out"
        for k, n in enumerate(names):
            A.by_name[n].role = "in"
            A.upload(n, np.stack([refs[b][k] for b in range(B)]).astype(dt))
        A.upload("img", np.zeros_like(x))
        assert inv(A.ptr("img"), *bands, B, Nr, Nc, C.byref(f)) == 0
        img = A.check("inverse level %s %s" % (wname, sfx))
        got = A.get(img, "img", shape=(B, Nr, Nc))
        e = max(band_err(got[b], x[b]) for b in range(B))
        assert e <= 10 * FWD[sfx], e
    finally:
        A.free()
