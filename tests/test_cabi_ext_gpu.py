"""The two boundary-mode level drivers of the C ABI (pdwt_ext2d_forward_level_* / pdwt_ext2d_inverse_level_*) on buffers of a CALLER:
every buffer guarded on both sides and misaligned down to its element size (tests/cabi_arena.py), a Haar bank with `reflect` on odd
sizes and an 8-tap bank with `symmetric` on bands that cross a tile boundary, both precisions.  After each call: return code 0, no byte
outside a payload and no byte of a read-only payload changed, and the values within the bounds of tests/test_ext2d_gpu.py of
tests/refext.py.  A bad mode and a line shorter than hlen - 1 are PDWT_EINVAL and touch nothing."""
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
NAMES = ("a", "h", "v", "d")


@pytest.mark.parametrize("sfx", ["f32", "f64"])
@pytest.mark.parametrize("shape,wname,mode", [((61, 67), "db4", "symmetric"), ((33, 47), "haar", "reflect")])
def test_level_drivers_on_guarded_misaligned_buffers(shape, wname, mode, sfx):
    L = pdwt_amd.hip()
    dt = np.dtype(np.float32 if sfx == "f32" else np.float64)
    f = (nat.Filters32 if sfx == "f32" else nat.Filters64)()
    hlen = getattr(L, "pdwt_compute_filters_separable_" + sfx)(wname.encode(), 0, C.byref(f))
    assert hlen > 0
    f.hlen = hlen
    nr, nc = shape
    hr, hc = (nr + hlen - 1) // 2, (nc + hlen - 1) // 2
    x = np.random.RandomState(3).uniform(-100, 100, shape).astype(dt)
    ref = R.wavedec2(x, wname, 1, mode, np.float64)
    regions = [Region("img", x.size, dt, "in", 1)] + [Region(n, hr * hc, dt, "out", k + 1) for k, n in enumerate(NAMES)]
    A = Arena(L, regions, {"img": x})
    fwd, inv = getattr(L, "pdwt_ext2d_forward_level_" + sfx), getattr(L, "pdwt_ext2d_inverse_level_" + sfx)
    try:
        bands = [A.ptr(n) for n in NAMES]
        # refusals first: nothing may be touched (the bands still hold the fill pattern afterwards)
        assert fwd(A.ptr("img"), *bands, nr, nc, 5, C.byref(f)) == -1 and fwd(A.ptr("img"), *bands, nr, nc, -1, C.byref(f)) == -1
        if hlen > 2:
            assert fwd(A.ptr("img"), *bands, hlen - 2, nc, 2, C.byref(f)) == -1 and fwd(A.ptr("img"), *bands, nr, hlen - 2, 2, C.byref(f)) == -1
            assert inv(A.ptr("img"), *bands, hlen - 2, nc, C.byref(f)) == -1
        assert fwd(A.ptr("img"), *bands, 0, nc, 2, C.byref(f)) == -1 and fwd(None, *bands, nr, nc, 2, C.byref(f)) == -1
        for n in NAMES:
            A.by_name[n].role = "in"
        A.check("refusals %s %s" % (wname, sfx))
        for n in NAMES:
            A.by_name[n].role = "out"
        assert fwd(A.ptr("img"), *bands, nr, nc, R.MODES.index(mode), C.byref(f)) == 0
        img = A.check("forward %s %s %s" % (wname, mode, sfx))
        for k, n in enumerate(NAMES):
            e = band_err(A.get(img, n, shape=(hr, hc)), ref[k])
            print("%s %s %s band %s: %.3e" % (wname, mode, sfx, n.upper(), e))
            assert e <= FWD[sfx], (n, e)
        # inverse from the reference bands into a zeroed image
        A.by_name["img"].role = "out"
        for k, n in enumerate(NAMES):
            A.by_name[n].role = "in"
            A.upload(n, ref[k].astype(dt))
        A.upload("img", np.zeros_like(x))
        assert inv(A.ptr("img"), *bands, nr, nc, C.byref(f)) == 0
        img = A.check("inverse %s %s" % (wname, sfx))
        e = band_err(A.get(img, "img", shape=shape), x)
        print("%s %s inverse: %.3e" % (wname, sfx, e))
        assert e <= 10 * FWD[sfx], e
    finally:
        A.free()
