"""The two level drivers of the boundary-mode volume transform (pdwt_ext3d_forward_level_* / pdwt_ext3d_inverse_level_*) on buffers of
a CALLER: the volume, each of the eight bands and the scratch guarded on both sides and misaligned down to their element size
(tests/cabi_arena.py), 7 x 7 x 7 db4 `symmetric` (every window folds on all three axes) and 9 x 33 x 47 haar `reflect` (odd sizes), both
precisions.  After each call: return code 0, no byte outside a payload and no byte of a read-only payload changed, and the values
within the bounds of tests/test_ext3d_gpu.py of tests/refext3d.py.  A bad mode and an axis shorter than hlen - 1 are PDWT_EINVAL and
touch nothing."""
import ctypes as C

import numpy as np
import pytest

import pdwt_amd
from pdwt_amd import _native as nat
from tests import refext3d as R3
from tests.cabi_arena import Arena, Region
from tests.helpers import band_err

pytestmark = pytest.mark.gpu

FWD = {"f32": 1e-5, "f64": 1e-12}
NAMES = R3.LEVEL_KEYS


@pytest.mark.parametrize("sfx", ["f32", "f64"])
@pytest.mark.parametrize("shape,wname,mode", [((7, 7, 7), "db4", "symmetric"), ((9, 33, 47), "haar", "reflect")])
def test_level_drivers_on_guarded_misaligned_buffers(shape, wname, mode, sfx):
    L = pdwt_amd.hip()
    dt = np.dtype(np.float32 if sfx == "f32" else np.float64)
    ct = C.c_float if sfx == "f32" else C.c_double
    f = (nat.Filters32 if sfx == "f32" else nat.Filters64)()
    hlen = getattr(L, "pdwt_compute_filters_separable_" + sfx)(wname.encode(), 0, C.byref(f))
    assert hlen > 0
    f.hlen = hlen
    nz, nr, nc = shape
    bshape = tuple((n + hlen - 1) // 2 for n in shape)
    nband = bshape[0] * bshape[1] * bshape[2]
    ntmp = 4 * nz * bshape[1] * bshape[2]  # the four quadrants: what a level needs
    assert L.pdwt_ext3d_tmp_elems(nz, nr, nc, hlen) >= ntmp
    x = np.random.RandomState(3).uniform(-100, 100, shape).astype(dt)
    ref = R3.wavedec3(x, wname, 1, mode, np.float64)  # one level: aaa, then the details = LEVEL_KEYS order
    regions = [Region("vol", x.size, dt, "in", 1)] + [Region(n, nband, dt, "out", k % 3 + 1) for k, n in enumerate(NAMES)]
    regions.append(Region("tmp", ntmp, dt, "scratch", 3))
    A = Arena(L, regions, {"vol": x})
    fwd, inv = getattr(L, "pdwt_ext3d_forward_level_" + sfx), getattr(L, "pdwt_ext3d_inverse_level_" + sfx)
    try:
        tab = C.cast(A.band_table(NAMES, ct), C.POINTER(C.c_void_p))
        vol, tmp = A.ptr("vol"), A.ptr("tmp")
        # refusals first: nothing may be touched (the bands still hold the fill pattern afterwards)
        assert fwd(vol, tab, nz, nr, nc, 5, C.byref(f), tmp) == -1 and fwd(vol, tab, nz, nr, nc, -1, C.byref(f), tmp) == -1
        if hlen > 2:
            for bad in ((hlen - 2, nr, nc), (nz, hlen - 2, nc), (nz, nr, hlen - 2)):
                assert fwd(vol, tab, *bad, 2, C.byref(f), tmp) == -1 and inv(vol, tab, *bad, C.byref(f), tmp) == -1
        assert fwd(vol, tab, 0, nr, nc, 2, C.byref(f), tmp) == -1 and fwd(None, tab, nz, nr, nc, 2, C.byref(f), tmp) == -1
        assert fwd(vol, tab, nz, nr, nc, 2, C.byref(f), None) == -1 and inv(vol, tab, nz, nr, nc, C.byref(f), None) == -1
        for n in NAMES + ("tmp",):
            A.by_name[n].role = "in"
        A.check("refusals %s %s" % (wname, sfx))
        for n in NAMES:
            A.by_name[n].role = "out"
        A.by_name["tmp"].role = "scratch"
        assert fwd(vol, tab, nz, nr, nc, R3.MODES.index(mode), C.byref(f), tmp) == 0
        img = A.check("forward %s %s %s" % (wname, mode, sfx))
        for k, n in enumerate(NAMES):
            e = band_err(A.get(img, n, shape=bshape), ref[k])
            print("%s %s %s band %s: %.3e" % (wname, mode, sfx, n, e))
            assert e <= FWD[sfx], (n, e)
        # inverse from the reference bands into a zeroed volume
        A.by_name["vol"].role = "out"
        for k, n in enumerate(NAMES):
            A.by_name[n].role = "in"
            A.upload(n, ref[k].astype(dt))
        A.upload("vol", np.zeros_like(x))
        assert inv(vol, tab, nz, nr, nc, C.byref(f), tmp) == 0
        img = A.check("inverse %s %s" % (wname, sfx))
        e = band_err(A.get(img, "vol", shape=shape), x)
        print("%s %s inverse: %.3e" % (wname, sfx, e))
        assert e <= 10 * FWD[sfx], e
    finally:
        A.free()
