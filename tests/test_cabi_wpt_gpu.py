"""The two packet level drivers of the C ABI (pdwt_wpt2d_forward_level_* / pdwt_wpt2d_inverse_level_*) on buffers of a CALLER: every
buffer guarded on both sides and misaligned down to its element size (tests/cabi_arena.py), once with a device list of parent nodes
and once with NULL (all parents), a Haar bank and an 8-tap bank, both precisions.  After each call: return code 0, no byte outside
a payload and no byte of a read-only payload changed, the children / parents NOT named by the list still hold what they held, and the
values within the bounds of tests/test_wpt2d_gpu.py of tests/refwpt.py."""
import ctypes as C

import numpy as np
import pytest

import pdwt_amd
from pdwt_amd import _native as nat
from tests import refwpt as R
from tests.cabi_arena import Arena, Region
from tests.helpers import band_err

pytestmark = pytest.mark.gpu

NR, NC, NPAR = 21, 30, 4  # four parent nodes of 21 x 30 -> sixteen children of 11 x 15
FWD = {"f32": 1e-5, "f64": 1e-12}


@pytest.mark.parametrize("sfx", ["f32", "f64"])
@pytest.mark.parametrize("nodes", [None, (2, 0)], ids=["all", "list"])
@pytest.mark.parametrize("wname,hlen", [("haar", 2), ("db4", 8)])
def test_level_drivers_on_guarded_misaligned_buffers(wname, hlen, nodes, sfx):
    L = pdwt_amd.hip()
    dt = np.dtype(np.float32 if sfx == "f32" else np.float64)
    f = (nat.Filters32 if sfx == "f32" else nat.Filters64)()
    assert getattr(L, "pdwt_compute_filters_separable_" + sfx)(wname.encode(), 0, C.byref(f)) == hlen
    f.hlen = hlen
    hr, hc = (NR + 1) // 2, (NC + 1) // 2
    x = np.random.RandomState(3).uniform(-100, 100, (NPAR, NR, NC)).astype(dt)
    ref = np.stack([c for node in x for c in R.split(node, wname)])  # (16, hr, hc)
    worked = list(nodes) if nodes else list(range(NPAR))
    regions = [Region("parent", x.size, dt, "in", 1), Region("child", 4 * NPAR * hr * hc, dt, "out", 3),
               Region("list", len(worked), np.int32, "in", 1)]
    A = Arena(L, regions, {"parent": x, "list": np.array(worked, np.int32)})
    try:
        d_list, n = (C.c_void_p(A.ptr("list")), len(worked)) if nodes else (None, NPAR)
        pattern = A.get(A.host, "child", shape=(4 * NPAR, hr, hc))
        assert getattr(L, "pdwt_wpt2d_forward_level_" + sfx)(A.ptr("parent"), A.ptr("child"), NR, NC, d_list, n, C.byref(f)) == 0
        img = A.check("forward %s %s" % (wname, sfx))
        got = A.get(img, "child", shape=(4 * NPAR, hr, hc))
        for p in range(NPAR):
            for q in range(4):
                if p in worked:
                    assert band_err(got[4 * p + q], ref[4 * p + q]) <= FWD[sfx], (p, q)
                else:
                    assert np.array_equal(got[4 * p + q].view(np.uint8), pattern[4 * p + q].view(np.uint8)), (p, q)
        # inverse from the reference children into zeroed parents
        A.by_name["child"].role, A.by_name["parent"].role = "in", "out"
        A.upload("child", ref)
        A.upload("parent", np.zeros_like(x))
        assert getattr(L, "pdwt_wpt2d_inverse_level_" + sfx)(A.ptr("parent"), A.ptr("child"), NR, NC, d_list, n, C.byref(f)) == 0
        img = A.check("inverse %s %s" % (wname, sfx))
        back = A.get(img, "parent", shape=(NPAR, NR, NC))
        for p in range(NPAR):
            if p in worked:
                assert band_err(back[p], x[p]) <= 10 * FWD[sfx], p
            else:
                assert not back[p].any(), p
    finally:
        A.free()
