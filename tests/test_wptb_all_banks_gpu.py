"""Every filter bank of the table through the fused kernels of WaveletPacketBatch (wpt2db.hip: one instantiation per even length 2 .. 40,
direction and precision), against a float64 statement of the tree: the one-level transform of tests/ref2d.py applied to every node again
(tests/newer_bank_matrix.ref_forward / ref_inverse, as tests/test_newer_all_banks_gpu.py does for the single-image class).
  sweep        all 72 banks, ONE depth, two images of 2 (hlen - 1) x (2 (hlen - 1) + 1): the smallest the level clamp allows, odd columns; every
               length is fused there in both precisions (asserted through the plan function)
  two depths   one bank per length, two images of 4 (hlen - 1) x (4 (hlen - 1) + 1); fused where the plan says so (float32 up to 36 taps,
               float64 up to 24: beyond, the image does not fit and the same checks judge the per-depth form)
What is asserted per image (TOL = 1e-5 float32, 1e-12 float64, node-normalised: helpers.band_err):
  forward      every node of every depth                                                 <= TOL
  inverse      the image against the reference inverse of THE NODES THE GPU PRODUCED     <= 10 TOL
  round trip   the image against the input                                               <= 10 TOL + 4 D
               D = the reconstruction defect of the float64 reference itself on that image: the table's sym* and long bior banks
               (sym3, sym18, sym20, ...) reconstruct to ~1e-11 only in exact arithmetic; 4 D and not D because D is itself a rounded figure
               and the kernel's rounding adds to it (tests/test_newer_all_banks_gpu.py)
"""
import functools

import numpy as np
import pytest

import pdwt_amd
from pdwt_amd import WaveletPacketBatch
from pdwt_amd.wavelets import W_INIT
from tests import newer_bank_matrix as M
from tests.helpers import band_err

pytestmark = pytest.mark.gpu

B = 2


def sweep_shape(h):
    return 2 * (h - 1), 2 * (h - 1) + 1


def two_shape(h):
    return 4 * (h - 1), 4 * (h - 1) + 1


def _pcase(wname, shape, levels):
    return dict(cls="wpt", wname=wname, hlen=M.hlen_of(wname), shape=shape, levels=levels, mode=None)


@functools.lru_cache(maxsize=4)
def _reference(wname, shape, levels):
    """(float32-rounded images, per image: float64 nodes of depth 1 .. L flattened in depth order, the defect D of the reference)"""
    case = _pcase(wname, shape, levels)
    x = np.random.RandomState(2000 + M.ALL72.index(wname)).uniform(-100, 100, (B,) + shape).astype(np.float32)
    want, defect = [], []
    for b in range(B):
        w = M.ref_forward(case, x[b].astype(np.float64))
        want.append(w)
        defect.append(band_err(M.ref_inverse(case, w), x[b].astype(np.float64)))
    x.setflags(write=False)
    return x, want, defect


def _check(wname, shape, levels, dt):
    dt = np.dtype(dt)
    tol = M.TOL[dt]
    case = _pcase(wname, shape, levels)
    x32, want, defect = _reference(wname, shape, levels)
    x = x32.astype(dt)
    h = case["hlen"]
    plan = pdwt_amd.hip().pdwt_wptb_fused(shape[0], shape[1], h, levels, dt.itemsize)
    assert plan in (0, 1)
    W = WaveletPacketBatch(x, wname, levels)
    try:
        assert W.state == W_INIT and W.dtype == dt and W.levels == levels and W.fused == bool(plan), (wname, dt.name, W.state, W.levels)
        W.forward()
        lev = [W.get_level(d) for d in range(1, levels + 1)]
        got = [[n for l in lev for n in l[b]] for b in range(B)]  # per image: the nodes of depth 1, then of depth 2
        for b in range(B):
            assert len(got[b]) == len(want[b])
            for k, (g, o) in enumerate(zip(got[b], want[b])):
                e = band_err(g, o)
                assert g.dtype == dt and e <= tol, (wname, dt.name, "forward, image, node", b, k, e)
        W.inverse()
        rec = W.get_image()
        for b in range(B):
            e_inv = band_err(rec[b], M.ref_inverse(case, got[b]))
            e_rt = band_err(rec[b], x[b])
            assert e_inv <= 10 * tol, (wname, dt.name, "inverse of its own nodes, image", b, e_inv)
            assert e_rt <= 10 * tol + 4 * defect[b], (wname, dt.name, "round trip, image", b, e_rt, defect[b])
        return W.fused
    finally:
        W.close()


@pytest.mark.parametrize("wname", M.ALL72)
def test_every_bank_one_depth_fused(wname):
    shape = sweep_shape(M.hlen_of(wname))
    for dt in M.DTYPES:
        assert pdwt_amd.hip().pdwt_wptb_geometry(shape[0], shape[1], M.hlen_of(wname), 1, None, None) == 1
        assert _check(wname, shape, 1, dt) is True, (wname, dt)  # the fused kernels of this length ran


@pytest.mark.parametrize("wname", M.PER_LENGTH)
def test_one_bank_per_length_two_depths(wname):
    h = M.hlen_of(wname)
    shape = two_shape(h)
    assert pdwt_amd.hip().pdwt_wptb_geometry(shape[0], shape[1], h, 2, None, None) == 2
    assert pdwt_amd.hip().pdwt_wptb_geometry(shape[0] - 1, shape[1], h, 2, None, None) == 1  # the smallest the clamp allows
    for dt in M.DTYPES:
        # two image-sized buffers of 4 (hlen - 1) x (4 (hlen - 1) + 2) elements in 160 KiB: float32 up to 36 taps, float64 up to 24
        assert _check(wname, shape, 2, dt) == (h <= (36 if dt == M.F32 else 24)), (wname, dt)


def test_the_sweeps_reach_every_length():
    assert sorted({M.hlen_of(w) for w in M.ALL72}) == sorted({M.hlen_of(w) for w in M.PER_LENGTH}) == list(range(2, 42, 2)) and len(M.ALL72) == 72
