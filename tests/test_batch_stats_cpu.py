"""No-GPU tests of the batched band statistics (bandbatch.hip; ImageBatch.all_band_stats / estimate_sigma / threshold_bands / denoise /
norm1): the new C-ABI symbols are declared, bound and check their arguments, the Python surface checks its arguments before it
touches the native handle, and the ISA audit flags none of the new kernels."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest

import pdwt_amd
from pdwt_amd import _native as N
from tests.helpers import ROOT

PDWT_EINVAL = -1
ENTRIES = ["pdwt_bandbatch_stats_f32", "pdwt_bandbatch_stats_f64", "pdwt_bandbatch_thresh_f32", "pdwt_bandbatch_thresh_f64"]
HANDLE = ["num_bands", "all_band_stats", "estimate_sigma", "threshold_bands", "denoise", "norm1"]


def test_new_symbols_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "pdwt_hip.h")).read()
    L = pdwt_amd.hip()
    assert "bandbatch_stats" in N.TYPED_SYMBOLS and "bandbatch_thresh" in N.TYPED_SYMBOLS
    for name in ENTRIES:
        assert re.search(r"\bint %s\(" % name, header), name
        assert getattr(L, name).argtypes is not None, name
    batch_h = open(os.path.join(ROOT, "include", "wt_batch.h")).read()
    for dt in (np.float32, np.float64):
        H = N.host(dt)
        for m in HANDLE:
            assert getattr(H, "pdwt_images_" + m).argtypes is not None, m
            assert re.search(r"\b%s\(" % m, batch_h), m
    for m in ("nbands", "all_band_stats", "estimate_sigma", "threshold_bands", "denoise", "norm1"):
        assert hasattr(pdwt_amd.ImageBatch, m), m


@pytest.mark.parametrize("sfx,ct", [("f32", C.c_float), ("f64", C.c_double)])
def test_cabi_entries_check_their_arguments(sfx, ct):
    L = pdwt_amd.hip()
    stats, thresh = getattr(L, "pdwt_bandbatch_stats_" + sfx), getattr(L, "pdwt_bandbatch_thresh_" + sfx)
    tab = C.c_void_p(256)  # (never dereferenced: every call below is refused, or has nothing to do)
    n = (C.c_size_t * 98)()
    want = (C.c_ubyte * 98)()
    out = (N.BandStats * 98)()
    beta = (ct * 98)()
    for nb in (0, -3, 98):
        assert stats(tab, n, 1, nb, want, out) == PDWT_EINVAL
        assert thresh(0, tab, n, beta, 1, nb) == PDWT_EINVAL
    for B in (0, -1):
        assert stats(tab, n, B, 1, want, out) == PDWT_EINVAL
        assert thresh(0, tab, n, beta, B, 1) == PDWT_EINVAL
    assert stats(None, n, 1, 1, want, out) == PDWT_EINVAL
    assert stats(tab, None, 1, 1, want, out) == PDWT_EINVAL
    assert stats(tab, n, 1, 1, want, None) == PDWT_EINVAL
    assert thresh(0, None, n, beta, 1, 1) == PDWT_EINVAL
    assert thresh(0, tab, n, None, 1, 1) == PDWT_EINVAL
    assert thresh(2, tab, n, beta, 1, 1) == PDWT_EINVAL
    assert thresh(-1, tab, n, beta, 1, 1) == PDWT_EINVAL


def test_empty_bands_give_zeros_and_a_nan_median_without_a_device():
    L = pdwt_amd.hip()
    tab = C.c_void_p(256)
    n = (C.c_size_t * 2)(0, 0)
    want = (C.c_ubyte * 2)(1, 0)
    out = (N.BandStats * 6)()
    assert L.pdwt_bandbatch_stats_f32(tab, n, 3, 2, want, out) == 0
    for i in range(6):
        d = out[i].as_dict()
        assert (d["n"], d["sum_abs"], d["sum_sq"], d["max_abs"]) == (0, 0, 0, 0) and np.isnan(d["median_abs"])
    assert L.pdwt_bandbatch_thresh_f32(0, tab, n, (C.c_float * 6)(*[1] * 6), 3, 2) == 0  # nothing to do, nothing launched
    n[0] = n[1] = 100
    assert L.pdwt_bandbatch_thresh_f64(1, tab, n, (C.c_double * 6)(*[-1] * 6), 3, 2) == 0  # every beta negative: nothing launched


class _NoHandle:
    """stands in for the native library: the argument checks below must fail before any of its functions is called, except num_bands"""

    def __init__(self, nb):
        self.nb = nb

    def pdwt_images_num_bands(self, h):
        return self.nb

    def __getattr__(self, name):
        raise AssertionError("the native handle was used: " + name)


def _surface(B=3, nb=7, dtype=np.float32):
    b = pdwt_amd.ImageBatch.__new__(pdwt_amd.ImageBatch)
    b.dtype, b.shape, b.wname, b._L, b._h = np.dtype(dtype), (B, 64, 64), "db2", _NoHandle(nb), None
    return b


def test_python_surface_checks_its_arguments():
    b = _surface()
    assert b.nbands == 7
    for bad in ([1.0] * 6, np.ones((4, 7)), np.ones((3, 6)), np.ones((7, 3)), 1.0):
        with pytest.raises(ValueError):
            b.threshold_bands(bad)
    with pytest.raises(ValueError):
        b.threshold_bands(np.ones((3, 7)), kind="firm")
    with pytest.raises(ValueError):
        b.denoise("sure")
    with pytest.raises(ValueError):
        b.denoise("bayes", kind="garrote")
    for bad in (-2.0, [1.0] * 4, [1.0, -1.0, 1.0], np.ones((3, 1)), float("nan")):
        with pytest.raises(ValueError):
            b.denoise("visu", sigma=bad)


def test_isa_audit_flags_no_kernel_of_bandbatch():
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"):
        pytest.skip("no llvm-objdump")
    spec = importlib.util.spec_from_file_location("isa_audit", os.path.join(ROOT, "tools", "isa_audit.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mine = [r for r in mod.audit() if "k_bb_" in r[0]]  # (mangled names)
    # moments 2, combine 1, select_wg 2, hist 2, pick 1, thresh 2 x 2
    assert len(mine) == 12, [r[0] for r in mine]
    for name, c, m in mine:
        tot = sum(c.values())
        assert c["v_readlane_b32"] <= 0.02 * tot, (name, c["v_readlane_b32"], tot)
        assert not any(op.startswith("scratch_") for op in c), name
        assert m.get("vgpr_spill_count", 0) == 0 and m.get("sgpr_spill_count", 0) == 0 and m.get("private_segment_fixed_size", 0) == 0, (name, m)
