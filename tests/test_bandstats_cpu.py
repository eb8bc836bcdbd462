"""CPU-only checks of the band statistics feature: the numpy restatement itself, the argument checks of the new C-ABI entries (no
device is touched), the Python surface, and the ISA audit of the kernels of bandstats.hip."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import pdwt_amd
from pdwt_amd import _native as N
from tests.refstats import ref_stats, ref_threshold

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PDWT_EINVAL = -1


@pytest.mark.parametrize("n", [1, 2, 3, 17, 18, 1000, 4097])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_restated_median_is_numpy_median(n, dtype):
    x = np.random.default_rng(n).standard_normal(n).astype(dtype)
    x[::7] = -0.0
    s = ref_stats(x)
    assert s["median_abs"] == float(np.median(np.abs(x).astype(np.float64)))
    assert s["n"] == n and s["max_abs"] == float(np.abs(x).max())


def test_restated_threshold_keeps_untouched_bands_and_signed_zeros():
    x = np.array([-2.0, -0.5, -0.0, 0.0, 0.5, 2.0], dtype=np.float32)
    assert np.array_equal(ref_threshold(x, -1.0, "soft"), x)
    s, h = ref_threshold(x, 1.0, "soft"), ref_threshold(x, 1.0, "hard")
    assert np.array_equal(s, [-1, -0.0, -0.0, 0, 0, 1]) and np.array_equal(np.signbit(s), [1, 1, 1, 0, 0, 0])
    assert np.array_equal(h, [-2, -0.0, -0.0, 0, 0, 2]) and np.array_equal(np.signbit(h), [1, 1, 1, 0, 0, 0])


@pytest.mark.parametrize("sfx,ct", [("f32", C.c_float), ("f64", C.c_double)])
def test_new_cabi_entries_check_their_arguments(sfx, ct):
    L = pdwt_amd.hip()
    stats, thresh = getattr(L, "pdwt_bandlist_stats_" + sfx), getattr(L, "pdwt_bandlist_thresh_" + sfx)
    P = C.POINTER(ct)
    ptr = (P * 98)()
    n = (C.c_size_t * 98)()
    want = (C.c_ubyte * 98)()
    out = (N.BandStats * 98)()
    beta = (ct * 98)()
    for nb in (0, -3, 98):
        assert stats(ptr, n, nb, want, out) == PDWT_EINVAL
        assert thresh(0, ptr, n, beta, nb) == PDWT_EINVAL
    assert stats(None, n, 1, want, out) == PDWT_EINVAL
    assert stats(ptr, None, 1, want, out) == PDWT_EINVAL
    assert stats(ptr, n, 1, want, None) == PDWT_EINVAL
    assert thresh(0, None, n, beta, 1) == PDWT_EINVAL
    assert thresh(0, ptr, None, beta, 1) == PDWT_EINVAL
    assert thresh(0, ptr, n, None, 1) == PDWT_EINVAL
    assert thresh(2, ptr, n, beta, 1) == PDWT_EINVAL and thresh(-1, ptr, n, beta, 1) == PDWT_EINVAL
    n[0] = 5  # elements behind a null band pointer
    assert stats(ptr, n, 1, want, out) == PDWT_EINVAL


def test_empty_bands_give_zeros_and_a_nan_median_without_a_device():
    L = pdwt_amd.hip()
    ptr = (C.POINTER(C.c_float) * 2)()
    n = (C.c_size_t * 2)(0, 0)
    want = (C.c_ubyte * 2)(1, 0)
    out = (N.BandStats * 2)()
    assert L.pdwt_bandlist_stats_f32(ptr, n, 2, want, out) == 0
    for k in range(2):
        d = out[k].as_dict()
        assert (d["n"], d["sum_abs"], d["sum_sq"], d["max_abs"]) == (0, 0, 0, 0) and np.isnan(d["median_abs"])
    assert L.pdwt_bandlist_thresh_f32(0, ptr, n, (C.c_float * 2)(1, 1), 2) == 0  # nothing to do, nothing launched


def test_python_classes_expose_the_five_methods():
    for cls in (pdwt_amd.Wavelets, pdwt_amd.Wavelets3D, pdwt_amd.StationaryWavelets3D):
        for m in ("band_stats", "all_band_stats", "estimate_sigma", "threshold_bands", "denoise"):
            assert callable(getattr(cls, m)), (cls, m)
    for dt in (np.float32, np.float64):
        H = N.host(dt)
        for pfx in ("pdwt_wavelets_", "pdwt_wavelets3d_", "pdwt_swt3d_"):
            for m in ("band_stats", "all_band_stats", "estimate_sigma", "threshold_bands", "denoise"):
                assert hasattr(H, pfx + m), pfx + m


def test_isa_audit_flags_no_kernel_of_bandstats():
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump"):
        pytest.skip("no llvm-objdump")
    spec = importlib.util.spec_from_file_location("isa_audit", os.path.join(ROOT, "tools", "isa_audit.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mine = [r for r in mod.audit() if any(k in r[0] for k in ("k_band_moments", "k_band_hist", "k_band_pick"))]  # (mangled names)
    assert len(mine) == 14, [r[0] for r in mine]  # moments 2 x 2, hist 2 x 2 x 2, pick 2
    for name, c, m in mine:
        tot = sum(c.values())
        assert c["v_readlane_b32"] <= 0.02 * tot, (name, c["v_readlane_b32"], tot)
        assert not any(op.startswith("scratch_") for op in c), name
        assert m.get("vgpr_spill_count", 0) == 0 and m.get("private_segment_fixed_size", 0) == 0, (name, m)
