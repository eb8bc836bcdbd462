"""CPU-only checks of the 3-D stationary transform: the pdwt_*swt3d* C-ABI is declared and exported, include/swt3d.h is plain host
C++, pdwt_amd.StationaryWavelets3D is importable, the band table follows the documented layout (7L+1 full-size bands), and the
numpy restatement of the dilated 1-D a-trous level -- the reference of tests/test_swt3d_gpu.py -- is pinned against the oracle's
multi-level 1-D SWT."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import pdwt_amd
from pdwt_amd import _native as N
from oracle import oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ABI_SWT3D = ["pdwt_num_bands_swt3d", "pdwt_band_size_swt3d", "pdwt_tmp_elems_swt3d"] + [
    "pdwt_%s_%s" % (n, s) for n in ("create_coeffs_buffer_swt3d", "free_coeffs_buffer_swt3d", "forward3d_swt", "inverse3d_swt",
                                    "soft_thresh_swt3d", "hard_thresh_swt3d", "norm1_swt3d") for s in ("f32", "f64")]
HANDLES_SWT3D = ["pdwt_swt3d_" + n for n in ("new", "delete", "forward", "inverse", "soft_threshold", "hard_threshold", "norm1",
                                              "norm1_f64", "get_image", "set_image", "num_bands", "band_shape", "get_coeff",
                                              "set_coeff", "state", "info", "image_int_ptr", "coeff_int_ptr")]


# ---- the numpy restatement of one a-trous level along an axis (SURVEY A-3 / A-4) ---------------------------------------
def bank(wname, dtype):
    """(L, H, IL, IH) of a bank as numpy arrays of dtype"""
    _, F, _ = orc.filters(wname, dtype, do_swt=1)
    return F["L"], F["H"], F["IL"], F["IH"]


def atrous_ana(x, axis, F, f):
    """lo, hi along `axis` at tap spacing f: out[g] = sum_k x[(g - c + f*k) mod n] * F[hlen-1-k], c = (hlen/2 - 1)*f"""
    FL, FH = F[0], F[1]
    hlen = len(FL)
    c = (hlen // 2 - 1) * f
    lo, hi = np.zeros_like(x), np.zeros_like(x)
    for k in range(hlen):
        s = np.roll(x, c - f * k, axis=axis)  # s[g] = x[(g - c + f*k) mod n]
        lo = lo + s * FL[hlen - 1 - k]
        hi = hi + s * FH[hlen - 1 - k]
    return lo, hi


def atrous_syn(a, d, axis, F, f):
    """the a-trous synthesis along `axis`: c = (hlen/2)*f, each of the two sums of products halved"""
    FIL, FIH = F[2], F[3]
    hlen = len(FIL)
    c = (hlen // 2) * f
    sa, sd = np.zeros_like(a), np.zeros_like(a)
    for k in range(hlen):
        sa = sa + np.roll(a, c - f * k, axis=axis) * FIL[hlen - 1 - k] / 2
        sd = sd + np.roll(d, c - f * k, axis=axis) * FIH[hlen - 1 - k] / 2
    return sa + sd


def test_abi_swt3d_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "pdwt_hip.h")).read()
    declared = set(re.findall(r"\b(pdwt_[a-z0-9_]+)\s*\(", hdr))
    L = pdwt_amd.hip()
    for s in ABI_SWT3D:
        assert s in declared, s
        assert hasattr(L, s), s


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_host_libraries_export_swt3d_handles(dtype):
    L = N.host(dtype)
    missing = [s for s in HANDLES_SWT3D if not hasattr(L, s)]
    assert not missing, missing


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
@pytest.mark.parametrize("flags", [[], ["-DDOUBLEPRECISION"]])
def test_swt3d_header_is_plain_host_cpp(tmp_path, flags):
    src = tmp_path / "use_swt3d.cpp"
    src.write_text('#include "swt3d.h"\n'
                   "int use(DTYPE* v) {\n"
                   "    StationaryWavelets3D W(v, 8, 8, 8, \"haar\", 1);\n"
                   "    W.forward(); W.soft_threshold((DTYPE)1, 1, 1); W.hard_threshold((DTYPE)1); W.inverse();\n"
                   "    DTYPE n = W.norm1(); (void)n; (void)W.image_int_ptr(); (void)W.coeff_int_ptr(1); (void)W.norm1_double();\n"
                   "    W.set_image(v); W.set_coeff(v, 1); return W.get_image(v) + W.get_coeff(v, 0) + (int)W.state + W.num_bands();\n"
                   "}\n")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include")] + flags + [str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    includes = re.findall(r'^\s*#\s*include\s*[<"]([^>"]+)[>"]', open(os.path.join(ROOT, "include", "swt3d.h")).read(), re.M)
    assert includes == ["wt3d.h"], includes


def test_stationary_wavelets3d_is_exported():
    assert pdwt_amd.StationaryWavelets3D.__module__ == "pdwt_amd.swt3d"
    assert "StationaryWavelets3D" in pdwt_amd.__all__


@pytest.mark.parametrize("dims,L,hlen", [((64, 64, 64), 3, 8), ((33, 47, 61), 2, 8), ((8, 256, 256), 1, 8), ((9, 13, 7), 2, 2),
                                         ((256, 256, 256), 2, 40), ((5, 3, 7), 1, 2)])
def test_band_geometry_swt3d(dims, L, hlen):
    H = pdwt_amd.hip()
    info = N.Info3D(dims[0], dims[1], dims[2], L, hlen)
    V = dims[0] * dims[1] * dims[2]
    assert H.pdwt_num_bands_swt3d(info) == 7 * L + 1
    for k in range(7 * L + 1):
        z, r, c = C.c_int(), C.c_int(), C.c_int()
        assert H.pdwt_band_size_swt3d(info, k, C.byref(z), C.byref(r), C.byref(c)) == V
        assert (z.value, r.value, c.value) == dims, k
    assert H.pdwt_band_size_swt3d(info, 7 * L + 1, None, None, None) < 0
    assert H.pdwt_band_size_swt3d(info, -1, None, None, None) < 0
    # scratch: the four full-size x-y quadrants of a level
    assert 4 * V <= H.pdwt_tmp_elems_swt3d(info) <= 4 * (V + 64)


def test_bad_swt3d_geometry_is_refused():
    H = pdwt_amd.hip()
    for bad in (N.Info3D(0, 8, 8, 1, 2), N.Info3D(8, 8, 8, 0, 2), N.Info3D(8, -1, 8, 1, 2), N.Info3D(2, 65536, 32768, 1, 2),
                N.Info3D(65536, 8, 8, 1, 2),  # a plane of 2^31 elements; more than 65535 planes
                N.Info3D(7, 64, 64, 1, 8),  # (hlen - 1) * 2^(L-1) = 7 is not below min(N) = 7
                N.Info3D(64, 64, 64, 5, 8),  # 7 * 16 >= 64: above the level clamp
                N.Info3D(64, 64, 64, 1, 7), N.Info3D(64, 64, 64, 1, 0), N.Info3D(64, 64, 64, 1, 42)):  # no such bank length
        assert H.pdwt_num_bands_swt3d(bad) < 0
        assert H.pdwt_tmp_elems_swt3d(bad) == 0
        assert H.pdwt_band_size_swt3d(bad, 0, None, None, None) < 0


def test_large_volumes_are_accepted():
    # a volume past 2^31 elements is fine as long as a plane is below it: 2048^3 float32
    H = pdwt_amd.hip()
    info = N.Info3D(2048, 2048, 2048, 3, 8)
    assert H.pdwt_num_bands_swt3d(info) == 22
    assert H.pdwt_band_size_swt3d(info, 0, None, None, None) == 2048 ** 3
    assert H.pdwt_tmp_elems_swt3d(info) >= 4 * 2048 ** 3


# ---- the restatement against the oracle's multi-level 1-D SWT ---------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("wname,n", [("haar", 37), ("db2", 64), ("db4", 101), ("sym8", 255), ("coif3", 200), ("db20", 311)])
def test_atrous_restatement_vs_oracle_1d_swt(wname, n, dtype):
    dt = np.dtype(dtype)
    tol = 1e-5 if dt == np.float32 else 1e-12
    F = bank(wname, dt)
    lines = np.random.RandomState(n).uniform(-10, 10, (5, n)).astype(dt)
    O = orc.OracleWavelets(lines, wname, 99, do_swt=1, ndim=1)
    L = O.info.nlevels
    assert L == orc.ilog2(n // (len(F[0]) - 1)) >= 1
    O.forward()
    got = O.coeffs  # [A_L, D_1 .. D_L]
    a, details = lines, []
    for lev in range(1, L + 1):
        a, d = atrous_ana(a, 1, F, 2 ** (lev - 1))
        details.append(d)
    from tests.helpers import band_err
    assert band_err(got[0], a) <= tol, (wname, n)
    for lev in range(1, L + 1):
        assert band_err(got[lev], details[lev - 1]) <= tol, (wname, n, lev)
    # synthesis of the oracle's bands, level by level
    O.inverse()
    r = got[0]
    for lev in range(L, 0, -1):
        r = atrous_syn(r, got[lev], 1, F, 2 ** (lev - 1))
    assert band_err(r, O.get_image()) <= tol, (wname, n)
    assert band_err(r, lines) <= 10 * tol, (wname, n)
