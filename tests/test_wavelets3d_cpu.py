"""CPU-only checks of the 3-D transform's interface: the pdwt_*3d* C-ABI is declared and exported, include/wt3d.h is plain host
C++, pdwt_amd.Wavelets3D is importable, and the band table follows the documented layout (7 detail bands per level, coarsest
level first, ceil-half sizes along every axis)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import pdwt_amd
from pdwt_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ABI3D = ["pdwt_num_bands3d", "pdwt_band_size3d", "pdwt_tmp_elems3d"] + [
    "pdwt_%s_%s" % (n, s) for n in ("create_coeffs_buffer3d", "free_coeffs_buffer3d", "forward3d_separable", "inverse3d_separable",
                                    "soft_thresh3d", "hard_thresh3d", "norm1_3d") for s in ("f32", "f64")]
HANDLES3D = ["pdwt_wavelets3d_" + n for n in ("new", "delete", "forward", "inverse", "soft_threshold", "hard_threshold", "norm1",
                                               "norm1_f64", "get_image", "set_image", "num_bands", "band_shape", "get_coeff",
                                               "set_coeff", "state", "info", "image_int_ptr", "coeff_int_ptr")]


def _div2(n):
    return (n + 1) // 2


def _layout(Nz, Nr, Nc, L):
    """[A_L, then levels L .. 1: aad, ada, add, daa, dad, dda, ddd] with the level's ceil-halved shape"""
    def shape(lev):
        s = (Nz, Nr, Nc)
        for _ in range(lev):
            s = tuple(_div2(v) for v in s)
        return s
    out = [shape(L)]
    for lev in range(L, 0, -1):
        out += [shape(lev)] * 7
    return out


def test_abi3d_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "pdwt_hip.h")).read()
    declared = set(re.findall(r"\b(pdwt_[a-z0-9_]+)\s*\(", hdr))
    assert "typedef struct pdwt_info3d" in hdr
    L = pdwt_amd.hip()
    for s in ABI3D:
        assert s in declared, s
        assert hasattr(L, s), s


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_host_libraries_export_wavelets3d_handles(dtype):
    L = N.host(dtype)
    missing = [s for s in HANDLES3D if not hasattr(L, s)]
    assert not missing, missing


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
@pytest.mark.parametrize("flags", [[], ["-DDOUBLEPRECISION"]])
def test_wt3d_header_is_plain_host_cpp(tmp_path, flags):
    src = tmp_path / "use_wt3d.cpp"
    src.write_text('#include "wt3d.h"\n'
                   "#include \"wt.h\"\n"
                   "int use(DTYPE* v) {\n"
                   "    Wavelets3D W(v, 8, 8, 8, \"haar\", 1);\n"
                   "    W.forward(); W.soft_threshold((DTYPE)1, 1, 1); W.hard_threshold((DTYPE)1); W.inverse();\n"
                   "    DTYPE n = W.norm1(); (void)n; (void)W.image_int_ptr(); (void)W.coeff_int_ptr(1);\n"
                   "    W.set_image(v); W.set_coeff(v, 1); return W.get_image(v) + W.get_coeff(v, 0) + (int)W.state;\n"
                   "}\n")
    # no HIP include path: the header must not need one
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include")] + flags + [str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    includes = re.findall(r'^\s*#\s*include\s*[<"]([^>"]+)[>"]', open(os.path.join(ROOT, "include", "wt3d.h")).read(), re.M)
    assert includes == ["wt.h"], includes


def test_wavelets3d_is_exported():
    assert pdwt_amd.Wavelets3D.__module__ == "pdwt_amd.wavelets3d"
    assert "Wavelets3D" in pdwt_amd.__all__
    from pdwt_amd.wavelets3d import BAND_KEYS
    assert BAND_KEYS == ("aad", "ada", "add", "daa", "dad", "dda", "ddd")


@pytest.mark.parametrize("dims,L", [((64, 64, 64), 3), ((33, 47, 61), 2), ((16, 256, 256), 2), ((96, 80, 72), 4), ((1, 1, 1), 1),
                                    ((7, 2, 5), 3)])
def test_band_geometry_3d(dims, L):
    H = pdwt_amd.hip()
    info = N.Info3D(dims[0], dims[1], dims[2], L, 8)
    want = _layout(*dims, L)
    assert H.pdwt_num_bands3d(info) == len(want) == 7 * L + 1
    for k, s in enumerate(want):
        z, r, c = C.c_int(), C.c_int(), C.c_int()
        assert H.pdwt_band_size3d(info, k, C.byref(z), C.byref(r), C.byref(c)) == s[0] * s[1] * s[2]
        assert (z.value, r.value, c.value) == s, k
    assert H.pdwt_band_size3d(info, len(want), None, None, None) < 0
    assert H.pdwt_band_size3d(info, -1, None, None, None) < 0
    # scratch: the four x-y quadrants of level 1 and one level-1 approximation
    h = [_div2(v) for v in dims]
    assert H.pdwt_tmp_elems3d(info) >= 4 * dims[0] * h[1] * h[2] + h[0] * h[1] * h[2]


def test_large_volumes_are_accepted():
    # a volume past 2^31 elements is fine as long as a plane is below it: 2048^3 float32 (32 GB)
    H = pdwt_amd.hip()
    info = N.Info3D(2048, 2048, 2048, 3, 8)
    assert H.pdwt_num_bands3d(info) == 22
    assert H.pdwt_band_size3d(info, 0, None, None, None) == 256 ** 3
    assert H.pdwt_tmp_elems3d(info) >= 4 * 2048 * 1024 * 1024 + 1024 ** 3


def test_bad_3d_geometry_is_refused():
    H = pdwt_amd.hip()
    for bad in (N.Info3D(0, 8, 8, 1, 2), N.Info3D(8, 8, 8, 0, 2), N.Info3D(8, -1, 8, 1, 2), N.Info3D(8, 8, 8, 14, 2),
                N.Info3D(2, 65536, 32768, 1, 2), N.Info3D(65536, 8, 8, 1, 2)):  # (a plane of 2^31 elements; more than 65535 planes)
        assert H.pdwt_num_bands3d(bad) < 0
        assert H.pdwt_tmp_elems3d(bad) == 0
        assert H.pdwt_band_size3d(bad, 0, None, None, None) < 0
