"""CPU-only transcript of the host side of the three wavelet packet classes (include/wpt.h, include/wpt1d.h, include/wpt_batch.h;
pdwt_amd/csrc/wpt.cpp) through their flat handle APIs: constructions that fail before any device allocation, then every handle function
on the failed instance.  Pins the messages the classes print, byte for byte, and what the functions return in state W_CREATION_ERROR,
for the three classes and both precisions; and the handle functions that take no instance (geometry, path_index, frequency_order).  The
messages that need a device (the state machine after a forward()) are in test_packets_state_gpu.py."""
import ctypes as C

import numpy as np
import pytest

from pdwt_amd import _native as N

# prefix -> (class name, noun of its size message, info struct, info fields)
CLASSES = {
    "pdwt_wpt_": ("WaveletPackets", "image", N.InfoWPT, ("Nr", "Nc", "nlevels", "hlen")),
    "pdwt_wp1h_": ("WaveletPackets1D", "batch", N.InfoWPT1, ("Nr", "Nc", "nlevels", "hlen")),
    "pdwt_wpbh_": ("WaveletPacketsImages", "image", N.InfoWPTB, ("B", "Nr", "Nc", "nlevels", "hlen")),
}

FORCE1 = "Warning: cannot initialize wavelet coefficients with nlevels < 1. Forcing nlevels = 1\n"
SMALL = {
    "pdwt_wpt_": "Warning: required level (1) is greater than the maximum possible level for db4 packets (0) on a 6x6 image.\nForcing nlevels = 0\n"
                 "ERROR: a 6x6 image is too small for one level of db4\n",
    "pdwt_wp1h_": "Warning: required level (1) is greater than the maximum possible level for db4 packets (0) on rows of 6 samples.\nForcing nlevels = 0\n"
                  "ERROR: rows of 6 samples are too short for one level of db4\n",
}
INVALID = "ERROR: {C}(): invalid {noun} size or wavelet name\n"
# the single-image and the 1-D class: case -> ((Nr, Nc, wname, levels), what the constructor prints ({C}: the class name, {noun}: its
# noun; a dict where the two differ by more than that), info)
CASES_2 = {
    "zero size": ((0, 8, b"haar", 1), INVALID, "0 8 1 0"),
    "2^31 elements": ((65536, 32768, b"haar", 1), INVALID, "65536 32768 1 0"),
    "no name": ((8, 8, None, 1), INVALID, "8 8 1 0"),
    "unknown wavelet": ((8, 8, b"nosuchwavelet", 1), "ERROR: unknown wavelet name nosuchwavelet\n", "8 8 1 0"),
    "too small": ((6, 6, b"db4", 1), SMALL, "6 6 0 8"),
    "levels 0": ((6, 6, b"db4", 0), {k: FORCE1 + v for k, v in SMALL.items()}, "6 6 0 8"),
}
# the batch class: case -> ((B, Nr, Nc, wname, levels), what the constructor prints, info)
CASES_B = {
    "no images": ((0, 64, 64, b"db4", 3), "ERROR: WaveletPacketsImages(): a batch holds 1 .. 65535 images (0 given)\n", "0 64 64 3 0"),
    "too many images": ((65536, 64, 64, b"db4", 3), "ERROR: WaveletPacketsImages(): a batch holds 1 .. 65535 images (65536 given)\n", "65536 64 64 3 0"),
    "bad size": ((4, 0, 64, b"db4", 3), "ERROR: WaveletPacketsImages(): invalid image size or wavelet name\n", "4 0 64 3 0"),
    "2^31 elements": ((4, 65536, 32768, b"db4", 3), "ERROR: WaveletPacketsImages(): invalid image size or wavelet name\n", "4 65536 32768 3 0"),
    "no name": ((4, 64, 64, None, 3), "ERROR: WaveletPacketsImages(): invalid image size or wavelet name\n", "4 64 64 3 0"),
    "unknown wavelet": ((4, 64, 64, b"nosuchwavelet", 3), "ERROR: unknown wavelet name nosuchwavelet\n", "4 64 64 3 0"),
    "too small": ((4, 6, 64, b"db4", 2),
                  "Warning: required level (2) is greater than the maximum possible level for db4 packets (0) on a 6x64 image.\nForcing nlevels = 0\n"
                  "ERROR: a 6x64 image is too small for one level of db4\n", "4 6 64 0 8"),
    "too many nodes": ((65535, 64, 64, b"haar", 4), "ERROR: WaveletPacketsImages(): 65535 images of 256 nodes exceed 2^22 nodes per depth\n", "65535 64 64 4 2"),
    "levels 0": ((4, 6, 64, b"db4", 0),
                 FORCE1 + "Warning: required level (1) is greater than the maximum possible level for db4 packets (0) on a 6x64 image.\nForcing nlevels = 0\n"
                 "ERROR: a 6x64 image is too small for one level of db4\n", "4 6 64 0 8"),
}

# One line per call, "name -> return value" (the name alone for a void function), then what the call printed: the same after every failed
# construction (state 4 = W_CREATION_ERROR).  {F}: "fused -> 0\n" for the classes that have it, {I1} / {I2}: the images_* lines of the
# batch class.
EXPECTED_METHODS = """state -> 4
{F}node_shape -> 0
forward
Warning: forward transform not computed, as there was an error when creating the wavelets
inverse
Warning: inverse transform not computed, as there was an error in a previous stage
get_image -> 0
set_image
get_node -> 0
get_level -> 0
set_node -> 0
Warning: set_node(): refused, the tree does not hold the coefficients of a forward() (run forward() first)
node_int_ptr -> 0
node_costs -> -1
best_basis -> -1
set_basis -> -1
basis_size -> 0
get_basis -> 0
soft_threshold
hard_threshold
norm1 -> -1.0
{I1}node_stats -> -1
estimate_sigma -> -1.0
{I2}state -> 4
delete
"""
VOID = ("delete", "forward", "inverse", "soft_threshold", "hard_threshold", "set_image")


def transcript(pfx, dtype, args, capfd):
    L = N.host(dtype)
    libc = C.CDLL(None)
    ct = C.c_float if np.dtype(dtype) == np.float32 else C.c_double
    _, _, info_t, fields = CLASSES[pfx]
    batch, one_d = pfx == "pdwt_wpbh_", pfx == "pdwt_wp1h_"
    lines = []

    def call(name, *a, show=None):
        capfd.readouterr()
        ret = getattr(L, pfx + name)(*a)
        libc.fflush(None)
        lines.append(name if name in VOID else "%s -> %s" % (name, show(ret) if show else ret))
        lines.extend(capfd.readouterr().out.splitlines())
        return ret

    h = call("new", None, *args, show=lambda r: "handle" if r else "NULL")
    assert h
    info = info_t()
    call("info", h, C.byref(info), show=lambda r: " ".join(str(getattr(info, f)) for f in fields))
    buf = np.zeros(64, dtype=dtype)
    p = buf.ctypes.data_as(C.c_void_p)
    dbl = (C.c_double * 8)()
    ints = (C.c_int * 8)()
    stats = (N.BandStats * 8)()
    call("state", h)
    if batch or one_d:
        call("fused", h)
    call("node_shape", h, 1, None, None)
    call("forward", h)
    call("inverse", h)
    call("get_image", h, p)
    call("set_image", h, p, 0)
    call("get_node", h, p, 1, 0)
    call("get_level", h, p, 1)
    call("set_node", h, p, 1, 0, 0)
    call("node_int_ptr", h, 1, 0, *(() if pfx == "pdwt_wpt_" else (None,)))
    call("node_costs", h, 1, 0, dbl, *(() if pfx == "pdwt_wpt_" else (dbl,)))
    call("best_basis", h, 0)
    call("set_basis", h, ints, ints, 1)
    call("basis_size", h)
    call("get_basis", h, ints, ints)
    call("soft_threshold", h, ct(1.0), 1)
    call("hard_threshold", h, ct(1.0), 0)
    call("norm1", h)
    if batch:
        call("images_norm1", h, dbl)
    call("node_stats", h, 1, stats)
    call("estimate_sigma", h)
    if batch:
        call("images_estimate_sigma", h, dbl)
    call("state", h)
    call("delete", h)
    return "\n".join(lines) + "\n"


ROWS = [(pfx, case) for pfx in ("pdwt_wpt_", "pdwt_wp1h_") for case in CASES_2] + [("pdwt_wpbh_", case) for case in CASES_B]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("pfx,case", ROWS)
def test_failed_construction_transcript(pfx, case, dtype, capfd):
    cls, noun, _, _ = CLASSES[pfx]
    batch = pfx == "pdwt_wpbh_"
    args, head, info = (CASES_B if batch else CASES_2)[case]
    head = head[pfx] if isinstance(head, dict) else head
    got = transcript(pfx, dtype, args + ((1, 1) if batch else (1,)), capfd)
    methods = EXPECTED_METHODS.format(F="" if pfx == "pdwt_wpt_" else "fused -> 0\n", I1="images_norm1 -> -1\n" if batch else "",
                                      I2="images_estimate_sigma -> -1\n" if batch else "")
    assert got == "new -> handle\n" + head.format(C=cls, noun=noun) + "info -> " + info + "\n" + methods


def test_static_handle_functions():
    """The handle functions that take no instance.  geometry: the level clamp (to 7 for the quad-trees, 12 for the binary tree) with the node
    sizes per depth, 0 for a size or a bank no instance can have; path_index: the node a path names, -1 for a bad letter or a path one
    deeper than the deepest tree; frequency_order: the Gray-code permutation of a depth."""
    L = N.host(np.float32)
    for pfx in ("pdwt_wpt_", "pdwt_wpbh_"):
        geometry, path_index = getattr(L, pfx + "geometry"), getattr(L, pfx + "path_index")
        nr, nc = (C.c_int * 9)(*[-7] * 9), (C.c_int * 9)(*[-7] * 9)
        assert geometry(37, 51, 6, 2, nr, nc) == 2 and (list(nr[:4]), list(nc[:4])) == ([37, 19, 10, -7], [51, 26, 13, -7])
        assert geometry(37, 51, 6, 9, None, None) == 2 and geometry(37, 51, 6, 0, None, None) == 1 and geometry(37, 51, 6, -3, None, None) == 1
        assert geometry(1 << 14, 1 << 14, 2, 40, nr, nc) == 7 and list(nr) == [1 << (14 - l) for l in range(8)] + [-7] == list(nc)  # WPT_MAX_LEVELS
        assert geometry(6, 64, 8, 1, None, None) == 0 and geometry(0, 5, 2, 1, None, None) == 0 and geometry(5, -1, 2, 1, None, None) == 0
        assert geometry(65536, 32768, 2, 1, None, None) == 0 and geometry(64, 64, 1, 1, None, None) == 0
        d = C.c_int(-7)
        assert path_index(b"", C.byref(d)) == 0 and d.value == 0
        assert path_index(b"ahd", C.byref(d)) == 7 and d.value == 3
        assert path_index(b"ddddddd", C.byref(d)) == 4 ** 7 - 1 and d.value == 7 and path_index(b"v", None) == 2
        d = C.c_int(-7)
        assert path_index(b"ahx", C.byref(d)) == -1 and path_index(b"aaaaaaaa", C.byref(d)) == -1 and path_index(None, C.byref(d)) == -1 and d.value == -7
    n = (C.c_int * 14)(*[-7] * 14)
    assert L.pdwt_wp1h_geometry(48, 4, 3, n) == 3 and list(n[:5]) == [48, 24, 12, 6, -7]
    assert L.pdwt_wp1h_geometry(51, 6, 9, n) == 3 and list(n[:5]) == [51, 26, 13, 7, -7]
    assert L.pdwt_wp1h_geometry(48, 4, 0, None) == 1
    assert L.pdwt_wp1h_geometry(1 << 20, 2, 40, n) == 12 and list(n) == [1 << (20 - l) for l in range(13)] + [-7]  # WPT1D_MAX_LEVELS
    assert L.pdwt_wp1h_geometry(6, 8, 1, None) == 0 and L.pdwt_wp1h_geometry(0, 2, 1, None) == 0 and L.pdwt_wp1h_geometry(64, 1, 1, None) == 0
    assert L.pdwt_wp1h_geometry(64, 3, 1, None) == 0
    d = C.c_int(-7)
    assert L.pdwt_wp1h_path_index(b"", C.byref(d)) == 0 and d.value == 0
    assert L.pdwt_wp1h_path_index(b"ad", C.byref(d)) == 1 and d.value == 2
    assert L.pdwt_wp1h_path_index(b"d" * 12, C.byref(d)) == 4095 and d.value == 12 and L.pdwt_wp1h_path_index(b"d", None) == 1
    d = C.c_int(-7)
    assert L.pdwt_wp1h_path_index(b"ah", C.byref(d)) == -1 and L.pdwt_wp1h_path_index(b"a" * 13, C.byref(d)) == -1
    assert L.pdwt_wp1h_path_index(None, C.byref(d)) == -1 and d.value == -7
    out = (C.c_int * 9)(*[-7] * 9)
    assert L.pdwt_wp1h_frequency_order(3, out) == 8 and list(out) == [0, 1, 3, 2, 6, 7, 5, 4, -7]
    assert L.pdwt_wp1h_frequency_order(0, out) == 1 and out[0] == 0
    assert L.pdwt_wp1h_frequency_order(-1, out) == 0 and L.pdwt_wp1h_frequency_order(13, out) == 0 and L.pdwt_wp1h_frequency_order(3, None) == 0
