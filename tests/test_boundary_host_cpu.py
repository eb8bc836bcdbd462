"""CPU-only transcript of the host side of the three boundary-mode classes (include/wt_ext.h; pdwt_amd/csrc/wt_ext.cpp) through their
flat handle APIs: constructions that fail before any device allocation, then every method on the failed instance.  Pins the messages
the classes print, byte for byte, and what the methods return in state W_CREATION_ERROR, for the three classes and both precisions.
The messages that need a device (the state machine after a forward()) are in test_boundary_state_gpu.py."""
import ctypes as C

import numpy as np
import pytest

from pdwt_amd import _native as N

# prefix -> (class name, info struct, number of sizes)
CLASSES = {"pdwt_bw_": ("BoundaryWavelets", N.InfoBW, 2), "pdwt_bw1_": ("BoundaryWavelets1D", N.InfoBW, 2),
           "pdwt_bw3_": ("BoundaryWavelets3D", N.InfoBW3, 3)}

# constructor arguments after the data pointer: the sizes (of pdwt_bw_ and pdwt_bw1_, of pdwt_bw3_), then wname, levels, mode, memisonhost
CASES = {
    "zero size": ((0, 8), (0, 8, 8), (b"haar", 1, 2, 1)),
    "NULL name": ((8, 8), (8, 8, 8), (None, 1, 2, 1)),
    "unknown bank": ((8, 8), (8, 8, 8), (b"nosuch", 1, 2, 1)),
    "mode 5": ((8, 8), (8, 8, 8), (b"haar", 1, 5, 1)),
    "mode -1": ((8, 8), (8, 8, 8), (b"haar", 1, -1, 1)),
    "too small": ((6, 6), (6, 6, 6), (b"db4", 1, 2, 1)),
    "levels 0": ((6, 6), (6, 6, 6), (b"db4", 0, 0, 1)),
    "too large": ((65536, 32768), (70000, 8, 8), (b"haar", 1, 2, 1)),  # Nr * Nc = 2^31; Nz > 65535
}

MODES = "(0 zero, 1 constant, 2 symmetric, 3 reflect, 4 periodic)"
# One line per call, "name -> return value" (the name alone for a void function), then what the call printed.  {C}: the class name, where
# the three print the same line; a dict where they do not.
EXPECTED = {
    "zero size": {
        "BoundaryWavelets": "new -> handle\nERROR: BoundaryWavelets(): invalid image size or wavelet name\ninfo -> 0 8 1 0 2\n",
        "BoundaryWavelets1D": "new -> handle\nERROR: BoundaryWavelets1D(): invalid batch size or wavelet name\ninfo -> 0 8 1 0 2\n",
        "BoundaryWavelets3D": "new -> handle\nERROR: BoundaryWavelets3D(): invalid volume size or wavelet name\ninfo -> 0 8 8 1 0 2\n",
    },
    "NULL name": {
        "BoundaryWavelets": "new -> handle\nERROR: BoundaryWavelets(): invalid image size or wavelet name\ninfo -> 8 8 1 0 2\n",
        "BoundaryWavelets1D": "new -> handle\nERROR: BoundaryWavelets1D(): invalid batch size or wavelet name\ninfo -> 8 8 1 0 2\n",
        "BoundaryWavelets3D": "new -> handle\nERROR: BoundaryWavelets3D(): invalid volume size or wavelet name\ninfo -> 8 8 8 1 0 2\n",
    },
    "unknown bank": "new -> handle\nERROR: unknown wavelet name nosuch\ninfo -> {S}1 0 2\n",
    "mode 5": "new -> handle\nERROR: {C}(): unknown boundary mode 5 " + MODES + "\ninfo -> {S}1 0 5\n",
    "mode -1": "new -> handle\nERROR: {C}(): unknown boundary mode -1 " + MODES + "\ninfo -> {S}1 0 -1\n",
    "too small": {
        "BoundaryWavelets": """\
new -> handle
Warning: required level (1) is greater than the maximum possible level for db4 (0) on a 6x6 image.
Forcing nlevels = 0
ERROR: a 6x6 image is too small for one level of db4
info -> 6 6 0 8 2
""",
        "BoundaryWavelets1D": """\
new -> handle
Warning: required level (1) is greater than the maximum possible level for db4 (0) on rows of 6 samples.
Forcing nlevels = 0
ERROR: rows of 6 samples are too short for one level of db4
info -> 6 6 0 8 2
""",
        "BoundaryWavelets3D": """\
new -> handle
Warning: required level (1) is greater than the maximum possible level for db4 (0) on a 6x6x6 volume.
Forcing nlevels = 0
ERROR: a 6x6x6 volume is too small for one level of db4
info -> 6 6 6 0 8 2
""",
    },
    "levels 0": {
        "BoundaryWavelets": """\
new -> handle
Warning: cannot initialize wavelet coefficients with nlevels < 1. Forcing nlevels = 1
Warning: required level (1) is greater than the maximum possible level for db4 (0) on a 6x6 image.
Forcing nlevels = 0
ERROR: a 6x6 image is too small for one level of db4
info -> 6 6 0 8 0
""",
        "BoundaryWavelets1D": """\
new -> handle
Warning: cannot initialize wavelet coefficients with nlevels < 1. Forcing nlevels = 1
Warning: required level (1) is greater than the maximum possible level for db4 (0) on rows of 6 samples.
Forcing nlevels = 0
ERROR: rows of 6 samples are too short for one level of db4
info -> 6 6 0 8 0
""",
        "BoundaryWavelets3D": """\
new -> handle
Warning: cannot initialize wavelet coefficients with nlevels < 1. Forcing nlevels = 1
Warning: required level (1) is greater than the maximum possible level for db4 (0) on a 6x6x6 volume.
Forcing nlevels = 0
ERROR: a 6x6x6 volume is too small for one level of db4
info -> 6 6 6 0 8 0
""",
    },
    "too large": {
        "BoundaryWavelets": "new -> handle\nERROR: BoundaryWavelets(): invalid image size or wavelet name\ninfo -> 65536 32768 1 0 2\n",
        "BoundaryWavelets1D": "new -> handle\nERROR: BoundaryWavelets1D(): invalid batch size or wavelet name\ninfo -> 65536 32768 1 0 2\n",
        "BoundaryWavelets3D": "new -> handle\nERROR: BoundaryWavelets3D(): unsupported volume size (Nz <= 65535 and Nr * Nc < 2^31 are required)\n"
                              "info -> 70000 8 8 1 0 2\n",
    },
}
# the same after every failed construction (state 4 = W_CREATION_ERROR); {F}: "fused -> 0\n" for the class that has it
EXPECTED_METHODS = """\
state -> 4
num_bands -> 0
coeff_shape -> 0 {U}
{F}forward
Warning: forward transform not computed, as there was an error when creating the wavelets
inverse
Warning: inverse transform not computed, as there was an error in a previous stage
soft_threshold
hard_threshold
norm1 -> -1.0
band_stats -> -1
all_band_stats -> -1
estimate_sigma -> -1.0
threshold_bands
denoise -> -1.0
get_image -> 0
get_coeff -> 0
set_image
set_coeff
image_int_ptr -> 0
coeff_int_ptr -> 0
state -> 4
delete
"""

VOID = ("delete", "forward", "inverse", "soft_threshold", "hard_threshold", "set_image", "set_coeff", "threshold_bands")  # no return value


def transcript(pfx, dtype, args, capfd):
    L = N.host(dtype)
    libc = C.CDLL(None)
    ct = C.c_float if np.dtype(dtype) == np.float32 else C.c_double
    _, info_t, nsz = CLASSES[pfx]
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
    fields = (("Nz",) if nsz == 3 else ()) + ("Nr", "Nc", "nlevels", "hlen", "mode")
    call("info", h, C.byref(info), show=lambda r: " ".join(str(getattr(info, f)) for f in fields))
    sz = [C.c_int(-7) for _ in range(nsz)]
    buf = np.zeros(64, dtype=dtype)
    p = buf.ctypes.data_as(C.c_void_p)
    stats = (N.BandStats * 97)()
    call("state", h)
    call("num_bands", h)
    call("coeff_shape", h, 0, *[C.byref(s) for s in sz], show=lambda n: "%d (%s)" % (n, ", ".join(str(s.value) for s in sz)))
    if pfx == "pdwt_bw1_":
        call("fused", h)
    call("forward", h)
    call("inverse", h)
    call("soft_threshold", h, ct(1.0), 1)
    call("hard_threshold", h, ct(1.0), 0)
    call("norm1", h)
    call("band_stats", h, 0, stats, 1)
    call("all_band_stats", h, stats, 0)
    call("estimate_sigma", h)
    call("threshold_bands", h, p, 0)
    call("denoise", h, 1, C.c_double(-1.0), 0, p)
    call("get_image", h, p)
    call("get_coeff", h, p, 0)
    call("set_image", h, p, 0)
    call("set_coeff", h, p, 0, 0)
    call("image_int_ptr", h)
    call("coeff_int_ptr", h, 0)
    call("state", h)
    call("delete", h)
    return "\n".join(lines) + "\n"


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("pfx", list(CLASSES))
def test_failed_construction_transcript(pfx, case, dtype, capfd):
    cls, _, nsz = CLASSES[pfx]
    sizes2, sizes3, rest = CASES[case]
    sizes = sizes3 if nsz == 3 else sizes2
    got = transcript(pfx, dtype, sizes + rest, capfd)
    head = EXPECTED[case]
    head = head[cls] if isinstance(head, dict) else head
    want = (head + EXPECTED_METHODS).format(C=cls, S="".join("%d " % s for s in sizes), U="(%s)" % ", ".join(["-7"] * nsz),
                                            F="fused -> 0\n" if pfx == "pdwt_bw1_" else "")
    assert got == want


def test_static_handle_functions():
    """The two handle functions that take no instance: the level clamp with the band sizes per level, and the mode numbers (one table
    for the three prefixes).  BoundaryWavelets1D::geometry sees one row, so it has no limit on Nr * Nc to check."""
    L = N.host(np.float32)
    n = [(C.c_int * 8)(*[-7] * 8) for _ in range(3)]
    assert L.pdwt_bw_geometry(24, 26, 4, 3, n[0], n[1]) == 3 and (list(n[0][:5]), list(n[1][:5])) == ([24, 13, 8, 5, -7], [26, 14, 8, 5, -7])
    assert L.pdwt_bw_geometry(24, 26, 4, 9, None, None) == 3 and L.pdwt_bw_geometry(24, 26, 4, 0, None, None) == 1
    assert L.pdwt_bw_geometry(6, 6, 8, 1, None, None) == 0 and L.pdwt_bw_geometry(65536, 32768, 2, 1, None, None) == 0
    assert L.pdwt_bw_geometry(24, 26, 3, 1, None, None) == 0 and L.pdwt_bw_geometry(24, 26, 42, 1, None, None) == 0
    assert L.pdwt_bw1_geometry(48, 4, 3, n[0]) == 3 and list(n[0][:5]) == [48, 25, 14, 8, -7]
    assert L.pdwt_bw1_geometry(6, 8, 1, None) == 0 and L.pdwt_bw1_geometry(0, 2, 1, None) == 0 and L.pdwt_bw1_geometry(1 << 30, 2, 40, None) == 30
    n = [(C.c_int * 8)(*[-7] * 8) for _ in range(3)]
    assert L.pdwt_bw3_geometry(8, 9, 10, 2, 2, n[0], n[1], n[2]) == 2
    assert [list(v[:4]) for v in n] == [[8, 4, 2, -7], [9, 5, 3, -7], [10, 5, 3, -7]]
    assert L.pdwt_bw3_geometry(70000, 8, 8, 2, 1, None, None, None) == 0 and L.pdwt_bw3_geometry(6, 6, 6, 8, 1, None, None, None) == 0
    assert L.pdwt_bw3_geometry(1 << 14, 1 << 14, 1 << 14, 2, 40, None, None, None) == 13  # BW3_MAX_LEVELS
    for pfx in CLASSES:
        fn = getattr(L, pfx + "mode_index")
        assert [fn(m) for m in (b"zero", b"constant", b"symmetric", b"reflect", b"periodic", b"periodization", b"", None)] == [0, 1, 2, 3, 4, -1, -1, -1]
