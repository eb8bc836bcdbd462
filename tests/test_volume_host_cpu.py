"""CPU-only transcript of the host side of the two volume classes (include/wt3d.h, include/swt3d.h; pdwt_amd/csrc/wt3d.cpp) through
their flat handle APIs: constructions that fail before any device allocation, then every method on the failed instance.  Pins the
messages the classes print, byte for byte, and what the methods return in state W_CREATION_ERROR, for both classes and both precisions.
The messages that need a device (a failed launch, a threshold after inverse()) are out of reach here."""
import ctypes as C

import numpy as np
import pytest

from pdwt_amd import _native as N

# constructor arguments after the volume pointer: Nz, Nr, Nc, wname, levels, memisonhost
CASES = [("zero size", (0, 8, 8, b"haar", 1, 1)),
         ("NULL name", (8, 8, 8, None, 1, 1)),
         ("unknown bank", (8, 8, 8, b"nosuch", 1, 1)),
         ("too small", (4, 4, 4, b"db4", 1, 1)),
         ("too many planes", (70000, 8, 8, b"haar", 0, 1))]

# {C}: the class name.  One line per call, "name -> return value" (the name alone for a void function), then what the call printed.
EXPECTED = {
    "zero size": """\
new -> handle
ERROR: {C}(): invalid volume size or wavelet name
info -> 0 8 8 1 0
""",
    "NULL name": """\
new -> handle
ERROR: {C}(): invalid volume size or wavelet name
info -> 8 8 8 1 0
""",
    "unknown bank": """\
new -> handle
ERROR: unknown wavelet name nosuch
info -> 8 8 8 1 0
""",
    "too small": """\
new -> handle
Warning: required level (1) is greater than the maximum possible level for db4 (0) on a 4x4x4 volume.
Forcing nlevels = 0
ERROR: a 4x4x4 volume is too small for one level of db4
info -> 4 4 4 0 8
""",
    "too many planes": """\
new -> handle
Warning: cannot initialize wavelet coefficients with nlevels < 1. Forcing nlevels = 1
ERROR: {C}(): unsupported volume size (Nz <= 65535 and Nr * Nc < 2^31 are required)
info -> 70000 8 8 1 2
""",
}
# the same after every failed construction (state 4 = W_CREATION_ERROR)
EXPECTED_METHODS = """\
state -> 4
num_bands -> 0
band_shape -> 0 (-7, -7, -7)
forward
Warning: forward transform not computed, as there was an error when creating the wavelets
inverse
Warning: inverse transform not computed, as there was an error in a previous stage
soft_threshold
hard_threshold
norm1_f64 -> 0.0
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
    info = N.Info3D()
    call("info", h, C.byref(info), show=lambda r: "%d %d %d %d %d" % (info.Nz, info.Nr, info.Nc, info.nlevels, info.hlen))
    z, r, c = C.c_int(-7), C.c_int(-7), C.c_int(-7)
    buf = np.zeros(64, dtype=dtype)
    p = buf.ctypes.data_as(C.c_void_p)
    stats = (N.BandStats * 97)()
    call("state", h)
    call("num_bands", h)
    call("band_shape", h, 0, C.byref(z), C.byref(r), C.byref(c), show=lambda n: "%d (%d, %d, %d)" % (n, z.value, r.value, c.value))
    call("forward", h)
    call("inverse", h)
    call("soft_threshold", h, ct(1.0), 1, 1)
    call("hard_threshold", h, ct(1.0), 0, 0)
    call("norm1_f64", h)
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
@pytest.mark.parametrize("case", [c[0] for c in CASES])
@pytest.mark.parametrize("pfx,cls", [("pdwt_wavelets3d_", "Wavelets3D"), ("pdwt_swt3d_", "StationaryWavelets3D")])
def test_failed_construction_transcript(pfx, cls, case, dtype, capfd):
    got = transcript(pfx, dtype, dict(CASES)[case], capfd)
    assert got == (EXPECTED[case] + EXPECTED_METHODS).format(C=cls)
