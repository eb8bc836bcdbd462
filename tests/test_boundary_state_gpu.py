"""Transcript of the state machine of the three boundary-mode classes (include/wt_ext.h; pdwt_amd/csrc/wt_ext.cpp) through their flat
handle APIs, on a device: what each call prints, byte for byte, what it returns and the state it leaves, from forward() over the
refusals after inverse() back to W_INIT.  These messages carry the class name and need coefficients on a device, so the CPU transcript
(test_boundary_host_cpu.py) cannot reach them.  The inputs are the smallest that walk every branch of the level walks: three levels in
2-D (both intermediate buffers), a fused and a per-level instance in 1-D, two levels in 3-D (the approximation goes through the scratch)."""
import ctypes as C

import numpy as np
import pytest

from pdwt_amd import _native as N

pytestmark = pytest.mark.gpu

# id -> (prefix, class name, dtype, sizes, wname, levels, bands, elements of band 0, fused or None)
CASES = {
    "2d-f32": ("pdwt_bw_", "BoundaryWavelets", np.float32, (24, 26), b"db2", 3, 10, 5 * 5, None),
    "2d-f64": ("pdwt_bw_", "BoundaryWavelets", np.float64, (24, 26), b"db2", 3, 10, 5 * 5, None),
    "1d-fused": ("pdwt_bw1_", "BoundaryWavelets1D", np.float32, (3, 48), b"db2", 3, 4, 3 * 8, 1),
    "1d-levels": ("pdwt_bw1_", "BoundaryWavelets1D", np.float32, (2, 40000), b"haar", 2, 3, 2 * 10000, 0),
    "3d-f32": ("pdwt_bw3_", "BoundaryWavelets3D", np.float32, (8, 9, 10), b"haar", 2, 15, 2 * 3 * 3, None),
}

# One line per call, "name -> return value" (the name alone for a void function), then what the call printed.  {C}: the class name,
# {NB}: its bands, {N0}: the elements of band 0, {F}: "fused -> 0 / 1\n" for the class that has it.  States: 0 W_INIT, 1 W_FORWARD,
# 2 W_INVERSE.
EXPECTED = """\
new -> handle
state -> 0
num_bands -> {NB}
{F}forward
state -> 1
soft_threshold
state -> 1
get_coeff -> {N0}
set_coeff
ERROR: set_coeff(): invalid coefficient index {NB}
state -> 1
inverse
state -> 2
inverse
Warning: W.inverse() has already been run. Inverse is available in W.get_image()
state -> 2
hard_threshold
Warning: {C}(): cannot threshold coefficients after W.inverse() (run forward() first)
state -> 2
get_coeff -> 0
Warning: get_coeff(): inverse() has been performed; run forward() first.
band_stats -> -1
denoise -> -1.0
state -> 2
set_image
state -> 0
delete
"""

VOID = ("delete", "forward", "inverse", "soft_threshold", "hard_threshold", "set_image", "set_coeff")  # no return value


@pytest.mark.parametrize("case", list(CASES))
def test_state_machine_transcript(case, capfd):
    pfx, cls, dtype, sizes, wname, levels, nb, n0, fused = CASES[case]
    N.require_gpu()
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

    x = np.random.RandomState(11).uniform(-1, 1, sizes).astype(dtype)
    buf = np.zeros(x.size, dtype=dtype)  # (no band is larger than the input here)
    px, p = x.ctypes.data_as(C.c_void_p), buf.ctypes.data_as(C.c_void_p)
    stats = (N.BandStats * 97)()
    h = call("new", px, *sizes, wname, levels, 2, 1, show=lambda r: "handle" if r else "NULL")
    assert h
    try:
        call("state", h)
        call("num_bands", h)
        if fused is not None:
            call("fused", h)
        call("forward", h)
        call("state", h)
        call("soft_threshold", h, ct(0.1), 0)
        call("state", h)
        call("get_coeff", h, p, 0)
        call("set_coeff", h, p, nb, 0)
        call("state", h)
        call("inverse", h)
        call("state", h)
        call("inverse", h)
        call("state", h)
        call("hard_threshold", h, ct(0.1), 0)
        call("state", h)
        call("get_coeff", h, p, 0)
        call("band_stats", h, 0, stats, 1)
        call("denoise", h, 1, C.c_double(-1.0), 0, p)
        call("state", h)
        call("set_image", h, px, 0)
        call("state", h)
    finally:
        call("delete", h)
    got = "\n".join(lines) + "\n"
    assert got == EXPECTED.format(C=cls, NB=nb, N0=n0, F="" if fused is None else "fused -> %d\n" % fused)
