"""Transcript of the state machine of the three wavelet packet classes (include/wpt.h, include/wpt1d.h, include/wpt_batch.h;
pdwt_amd/csrc/wpt.cpp) through their flat handle APIs, on a device: what each call prints, byte for byte, what it returns and the state it
leaves, from forward() over a best basis, a basis set by hand, a threshold and the refusals after it, to the refusals after inverse() and
back to W_INIT.  These messages need coefficients on a device, so the CPU transcript (test_packets_host_cpu.py) cannot reach them.  The
inputs are the smallest that walk every branch of the per-class code: a mixed basis whose inverse synthesises a proper subset of depth 1
(the parents lists of the single-image class, the chunk lists of the batch class with allow_fused = 0), a fused and a per-depth instance of
the 1-D and the batch class."""
import ctypes as C

import numpy as np
import pytest

from pdwt_amd import _native as N

pytestmark = pytest.mark.gpu

MIXED_2D = [(1, 0), (1, 1), (1, 2), (2, 12), (2, 13), (2, 14), (2, 15)]
MIXED_1D = [(1, 0), (2, 2), (2, 3)]

# id -> (prefix, class name, dtype, sizes, wname, levels, arguments after memisonhost, arity, mixed basis, elements of node (1, 0), fused or None)
CASES = {
    "2d-f32": ("pdwt_wpt_", "WaveletPackets", np.float32, (24, 26), b"db2", 2, (), 4, MIXED_2D, 12 * 13, None),
    "2d-f64": ("pdwt_wpt_", "WaveletPackets", np.float64, (24, 26), b"db2", 2, (), 4, MIXED_2D, 12 * 13, None),
    "1d-fused": ("pdwt_wp1h_", "WaveletPackets1D", np.float32, (3, 48), b"db2", 3, (), 2, MIXED_1D, 3 * 24, 1),
    "1d-depths": ("pdwt_wp1h_", "WaveletPackets1D", np.float32, (2, 40000), b"haar", 2, (), 2, MIXED_1D, 2 * 20000, 0),
    "batch-fused-f32": ("pdwt_wpbh_", "WaveletPacketsImages", np.float32, (3, 24, 26), b"db2", 2, (1,), 4, MIXED_2D, 3 * 12 * 13, 1),
    "batch-fused-f64": ("pdwt_wpbh_", "WaveletPacketsImages", np.float64, (3, 24, 26), b"db2", 2, (1,), 4, MIXED_2D, 3 * 12 * 13, 1),
    "batch-depths-f32": ("pdwt_wpbh_", "WaveletPacketsImages", np.float32, (3, 24, 26), b"db2", 2, (0,), 4, MIXED_2D, 3 * 12 * 13, 0),
    "batch-depths-f64": ("pdwt_wpbh_", "WaveletPacketsImages", np.float64, (3, 24, 26), b"db2", 2, (0,), 4, MIXED_2D, 3 * 12 * 13, 0),
}

# One line per call, "name -> return value" (the name alone for a void function), then what the call printed.  {C}: the class name,
# {F}: "fused -> 0 / 1\n" for the classes that have it, {BB}: the size of the best basis (checked below), {NN}: the elements of node (1, 0).
# States: 0 W_INIT, 1 W_FORWARD, 2 W_INVERSE, 3 W_THRESHOLD.
EXPECTED = """\
new -> handle
state -> 0
{F}forward
state -> 1
best_basis -> {BB}
basis_size -> {BB}
set_basis -> 0
soft_threshold
state -> 3
set_basis -> -1
best_basis -> -1
get_node -> {NN}
inverse
state -> 2
inverse
Warning: W.inverse() has already been run. Inverse is available in W.get_image()
hard_threshold
Warning: {C}(): cannot threshold coefficients, as they were modified by W.inverse()
get_node -> 0
Warning: get_node(): inverse() has been performed, the coefficients has been modified and do not make sense anymore.
get_level -> 0
Warning: get_level(): inverse() has been performed, the coefficients has been modified and do not make sense anymore.
set_node -> 0
Warning: set_node(): refused, the tree does not hold the coefficients of a forward() (run forward() first)
norm1 -> -1.0
node_stats -> -1
set_image
state -> 0
delete
"""

VOID = ("delete", "forward", "inverse", "soft_threshold", "hard_threshold", "set_image")  # no return value


def caller(L, pfx, capfd, lines):
    libc = C.CDLL(None)

    def call(name, *a, show=None):
        capfd.readouterr()
        ret = getattr(L, pfx + name)(*a)
        libc.fflush(None)
        lines.append(name if name in VOID else "%s -> %s" % (name, show(ret) if show else ret))
        lines.extend(capfd.readouterr().out.splitlines())
        return ret

    return call


def pairs(nodes):
    n = len(nodes)
    return (C.c_int * n)(*[v[0] for v in nodes]), (C.c_int * n)(*[v[1] for v in nodes]), n


@pytest.mark.parametrize("case", list(CASES))
def test_state_machine_transcript(case, capfd):
    pfx, cls, dtype, sizes, wname, levels, extra, arity, mixed, nn, fused = CASES[case]
    N.require_gpu()
    L = N.host(dtype)
    ct = C.c_float if np.dtype(dtype) == np.float32 else C.c_double
    lines = []
    call = caller(L, pfx, capfd, lines)
    x = np.random.RandomState(11).uniform(-1, 1, sizes).astype(dtype)
    buf = np.zeros(2 * x.size, dtype=dtype)  # (no depth is larger than that)
    px, p = x.ctypes.data_as(C.c_void_p), buf.ctypes.data_as(C.c_void_p)
    stats = (N.BandStats * 64)()
    h = call("new", px, *sizes, wname, levels, 1, *extra, show=lambda r: "handle" if r else "NULL")
    assert h
    try:
        call("state", h)
        if fused is not None:
            call("fused", h)
        call("forward", h)
        call("state", h)
        bb = call("best_basis", h, 1)
        call("basis_size", h)
        call("set_basis", h, *pairs(mixed))
        call("soft_threshold", h, ct(0.1), 0)
        call("state", h)
        call("set_basis", h, *pairs(mixed))
        call("best_basis", h, 1)
        call("get_node", h, p, 1, 0)
        call("inverse", h)
        call("state", h)
        call("inverse", h)
        call("hard_threshold", h, ct(0.1), 0)
        call("get_node", h, p, 1, 0)
        call("get_level", h, p, 1)
        call("set_node", h, p, 1, 0, 0)
        call("norm1", h)
        call("node_stats", h, 1, stats)
        call("set_image", h, px, 0)
        call("state", h)
    finally:
        call("delete", h)
    got = "\n".join(lines) + "\n"
    # a basis of a full tree has 1 + k (arity - 1) nodes, at most the arity^levels leaves
    assert 1 <= bb <= arity ** levels and (bb - 1) % (arity - 1) == 0
    assert got == EXPECTED.format(C=cls, F="" if fused is None else "fused -> %d\n" % fused, BB=bb, NN=nn)


@pytest.mark.parametrize("case", ["2d-f32", "1d-fused", "batch-fused-f32"])
def test_root_only_basis_inverts_to_the_input(case, capfd):
    """The basis (0, 0): the input itself is the coefficients.  inverse() has nothing to synthesise, launches nothing and still leaves
    W_INVERSE; the image is the input, bit for bit."""
    pfx, cls, dtype, sizes, wname, levels, extra, arity, mixed, nn, fused = CASES[case]
    N.require_gpu()
    L = N.host(dtype)
    lines = []
    call = caller(L, pfx, capfd, lines)
    x = np.random.RandomState(11).uniform(-1, 1, sizes).astype(dtype)
    out = np.zeros_like(x)
    h = call("new", x.ctypes.data_as(C.c_void_p), *sizes, wname, levels, 1, *extra, show=lambda r: "handle" if r else "NULL")
    assert h
    try:
        call("forward", h)
        call("set_basis", h, *pairs([(0, 0)]))
        call("basis_size", h)
        call("inverse", h)
        call("state", h)
        call("get_image", h, out.ctypes.data_as(C.c_void_p))
    finally:
        call("delete", h)
    assert "\n".join(lines) + "\n" == "new -> handle\nforward\nset_basis -> 0\nbasis_size -> 1\ninverse\nstate -> 2\nget_image -> %d\ndelete\n" % x.size
    assert np.array_equal(out, x)
