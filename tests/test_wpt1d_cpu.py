"""CPU-only: the 1-D wavelet packet layer loads and its device-free logic is right -- the exported symbols of the three libraries, the
geometry and its clamps against tests/refwpt1d.py, the budget rule of the fused path, frequency order and path arithmetic (C and Python
agree), the node-state table of the inverse, the unchanged 2-D behaviour of the shared helpers, the argument checks of the C-ABI entries
(refused before anything is launched, so they need no device), and the refusal to construct without a GPU."""
import ctypes as C

import numpy as np
import pytest

import pdwt_amd
from pdwt_amd import _native as nat
from pdwt_amd import wpt
from tests import refwpt as R2
from tests import refwpt1d as R

HANDLE = ["new", "delete", "forward", "inverse", "fused", "get_image", "set_image", "state", "info", "node_shape", "path_index", "geometry", "frequency_order",
          "get_node", "get_level", "set_node", "node_int_ptr", "node_costs", "best_basis", "set_basis", "basis_size", "get_basis", "soft_threshold",
          "hard_threshold", "norm1", "node_stats", "estimate_sigma"]
PLAIN = ["pdwt_wp1_geometry", "pdwt_wp1_fused", "pdwt_wp1_tmp_elems", "pdwt_wp1_frequency_order", "pdwt_wp1_state_table", "pdwt_memcpy2d"]
TYPED = ["wp1_forward_level", "wp1_inverse_level", "wp1_forward", "wp1_inverse", "wp1_moments", "wp1_thresh"]
# (Nr, Nc, bank, asked) of tests/test_wpt1d_gpu.py with the clamped depth and the node lengths
CASES = [(3, 64, "db2", 4, [64, 32, 16, 8, 4]), (5, 77, "haar", 9, [77, 39, 20, 10, 5, 3, 2]), (300, 33, "db2", 3, [33, 17, 9, 5]),
         (2, 1000, "sym8", 9, [1000, 500, 250, 125, 63, 32, 16]), (7, 96, "db4", 3, [96, 48, 24, 12]), (4, 200, "bior2.2", 9, [200, 100, 50, 25, 13, 7]),
         (2, 640, "db20", 9, [640, 320, 160, 80, 40]), (2, 1031, "db3", 9, [1031, 516, 258, 129, 65, 33, 17, 9]), (6, 48, "coif1", 9, [48, 24, 12, 6]),
         (64, 4096, "haar", 12, [4096 >> k for k in range(13)])]


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_handle_symbols_load(dt):
    L = nat.host(dt)
    missing = [n for n in HANDLE if not hasattr(L, "pdwt_wp1h_" + n)]
    assert not missing, missing
    assert pdwt_amd.WaveletPackets1D is wpt.WaveletPackets1D and "WaveletPackets1D" in pdwt_amd.__all__


def test_c_abi_symbols_are_listed_and_exported():
    L = pdwt_amd.hip()
    for n in PLAIN:
        assert n in nat.PLAIN_SYMBOLS and hasattr(L, n), n
    for n in TYPED:
        assert n in nat.TYPED_SYMBOLS
        for s in ("f32", "f64"):
            assert hasattr(L, "pdwt_%s_%s" % (n, s))


def _geom(nc, hlen, asked):
    n = (C.c_int * 13)()
    L = pdwt_amd.hip().pdwt_wp1_geometry(nc, hlen, asked, n)
    return L, [n[k] for k in range(L + 1)] if L else []


def test_geometry_against_the_reference():
    for _, nc, wname, asked, want in CASES:
        L, n = _geom(nc, R.hlen_of(wname), asked)
        assert L == R.clamp_levels(nc, wname, asked) == len(want) - 1, (nc, wname)
        assert n == want == R.lengths(nc, L), (nc, wname)
    for dt in (np.float32, np.float64):  # the class's static entry is the same function
        n = (C.c_int * 13)()
        assert nat.host(dt).pdwt_wp1h_geometry(1031, 6, 9, n) == 7 and list(n[:8]) == CASES[7][4]


def test_clamps_and_the_zero_level_refusal():
    assert _geom(64, 4, 0)[0] == 1 and _geom(64, 4, -3)[0] == 1      # fewer than one level asked for: one
    assert _geom(96, 8, 9)[0] == 3                                   # ilog2(96 / 7)
    assert _geom(2 ** 14, 2, 20)[0] == 12 and _geom(2 ** 20, 2, 13)[0] == 12  # the cap of 12
    assert _geom(6, 8, 2) == (0, []) and _geom(13, 8, 1) == (0, [])  # too short: ilog2(13 / 7) = 0
    assert _geom(14, 8, 5)[0] == 1
    assert _geom(0, 4, 1)[0] == 0 and _geom(-5, 4, 1)[0] == 0 and _geom(2 ** 30 + 1, 4, 1)[0] == 0
    for bad in (0, 1, 3, 42):
        assert _geom(1024, bad, 2)[0] == 0
    assert pdwt_amd.hip().pdwt_wp1_geometry(96, 8, 9, None) == 3
    # the rows do not count
    n = (C.c_int * 13)()
    assert nat.host(np.float32).pdwt_wp1h_geometry(4096, 2, 12, n) == 12 and n[12] == 1


@pytest.mark.parametrize("elem", [4, 8])
def test_fused_budget_rule(elem):
    L = pdwt_amd.hip()
    for hlen in range(2, 41, 2):
        assert L.pdwt_wp1_fused(4096, hlen, 12, elem) == 1, hlen
        assert L.pdwt_wp1_fused(2 ** 20, hlen, 3, elem) == 0, hlen
        last = 1
        for nc in list(range(2 * (hlen - 1), 600, 37)) + list(range(600, 60000, 997)):  # monotone in Nc: once it stops fitting it never fits again
            fu = L.pdwt_wp1_fused(nc, hlen, 3, elem)
            assert fu in (0, 1) and fu <= last, (hlen, nc)
            last = fu
        assert last == 0
    # roughly 20 000 float32 / 10 000 float64 samples
    lo, hi = 1000, 2 ** 20
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if L.pdwt_wp1_fused(mid, 8, 3, elem) == 1 else (lo, mid)
    assert (19000 if elem == 4 else 9500) <= lo <= (20480 if elem == 4 else 10240), lo
    assert L.pdwt_wp1_fused(13, 8, 1, elem) == -1 and L.pdwt_wp1_fused(4096, 8, 3, 2) == -1 and L.pdwt_wp1_fused(4096, 7, 3, elem) == -1
    assert L.pdwt_wp1_tmp_elems(8, 4096, 8, 3, elem) == 0 and L.pdwt_wp1_tmp_elems(8, 2 ** 20, 8, 3, elem) == 0
    assert L.pdwt_wp1_tmp_elems(0, 4096, 8, 3, elem) == -1 and L.pdwt_wp1_tmp_elems(65536, 32768, 8, 3, elem) == -1


def test_frequency_order_and_paths_agree():
    L, H = pdwt_amd.hip(), nat.host(np.float32)
    for d in range(0, 13):
        out = (C.c_int * 2 ** d)()
        assert L.pdwt_wp1_frequency_order(d, out) == 0
        assert list(out) == list(wpt.frequency_order(d)) == list(R.frequency_order(d))
        assert H.pdwt_wp1h_frequency_order(d, out) == 2 ** d
    assert L.pdwt_wp1_frequency_order(13, (C.c_int * 1)()) == -1 and L.pdwt_wp1_frequency_order(-1, (C.c_int * 1)()) == -1
    assert L.pdwt_wp1_frequency_order(2, None) == -1
    with pytest.raises(ValueError):
        wpt.frequency_order(13)
    assert [R.path_of(2, i) for i in wpt.frequency_order(2)] == ["aa", "ad", "dd", "da"]
    for path, want in (("", (0, 0)), ("a", (1, 0)), ("d", (1, 1)), ("ad", (2, 1)), ("dda", (3, 6)), ("d" * 12, (12, 4095))):
        d = C.c_int(-1)
        assert (H.pdwt_wp1h_path_index(path.encode(), C.byref(d)), d.value)[::-1] == want
        assert wpt.path_to_index(path, 2) == want == R.index_of(path)
        assert R.path_of(*want) == path
    assert H.pdwt_wp1h_path_index(b"ah", None) == -1 and H.pdwt_wp1h_path_index(b"a" * 13, None) == -1
    with pytest.raises(ValueError):
        wpt.path_to_index("ah", 2)


def test_two_d_helpers_are_unchanged():
    for path in ("", "a", "d", "ahd", "va", "ddddddd"):
        assert wpt.path_to_index(path) == wpt.path_to_index(path, 4) == R2.index_of(path)
    with pytest.raises(ValueError, match=r"\(a, h, v, d\)"):
        wpt.path_to_index("ab")
    assert wpt.check_basis(["a", "h", (1, 2), "dd", "da", "dh", "dv"], 2) == [(1, 0), (1, 1), (1, 2), (2, 12), (2, 13), (2, 14), (2, 15)]
    for bad in (["a", "h", "v"], ["a", "h", "v", "d", "ah"], ["aaa"], [(1, 4)]):
        with pytest.raises(ValueError):
            wpt.check_basis(bad, 2)
    assert wpt.MAX_LEVELS == 7 and wpt.MAX_LEVELS_1D == 12


def test_basis_validator_and_state_table():
    assert wpt.check_basis(["a", "dd", (2, 2)], 2, 2) == [(1, 0), (2, 2), (2, 3)]
    assert wpt.check_basis([""], 3, 2) == [(0, 0)]
    L = pdwt_amd.hip()

    def table(levels, nodes):
        d, i = (C.c_int * len(nodes))(*[v[0] for v in nodes]), (C.c_int * len(nodes))(*[v[1] for v in nodes])
        out = (C.c_ubyte * 2 ** (levels + 1))(*([9] * 2 ** (levels + 1)))
        return L.pdwt_wp1_state_table(levels, d, i, len(nodes), out), list(out)

    for bad in ([(1, 0)], [(1, 0), (1, 1), (2, 3)], [(1, 0), (1, 0), (1, 1)], [(3, 0)], [(1, 2)], [(0, 0), (1, 0)]):
        with pytest.raises(ValueError):
            wpt.check_basis(bad, 2, 2)
        with pytest.raises(ValueError):
            R.check_basis(bad, 2)
        assert table(2, bad)[0] == -1
    # 1 = a node of the basis, 2 = above it, 0 = below it; node i of depth l at 2^l - 1 + i
    assert table(2, [(1, 0), (2, 2), (2, 3)]) == (0, [2, 1, 2, 0, 0, 1, 1, 0])
    assert table(2, [(0, 0)]) == (0, [1, 0, 0, 0, 0, 0, 0, 0])
    assert table(2, [(2, k) for k in range(4)]) == (0, [2, 2, 2, 1, 1, 1, 1, 0])
    assert table(0, [(0, 0)])[0] == -1 and table(13, [(0, 0)])[0] == -1


@pytest.mark.parametrize("sfx,FT", [("f32", nat.Filters32), ("f64", nat.Filters64)])
def test_entries_refuse_bad_arguments(sfx, FT):
    """PDWT_EINVAL before anything is launched: the pointers are never dereferenced (they are not device memory)."""
    L = pdwt_amd.hip()
    f = FT()
    assert getattr(L, "pdwt_compute_filters_separable_" + sfx)(b"db4", 0, C.byref(f)) == 8
    f.hlen = 8
    g = FT()
    fake = C.c_void_p(4096)
    fwd, inv = getattr(L, "pdwt_wp1_forward_level_" + sfx), getattr(L, "pdwt_wp1_inverse_level_" + sfx)
    for fn, extra in ((fwd, ()), (inv, (None, 0))):
        assert fn(None, fake, 4, 2, 64, *extra, C.byref(f)) == -1
        assert fn(fake, None, 4, 2, 64, *extra, C.byref(f)) == -1
        assert fn(fake, fake, 4, 2, 64, *extra, None) == -1
        assert fn(fake, fake, 0, 2, 64, *extra, C.byref(f)) == -1
        assert fn(fake, fake, 4, 0, 64, *extra, C.byref(f)) == -1
        assert fn(fake, fake, 4, 4097, 64, *extra, C.byref(f)) == -1
        assert fn(fake, fake, 4, 2, 0, *extra, C.byref(f)) == -1
        assert fn(fake, fake, 65536, 2, 32768, *extra, C.byref(f)) == -1  # 2^32 elements
        for bad in (0, 3, 42):
            g.hlen = bad
            assert fn(fake, fake, 4, 2, 64, *extra, C.byref(g)) == -1
    assert inv(fake, fake, 4, 2, 64, fake, 0, C.byref(f)) == -1 and inv(fake, fake, 4, 2, 64, fake, 3, C.byref(f)) == -1  # a bad list length
    tab = (C.c_void_p * 3)(4096, 4096, 4096)
    hole = (C.c_void_p * 3)(4096, None, 4096)
    whole_f, whole_i = getattr(L, "pdwt_wp1_forward_" + sfx), getattr(L, "pdwt_wp1_inverse_" + sfx)
    for fn, extra in ((whole_f, ()), (whole_i, (fake,))):
        assert fn(None, tab, 4, 96, 3, *extra, C.byref(f)) == -1
        assert fn(fake, None, 4, 96, 3, *extra, C.byref(f)) == -1
        assert fn(fake, hole, 4, 96, 3, *extra, C.byref(f)) == -1
        assert fn(fake, tab, 4, 96, 3, *extra, None) == -1
        assert fn(fake, tab, 0, 96, 3, *extra, C.byref(f)) == -1
        assert fn(fake, tab, 4, 96, 4, *extra, C.byref(f)) == -1   # deeper than the clamp: ilog2(96 / 7) = 3
        assert fn(fake, tab, 4, 96, 0, *extra, C.byref(f)) == -1
        assert fn(fake, tab, 4, 6, 1, *extra, C.byref(f)) == -1    # too short for one level
        assert fn(fake, tab, 65536, 32768, 3, *extra, C.byref(f)) == -1
    assert whole_i(fake, tab, 4, 96, 3, None, C.byref(f)) == -1    # no state table
    out = (C.c_double * 16)()
    mom = getattr(L, "pdwt_wp1_moments_" + sfx)
    assert mom(None, 4, 16, out) == -1 and mom(fake, 0, 16, out) == -1 and mom(fake, 4, 0, out) == -1 and mom(fake, 4, 16, None) == -1
    assert mom(fake, 2 ** 31, 2, out) == -1
    thr = getattr(L, "pdwt_wp1_thresh_" + sfx)
    assert thr(0, None, 4, 2, 16, fake, 1.0) == -1 and thr(0, fake, 4, 2, 16, None, 1.0) == -1 and thr(2, fake, 4, 2, 16, fake, 1.0) == -1
    assert thr(0, fake, 0, 2, 16, fake, 1.0) == -1 and thr(0, fake, 4, 0, 16, fake, 1.0) == -1 and thr(0, fake, 4, 2, 0, fake, 1.0) == -1
    assert L.pdwt_memcpy2d(None, 8, fake, 8, 8, 2, 2) == -1 and L.pdwt_memcpy2d(fake, 4, fake, 8, 8, 2, 2) == -1 and L.pdwt_memcpy2d(fake, 8, fake, 8, 8, 2, 4) == -1
    assert L.pdwt_memcpy2d(fake, 8, fake, 8, 0, 2, 2) == 0  # nothing to copy


def test_class_refuses_to_construct_without_a_gpu():
    if pdwt_amd.hip().pdwt_device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(RuntimeError, match="no HIP device"):
        pdwt_amd.WaveletPackets1D(np.zeros((4, 64), np.float32), "db2", 2)
