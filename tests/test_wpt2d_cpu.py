"""CPU-only: the wavelet packet layer loads and its device-free logic is right -- the handle symbols of both host libraries, the
path <-> index arithmetic (C and Python agree), node geometry, level clamping, the basis validator, and the argument checks of the
C-ABI level entries (refused before anything is launched, so they need no device)."""
import ctypes as C

import numpy as np
import pytest

import pdwt_amd
from pdwt_amd import _native as nat
from pdwt_amd import wpt
from tests import refwpt as R

HANDLE = ["new", "delete", "forward", "inverse", "get_image", "set_image", "state", "info", "node_shape", "path_index", "geometry", "get_node", "get_level",
          "set_node", "node_int_ptr", "node_costs", "best_basis", "set_basis", "basis_size", "get_basis", "soft_threshold", "hard_threshold",
          "norm1", "node_stats", "estimate_sigma"]


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_handle_symbols_load(dt):
    L = nat.host(dt)
    missing = [n for n in HANDLE if not hasattr(L, "pdwt_wpt_" + n)]
    assert not missing, missing
    assert pdwt_amd.WaveletPackets2D is wpt.WaveletPackets2D


def test_level_symbols_are_listed():
    for n in ("wpt2d_forward_level", "wpt2d_inverse_level", "wpt2d_node_cost"):
        assert n in nat.TYPED_SYMBOLS
        for s in ("f32", "f64"):
            assert hasattr(pdwt_amd.hip(), "pdwt_%s_%s" % (n, s))


def test_paths():
    L = nat.host(np.float32)
    for path, want in (("", (0, 0)), ("a", (1, 0)), ("d", (1, 3)), ("ahd", (3, 7)), ("va", (2, 8)), ("ddddddd", (7, 4 ** 7 - 1))):
        d = C.c_int(-1)
        assert (L.pdwt_wpt_path_index(path.encode(), C.byref(d)), d.value)[::-1] == want
        assert wpt.path_to_index(path) == want == R.index_of(path)
        assert R.path_of(*want) == path
    assert L.pdwt_wpt_path_index(b"ax", None) == -1
    assert L.pdwt_wpt_path_index(b"aaaaaaaa", None) == -1  # deeper than 7
    with pytest.raises(ValueError):
        wpt.path_to_index("ab")


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_geometry_and_clamping(dt):
    """pdwt_wpt_geometry is what the constructor of WaveletPackets calls: the clamp and the node shapes, without a device"""
    L = nat.host(dt)

    def geom(shape, hlen, asked):
        nr, nc = (C.c_int * 8)(), (C.c_int * 8)()
        n = L.pdwt_wpt_geometry(shape[0], shape[1], hlen, asked, nr, nc)
        return n, [(nr[k], nc[k]) for k in range(n + 1)] if n else []

    assert geom((33, 47), 2, 3) == (3, [(33, 47), (17, 24), (9, 12), (5, 6)])
    assert geom((128, 128), 2, 7)[1][-1] == (1, 1)
    assert geom((96, 80), 8, 9)[0] == 3 and geom((256, 256), 2, 9)[0] == 7 and geom((6, 64), 8, 2) == (0, [])
    assert geom((64, 64), 4, 0)[0] == 1 and geom((64, 64), 4, -3)[0] == 1  # fewer than one level asked for: one
    assert geom((0, 64), 4, 1)[0] == 0 and geom((65536, 32768), 4, 1)[0] == 0  # bad sizes
    assert L.pdwt_wpt_geometry(96, 80, 8, 9, None, None) == 3
    for shape, wname, asked in (((96, 80), "db4", 9), ((256, 256), "haar", 9), ((128, 128), "haar", 7), ((6, 64), "db4", 2), ((64, 64), "db2", 0),
                                ((130, 70), "db8", 3), ((40, 72), "coif1", 2), ((61, 67), "db2", 3), ((2048, 2048), "db20", 9)):
        n, shapes = geom(shape, R.hlen_of(wname), asked)
        assert n == R.clamp_levels(shape, wname, asked), (shape, wname)
        want = [shape]
        for _ in range(n):
            want.append(((want[-1][0] + 1) // 2, (want[-1][1] + 1) // 2))
        assert shapes == (want if n else []), (shape, wname)


def test_basis_validator():
    assert wpt.check_basis(["a", "h", (1, 2), "dd", "da", "dh", "dv"], 2) == [(1, 0), (1, 1), (1, 2), (2, 12), (2, 13), (2, 14), (2, 15)]
    assert wpt.check_basis([""], 3) == [(0, 0)]
    for bad in (["a", "h", "v"], ["a", "h", "v", "d", "ah"], ["a", "a", "h", "v", "d"], ["aaa"], [(1, 4)], [(0, 0), "a"]):
        with pytest.raises(ValueError):
            wpt.check_basis(bad, 2)
        with pytest.raises(ValueError):
            R.check_basis([wpt.path_to_index(n) if isinstance(n, str) else n for n in bad], 2)


@pytest.mark.parametrize("sfx,FT", [("f32", nat.Filters32), ("f64", nat.Filters64)])
def test_level_entries_refuse_bad_arguments(sfx, FT):
    """PDWT_EINVAL before anything is launched: the pointers are never dereferenced (they are not device memory)."""
    L = pdwt_amd.hip()
    f = FT()
    assert getattr(L, "pdwt_compute_filters_separable_" + sfx)(b"db4", 0, C.byref(f)) == 8
    f.hlen = 8
    fake = C.c_void_p(4096)
    for name in ("pdwt_wpt2d_forward_level_", "pdwt_wpt2d_inverse_level_"):
        fn = getattr(L, name + sfx)
        assert fn(None, fake, 64, 64, None, 1, C.byref(f)) == -1
        assert fn(fake, None, 64, 64, None, 1, C.byref(f)) == -1
        assert fn(fake, fake, 64, 64, None, 1, None) == -1
        assert fn(fake, fake, 0, 64, None, 1, C.byref(f)) == -1
        assert fn(fake, fake, 64, 64, None, 0, C.byref(f)) == -1
        assert fn(fake, fake, 64, 64, None, 16385, C.byref(f)) == -1
        assert fn(fake, fake, 7, 64, None, 1, C.byref(f)) == -1        # a node smaller than the bank
        assert fn(fake, fake, 65536, 32768, None, 1, C.byref(f)) == -1  # 2^31 elements
        assert fn(fake, fake, 4000000, 8, None, 1, C.byref(f)) == -1    # more than 65535 rows of tiles
        g2 = FT()
        g2.hlen = 2
        assert fn(fake, fake, 600000, 8, None, 1, C.byref(g2)) == -1    # the same for the Haar kernels
        g = FT()
        for bad in (0, 3, 42):
            g.hlen = bad
            assert fn(fake, fake, 64, 64, None, 1, C.byref(g)) == -1
    out = (C.c_double * 4)()
    cost = getattr(L, "pdwt_wpt2d_node_cost_" + sfx)
    assert cost(None, 16, 4, 0, out) == -1 and cost(fake, 0, 4, 0, out) == -1 and cost(fake, 16, 0, 0, out) == -1
    assert cost(fake, 16, 4, 2, out) == -1 and cost(fake, 16, 4, 0, None) == -1
