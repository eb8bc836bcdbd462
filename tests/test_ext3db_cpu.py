"""The batched 3-D boundary-mode drivers (include/pdwt_hip.h "Batched 3-D DWT with boundary modes") without a device: the symbols, the scratch
formulas of the header and the refusals, which come before anything is launched or touched (the pointers here are fakes)."""
import ctypes as C

import pytest

import pdwt_amd
from pdwt_amd import _native as nat
from tests import refext3d as R3

PLAIN = ("pdwt_ext3db_tmp_elems", "pdwt_ext3db_adjoint_tmp_elems")
TYPED = ("ext3db_forward", "ext3db_inverse", "ext3db_forward_adjoint", "ext3db_inverse_adjoint")


def bank(sfx, wname):
    L = pdwt_amd.hip()
    f = (nat.Filters32 if sfx == "f32" else nat.Filters64)()
    f.hlen = getattr(L, "pdwt_compute_filters_separable_" + sfx)(wname.encode(), 0, C.byref(f))
    assert f.hlen >= 2
    return f


def test_the_ten_symbols_exist_and_are_listed():
    L = pdwt_amd.hip()
    for name in PLAIN:
        assert name in nat.PLAIN_SYMBOLS and hasattr(L, name), name
    for t in TYPED:
        assert t in nat.TYPED_SYMBOLS, t
        for sfx in ("f32", "f64"):
            assert hasattr(L, "pdwt_%s_%s" % (t, sfx)), (t, sfx)
    assert len(PLAIN) + 2 * len(TYPED) == 10


def header_tmp_elems(V, shape, hlen, levels):
    """the formulas of the header, from the level shapes of the reference"""
    s = R3.level_shapes(shape, hlen, levels)
    quads = 4 * V * s[0][0] * s[1][1] * s[1][2]
    approx = 2 * V * s[1][0] * s[1][1] * s[1][2] if levels > 1 else 0
    frames = max(V * s[l][0] * ((2 * s[l + 1][1] + hlen - 2) * (2 * s[l + 1][2] + hlen - 2) - s[l][1] * s[l][2]) for l in range(levels))
    return quads + approx, quads + approx + frames


@pytest.mark.parametrize("V,shape,wname,levels", [(3, (16, 16, 16), "db2", 2), (1, (7, 7, 7), "db4", 1), (5, (9, 33, 47), "haar", 3)])
def test_tmp_elems_are_the_formulas_of_the_header(V, shape, wname, levels):
    L = pdwt_amd.hip()
    hlen = R3.bank(wname)[0]
    plain, adjoint = header_tmp_elems(V, shape, hlen, levels)
    assert L.pdwt_ext3db_tmp_elems(V, shape[0], shape[1], shape[2], hlen, levels) == plain
    assert L.pdwt_ext3db_adjoint_tmp_elems(V, shape[0], shape[1], shape[2], hlen, levels) == adjoint
    assert 0 < plain < adjoint  # (every case has frames: an odd axis or more than two taps)


def test_tmp_elems_refuse_what_the_drivers_refuse():
    L = pdwt_amd.hip()
    for fn in (L.pdwt_ext3db_tmp_elems, L.pdwt_ext3db_adjoint_tmp_elems):
        assert fn(3, 16, 16, 16, 4, 2) > 0
        bad = [fn(0, 16, 16, 16, 4, 2), fn(-1, 16, 16, 16, 4, 2), fn(3, 16, 16, 16, 4, 0), fn(3, 16, 16, 16, 4, 14), fn(3, 16, 16, 16, 3, 1), fn(3, 16, 16, 16, 42, 1),
               fn(3, 2, 16, 16, 4, 1), fn(3, 16, 2, 16, 4, 1), fn(3, 16, 16, 2, 4, 1), fn(3, 0, 16, 16, 2, 1), fn(1, 65536, 2, 2, 2, 1), fn(1, 2, 65536, 65536, 2, 1),
               fn(65536, 32768, 2, 2, 2, 1),        # 2^31 planes
               fn(1024, 1024, 1024, 1024, 2, 1)]    # 2^40 elements
        assert bad == [-1] * len(bad), bad
        assert fn(1, 65535, 2, 2, 2, 1) > 0 and fn(65535, 32768, 2, 2, 2, 1) > 0 and fn(1023, 1024, 1024, 1024, 2, 1) > 0
        assert fn(1, 7, 7, 7, 8, 13) > 0  # an axis of hlen - 1 samples keeps its length: 13 levels, not clamped


@pytest.mark.parametrize("sfx", ["f32", "f64"])
def test_every_refusal_is_einval_before_anything_is_touched(sfx):
    L = pdwt_amd.hip()
    f = bank(sfx, "db2")
    fp = C.byref(f)
    V, (Nz, Nr, Nc), levels, m = 3, (16, 16, 16), 2, 2
    fake = lambda k: 0x10000 + 0x1000 * k  # never dereferenced
    x, tmp = fake(0), fake(1)
    tab = (C.c_void_p * (7 * levels + 1))(*[fake(2 + k) for k in range(7 * levels + 1)])
    holes = [(C.c_void_p * (7 * levels + 1))(*[None if k == h else fake(2 + k) for k in range(7 * levels + 1)]) for h in (0, 7, 7 * levels)]
    moded = {"ext3db_forward": True, "ext3db_inverse": False, "ext3db_forward_adjoint": True, "ext3db_inverse_adjoint": False}
    for name, has_mode in moded.items():
        fn = getattr(L, "pdwt_%s_%s" % (name, sfx))

        def call(x=x, tab=tab, V=V, Nz=Nz, Nr=Nr, Nc=Nc, levels=levels, mode=m, fp=fp, tmp=tmp):
            return fn(x, tab, V, Nz, Nr, Nc, levels, mode, fp, tmp) if has_mode else fn(x, tab, V, Nz, Nr, Nc, levels, fp, tmp)

        refused = [call(x=None), call(tab=None), call(fp=None), call(tmp=None)] + [call(tab=h) for h in holes]
        refused += [call(V=0), call(V=-3), call(levels=0), call(levels=14), call(levels=-1)]
        refused += [call(Nz=2), call(Nr=2), call(Nc=2), call(Nz=0), call(Nz=65536), call(Nr=65536, Nc=65536)]
        refused += [call(V=65536, Nz=32768), call(V=1024, Nz=1024, Nr=1024, Nc=1024)]
        if has_mode:
            refused += [call(mode=-1), call(mode=5)]
        assert refused == [-1] * len(refused), (name, refused)


def test_the_cases_of_the_gpu_tests_are_cases_of_the_reference_module():
    from tests import refadj3d as A3
    from tests import test_ext3db_gpu as G
    assert len(G.CASES) == 19
    for s, w, L, m in G.CASES:
        assert any(c[:3] == (s, w, L) and m in c[3] for c in A3.CASES), (s, w, L, m)
