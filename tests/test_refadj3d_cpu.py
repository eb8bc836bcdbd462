"""CPU-only: the reference of the 3-D adjoints (tests/refadj3d.py) against dense matrices built from tests/refext3d.py, the float32 error of
the kernels' order on every GPU case of tests/test_adjoint3d_gpu.py, and what the built libraries answer without a device: the new
symbols, the scratch geometry, the interior run of the z pass, the refusals of the level entries on fake pointers and the TypeErrors of
the functional layer.

Bounds of the GPU tests.  The family's: 1e-5 (float32) / 1e-12 (float64) of max|ref|, valid for a case as long as the float32 figure
measured here is at most a quarter of it (2.5e-6).  Measured (pytest -s): the forward adjoints lie between 1.1e-7 and 3.0e-7 (the largest:
the `constant` mode of the 40-tap bank on (40, 48, 40), up to 39 pre-images per axis), the inverse adjoints between 1.9e-7 and 3.7e-7
((40, 48, 40) db20) -- so no case needs a bound of its own."""
import ctypes as C
import inspect

import numpy as np
import pytest

import pdwt_amd
from pdwt_amd import _native as nat
from tests import refadj as A
from tests import refadj3d as A3
from tests import refext3d as R3

FAKE = 0x10000  # a pointer that is never dereferenced: every call below must be refused first


def _flat(bands):
    return np.concatenate([np.ravel(bands[k]) for k in R3.LEVEL_KEYS])


def _split(c, bshape):
    n = int(np.prod(bshape))
    return {k: c[i * n:(i + 1) * n].reshape(bshape) for i, k in enumerate(R3.LEVEL_KEYS)}


@pytest.mark.parametrize("shape,wname", [((2, 3, 3), "haar"), ((3, 4, 5), "db2"), ((5, 5, 6), "bior2.2"), ((7, 7, 8), "db4")])
def test_level_adjoints_are_the_transposes_of_the_dense_matrices(shape, wname):
    F, t = R3.bank(wname)
    bshape = R3.level_shapes(shape, F, 1)[1]
    n, nb = int(np.prod(shape)), 8 * int(np.prod(bshape))
    rs = np.random.RandomState(5)
    worst = 0.0
    for mode in R3.MODES:
        M = A.dense(lambda x: _flat(R3.dwt3(x.reshape(shape), t, mode)), n)
        assert M.shape == (nb, n)
        c = rs.standard_normal(nb)
        got = A3.dwt3_adjoint(_split(c, bshape), shape, t, mode)
        worst = max(worst, float(np.abs(got.ravel() - M.T @ c).max()))
    S = A.dense(lambda c: R3.idwt3(_split(c, bshape), shape, t), nb)
    assert S.shape == (n, nb)
    y = rs.standard_normal(shape)
    worst_s = float(np.abs(_flat(A3.idwt3_adjoint(y, t)) - S.T @ y.ravel()).max())
    print("%s %s: worst |adj - M^T c| = %.2e, |adj - S^T y| = %.2e" % (shape, wname, worst, worst_s))
    assert worst <= 1e-13 and worst_s <= 1e-13


@pytest.mark.parametrize("mode", R3.MODES)
def test_two_level_operator_identity(mode):
    shape = (8, 9, 10)
    rs = np.random.RandomState(7)
    x = rs.standard_normal(shape)
    b = R3.wavedec3(x, "db2", 2, mode)
    c = [rs.standard_normal(v.shape) for v in b]
    lhs = sum(float((u * v).sum()) for u, v in zip(b, c))
    rhs = float((x * A3.wavedec3_adjoint(c, shape, "db2", mode)).sum())
    scale = np.sqrt(sum(float((u * u).sum()) for u in b)) * np.sqrt(sum(float((v * v).sum()) for v in c))
    assert abs(lhs - rhs) <= 1e-12 * scale, (lhs, rhs)
    y = rs.standard_normal(shape)
    Sc = R3.waverec3(c, shape, "db2")
    lhs = float((Sc * y).sum())
    rhs = sum(float((u * v).sum()) for u, v in zip(c, A3.waverec3_adjoint(y, "db2", 2)))
    scale = np.sqrt(float((Sc * Sc).sum())) * np.sqrt(float((y * y).sum()))
    assert abs(lhs - rhs) <= 1e-12 * scale, (lhs, rhs)


def test_float32_error_of_the_kernel_order_on_every_gpu_case():
    """the figure that decides whether the family's bound holds for a case (module docstring)"""
    for shape, w, L, modes in A3.CASES:
        F, _ = R3.bank(w)
        c = A.cotangent(R3.band_shapes(shape, F, L), (), 1)
        for mode in modes:
            e = A.rel_err(A3.wavedec3_adjoint(c, shape, w, mode, np.float32), A3.wavedec3_adjoint(c, shape, w, mode))
            print("3-D %-14s %-8s L%d %-9s float32 order: %.2e" % (shape, w, L, mode, e))
            assert 4 * e <= A3.bound("f32", shape, w, L, mode), (shape, w, mode, e)
        x = A.cotangent([shape], (), 2)[0]
        e = max(A.rel_err(p, q) for p, q in zip(A3.waverec3_adjoint(x, w, L, np.float32), A3.waverec3_adjoint(x, w, L)))
        print("3-D %-14s %-8s L%d inverse adjoint float32 order: %.2e" % (shape, w, L, e))
        assert 4 * e <= A3.F32_BOUND, (shape, w, e)
    assert all(v >= A3.F32_BOUND for v in A3.F32_BOUND_OF.values())  # a bound of its own is never a narrower promise than it needs to be


# ---- the built libraries, no device ----------------------------------------------------------------------------------------------------
NEW_PLAIN = ["pdwt_ext3d_adjoint_level_tmp_elems", "pdwt_ext3d_adjoint_z_run"]
NEW_TYPED = ["ext3d_forward_adjoint_level", "ext3d_inverse_adjoint_level"]


def test_every_new_symbol_is_exported_with_the_declared_signature():
    L = pdwt_amd.hip()
    for s in NEW_PLAIN + ["pdwt_%s_%s" % (t, sfx) for t in NEW_TYPED for sfx in ("f32", "f64")]:
        assert hasattr(L, s), s
    assert L.pdwt_ext3d_adjoint_level_tmp_elems.restype is C.c_longlong and len(L.pdwt_ext3d_adjoint_level_tmp_elems.argtypes) == 4
    for sfx in ("f32", "f64"):
        assert len(getattr(L, "pdwt_ext3d_forward_adjoint_level_" + sfx).argtypes) == 8
        assert len(getattr(L, "pdwt_ext3d_inverse_adjoint_level_" + sfx).argtypes) == 7
    want = {"dwt3": ["x", "wname", "levels", "mode"], "idwt3": ["bands", "shape", "wname"], "dwt3_adjoint": ["bands", "shape", "wname", "mode"],
            "idwt3_adjoint": ["x", "wname", "levels"]}
    for name, args in want.items():
        fn = getattr(pdwt_amd, name)
        assert fn is getattr(pdwt_amd.functional, name) and name in pdwt_amd.__all__ and name in pdwt_amd.functional.__all__
        sig = inspect.signature(fn)
        assert list(sig.parameters) == args, (name, sig)
        assert {k: p.default for k, p in sig.parameters.items() if p.default is not inspect.Parameter.empty} == {
            k: v for k, v in (("levels", 1), ("mode", "symmetric")) if k in args}
    assert "coarsest" in pdwt_amd.dwt3.__doc__.lower() and "dwt2" in pdwt_amd.dwt3.__doc__


def _pad64(n):
    return (n + 63) // 64 * 64


def test_scratch_geometry():
    L = pdwt_amd.hip()
    g = L.pdwt_ext3d_adjoint_level_tmp_elems
    # pad64(4 nz hr hc) for the quadrants, then nz frames of (2 hr + F - 2)(2 hc + F - 2) - nr nc cells
    for nz, nr, nc, F in ((40, 24, 24, 4), (9, 33, 47, 2), (7, 7, 7, 8), (40, 48, 40, 40), (6, 104, 200, 4), (30, 32, 36, 16)):
        hr, hc = (nr + F - 1) // 2, (nc + F - 1) // 2
        assert g(nz, nr, nc, F) == _pad64(4 * nz * hr * hc) + nz * ((2 * hr + F - 2) * (2 * hc + F - 2) - nr * nc), (nz, nr, nc, F)
    assert g(9, 33, 47, 2) == _pad64(4 * 9 * 17 * 24) + 9 * (34 * 48 - 33 * 47)
    # enough for the forward level it also serves (the inverse adjoint): the four quadrants
    assert g(40, 24, 24, 4) >= 4 * 40 * 13 * 13
    for bad in ((0, 8, 8, 4), (8, 0, 8, 4), (8, 8, 0, 4), (2, 8, 8, 4), (8, 2, 8, 4), (8, 8, 2, 4), (8, 8, 8, 3), (8, 8, 8, 0), (80, 80, 80, 42), (65536, 8, 8, 4),
                (8, 1 << 16, 1 << 15, 4)):
        assert g(*bad) == -1, bad
    assert g(65535, 3, 3, 4) > 0


def _targets(nz, F, mode):
    """the samples that the halo cells of a line repeat (mode by name), from the reference's own index map"""
    from tests import refext as R
    hz = (nz + F - 1) // 2
    s = np.array([v for v in range(2 - F, 2 * hz) if v < 0 or v >= nz], np.int64)
    idx, ok = R.ext_index(s, nz, mode)
    return sorted(int(i) for i, o in zip(idx, ok) if o)


@pytest.mark.parametrize("nz,F", [(40, 4), (21, 4), (7, 8), (9, 2), (40, 40), (39, 40), (50, 16), (1, 2)])
def test_interior_run_of_the_z_pass(nz, F):
    L = pdwt_amd.hip()
    for m, mode in enumerate(R3.MODES):
        z0, z1 = C.c_int(-7), C.c_int(-7)
        assert L.pdwt_ext3d_adjoint_z_run(nz, F, m, C.byref(z0), C.byref(z1)) == 0
        t = _targets(nz, F, mode)
        assert 0 <= z0.value <= z1.value <= nz
        assert not [k for k in t if z0.value <= k < z1.value], (mode, t, z0.value, z1.value)
        # the longest such run
        edges = [-1] + t + [nz]
        assert z1.value - z0.value == max(b - a - 1 for a, b in zip(edges, edges[1:])), (mode, t, z0.value, z1.value)
    assert L.pdwt_ext3d_adjoint_z_run(nz, F, 5, None, None) == -1 and L.pdwt_ext3d_adjoint_z_run(nz, F + 1, 2, None, None) == -1
    assert L.pdwt_ext3d_adjoint_z_run(65536, 2, 2, None, None) == -1 and L.pdwt_ext3d_adjoint_z_run(F - 2, F, 2, None, None) == -1
    assert L.pdwt_ext3d_adjoint_z_run(nz, F, 2, None, None) == 0


@pytest.mark.parametrize("sfx", ["f32", "f64"])
def test_the_level_entries_refuse_bad_arguments_before_they_touch_anything(sfx):
    L = pdwt_amd.hip()
    f = (nat.Filters32 if sfx == "f32" else nat.Filters64)()
    f.hlen = getattr(L, "pdwt_compute_filters_separable_" + sfx)(b"db4", 0, C.byref(f))
    assert f.hlen == 8
    fp, p = C.byref(f), FAKE
    fwd, inv = (getattr(L, "pdwt_ext3d_%s_adjoint_level_%s" % (d, sfx)) for d in ("forward", "inverse"))
    tab = (C.c_void_p * 8)(*[p] * 8)
    refused = [
        # a NULL in each position
        fwd(None, tab, 16, 17, 18, 2, fp, p), fwd(p, None, 16, 17, 18, 2, fp, p), fwd(p, tab, 16, 17, 18, 2, None, p), fwd(p, tab, 16, 17, 18, 2, fp, None),
        inv(None, tab, 16, 17, 18, fp, p), inv(p, None, 16, 17, 18, fp, p), inv(p, tab, 16, 17, 18, None, p), inv(p, tab, 16, 17, 18, fp, None),
        # a bad mode
        fwd(p, tab, 16, 17, 18, -1, fp, p), fwd(p, tab, 16, 17, 18, 5, fp, p),
        # an axis below hlen - 1 = 7, or none at all
        fwd(p, tab, 6, 17, 18, 2, fp, p), fwd(p, tab, 16, 6, 18, 2, fp, p), fwd(p, tab, 16, 17, 6, 2, fp, p), fwd(p, tab, 0, 17, 18, 2, fp, p),
        inv(p, tab, 6, 17, 18, fp, p), inv(p, tab, 16, 6, 18, fp, p), inv(p, tab, 16, 17, 6, fp, p), inv(p, tab, 16, 0, 18, fp, p),
        # nz above 65535; a plane of 2^31 elements
        fwd(p, tab, 65536, 17, 18, 2, fp, p), inv(p, tab, 65536, 17, 18, fp, p), fwd(p, tab, 16, 1 << 16, 1 << 15, 2, fp, p), inv(p, tab, 16, 1 << 16, 1 << 15, fp, p),
    ]
    # a hole in the table, at every position
    for k in range(8):
        hole = (C.c_void_p * 8)(*[None if j == k else p for j in range(8)])
        refused += [fwd(p, hole, 16, 17, 18, 2, fp, p), inv(p, hole, 16, 17, 18, fp, p)]
    assert refused == [-1] * len(refused), [k for k, rc in enumerate(refused) if rc != -1]
    # an odd or oversized bank length
    for hlen in (7, 0, 42):
        f.hlen = hlen
        assert fwd(p, tab, 64, 64, 64, 2, fp, p) == -1 and inv(p, tab, 64, 64, 64, fp, p) == -1, hlen


def test_the_functional_layer_wants_tensors():
    x = np.zeros((8, 8, 8), np.float32)
    with pytest.raises(TypeError):
        pdwt_amd.dwt3(x, "db2", 1)
    with pytest.raises(TypeError):
        pdwt_amd.idwt3([x] * 8, (8, 8, 8), "db2")
    with pytest.raises(TypeError):
        pdwt_amd.dwt3_adjoint([x] * 8, (8, 8, 8), "db2")
    with pytest.raises(TypeError):
        pdwt_amd.idwt3_adjoint(x, "db2", 1)
    with pytest.raises(TypeError):
        pdwt_amd.dwt3([[0.0]], "db2", 1)
