"""CPU-only: the reference of the adjoints (tests/refadj.py) against dense matrices built from tests/refext.py, the float32 error of the
kernels' summation order on every GPU case of tests/test_adjoint_gpu.py, and what the built libraries answer without a device: the
new symbols, the scratch geometry and the refusals of every adjoint driver on fake pointers.

Bounds of the GPU tests.  The family's: 1e-5 (float32) / 1e-12 (float64) of max|ref|, valid for a case as long as the float32 figure
measured here is at most a quarter of it (2.5e-6).  Measured (pytest -s): every case lies between 7e-8 and 3.1e-7 -- the worst are the
`constant` corner of the 40-tap bank on (96, 80), 2.4e-7 (up to 40 x 40 pre-images of the corner sample), and the inverse adjoint of the
same case, 3.1e-7 -- so no case needs a bound of its own."""
import ctypes as C

import numpy as np
import pytest

import pdwt_amd
from pdwt_amd import _native as nat
from tests import refadj as A
from tests import refext as R

BANKS = ("haar", "db2", "db4", "bior2.2", "sym8")
F32_BOUND, F64_BOUND = 1e-5, 1e-12
FAKE = 0x10000  # a pointer that is never dereferenced: every call below must be refused first


def _lengths(F):
    return sorted({n for n in (F - 1, F, F + 1, 2 * F + 3, 37) if n >= max(F - 1, 1)})


@pytest.mark.parametrize("wname", BANKS)
def test_line_adjoint_is_the_transpose_of_the_analysis_matrix(wname):
    F, t = R.bank(wname)
    rs = np.random.RandomState(5)
    worst = 0.0
    for n in _lengths(F):
        N = (n + F - 1) // 2
        for mode in R.MODES:
            M = A.dense(lambda x: list(R.analysis(x, t["L"], t["H"], mode)), n)
            assert M.shape == (2 * N, n)
            c = rs.standard_normal(2 * N)
            got = A.analysis_adjoint(c[:N], c[N:], t["L"], t["H"], n, mode)
            worst = max(worst, float(np.abs(got - M.T @ c).max()))
    print("%s: worst |adj - M^T c| = %.2e" % (wname, worst))
    assert worst <= 1e-13


@pytest.mark.parametrize("wname", BANKS)
def test_inverse_adjoint_is_the_transpose_of_the_synthesis_matrix_and_a_zero_mode_analysis(wname):
    F, t = R.bank(wname)
    rs = np.random.RandomState(6)
    for n in _lengths(F):
        N = (n + F - 1) // 2
        S = A.dense(lambda c: R.synthesis(c[:N], c[N:], t["IL"], t["IH"], n), 2 * N)
        y = rs.standard_normal(n)
        a, d = A.synthesis_adjoint(y, t["IL"], t["IH"])
        assert np.abs(np.concatenate([a, d]) - S.T @ y).max() <= 1e-13
        a2, d2 = R.analysis(y, np.ascontiguousarray(t["IL"][::-1]), np.ascontiguousarray(t["IH"][::-1]), "zero")
        assert np.array_equal(a, a2) and np.array_equal(d, d2)


@pytest.mark.parametrize("mode", R.MODES)
def test_multilevel_2d_operator_identity(mode):
    rs = np.random.RandomState(7)
    x = rs.standard_normal((13, 18))
    b = R.wavedec2(x, "db2", 2, mode)
    c = [rs.standard_normal(v.shape) for v in b]
    lhs = sum(float((u * v).sum()) for u, v in zip(b, c))
    rhs = float((x * A.wavedec2_adjoint(c, (13, 18), "db2", mode)).sum())
    assert abs(lhs - rhs) <= 1e-12 * abs(lhs), (lhs, rhs)
    y = rs.standard_normal((13, 18))
    lhs = float((R.waverec2(c, (13, 18), "db2") * y).sum())
    rhs = sum(float((u * v).sum()) for u, v in zip(c, A.waverec2_adjoint(y, "db2", 2)))
    assert abs(lhs - rhs) <= 1e-12 * abs(lhs), (lhs, rhs)


def test_float32_error_of_the_kernel_order_on_every_gpu_case():
    """the figure that decides whether the family's bound holds for a case (module docstring)"""
    worst = 0.0
    for shape, w, L, modes in A.CASES_2D:
        F, _ = R.bank(w)
        c = A.cotangent(R.band_shapes(shape, F, L), (3,), 1)
        for mode in modes:
            e = A.rel_err(A.wavedec2_adjoint(c, shape, w, mode, np.float32), A.wavedec2_adjoint(c, shape, w, mode))
            print("2-D %-10s %-8s L%d %-9s float32 order: %.2e" % (shape, w, L, mode, e))
            worst = max(worst, e)
        x = A.cotangent([shape], (3,), 2)[0]
        e = max(A.rel_err(p, q) for p, q in zip(A.waverec2_adjoint(x, w, L, np.float32), A.waverec2_adjoint(x, w, L)))
        print("2-D %-10s %-8s L%d inverse adjoint float32 order: %.2e" % (shape, w, L, e))
        worst = max(worst, e)
    for (rows, n), w, L, modes, _ in A.CASES_1D:
        F, _ = R.bank(w)
        ns = A.lengths(n, F, L)
        c = A.cotangent([(ns[L],)] + [(k,) for k in ns[1:]], (rows,), 3)
        for mode in modes:
            e = A.rel_err(A.wavedec1_adjoint(c, n, w, mode, np.float32), A.wavedec1_adjoint(c, n, w, mode))
            print("1-D %-12s %-8s L%d %-9s float32 order: %.2e" % ((rows, n), w, L, mode, e))
            worst = max(worst, e)
        x = A.cotangent([(n,)], (rows,), 4)[0]
        e = max(A.rel_err(p, q) for p, q in zip(A.waverec1_adjoint(x, w, L, np.float32), A.waverec1_adjoint(x, w, L)))
        print("1-D %-12s %-8s L%d inverse adjoint float32 order: %.2e" % ((rows, n), w, L, e))
        worst = max(worst, e)
    assert 4 * worst <= F32_BOUND, worst


# ---- the built libraries, no device ----------------------------------------------------------------------------------------------------
NEW_PLAIN = ["pdwt_ext2db_adjoint_tmp_elems", "pdwt_ext1d_adjoint_tmp_elems"]
NEW_TYPED = ["ext2db_forward_adjoint_level", "ext2db_forward_adjoint", "ext2db_inverse_adjoint",
             "ext1d_forward_adjoint_level", "ext1d_forward_adjoint", "ext1d_inverse_adjoint"]


def test_every_adjoint_symbol_is_exported_and_the_module_is_there():
    L = pdwt_amd.hip()
    for s in NEW_PLAIN + ["pdwt_%s_%s" % (t, sfx) for t in NEW_TYPED for sfx in ("f32", "f64")]:
        assert hasattr(L, s), s
    for name in ("dwt2", "idwt2", "dwt1", "idwt1", "dwt2_adjoint", "idwt2_adjoint", "dwt1_adjoint", "idwt1_adjoint"):
        assert callable(getattr(pdwt_amd, name)) and getattr(pdwt_amd.functional, name) is getattr(pdwt_amd, name)


def test_scratch_geometry():
    L = pdwt_amd.hip()
    # 2-D: B frames of (Nr + 2F - 3)(Nc + 2F - 3) - Nr Nc cells, plus two approximation stacks when there is more than one level
    assert L.pdwt_ext2db_adjoint_tmp_elems(3, 13, 18, 4, 2, 4) == 3 * (18 * 23 - 13 * 18) + 2 * 3 * 8 * 10
    assert L.pdwt_ext2db_adjoint_tmp_elems(1, 96, 80, 40, 1, 8) == (96 + 77) * (80 + 77) - 96 * 80
    assert L.pdwt_ext2db_adjoint_tmp_elems(2, 33, 47, 2, 3, 4) == 2 * (34 * 48 - 33 * 47) + 2 * 2 * 17 * 24
    for bad in ((0, 13, 18, 4, 2, 4), (65536, 13, 18, 4, 2, 4), (1, 2, 18, 4, 1, 4), (1, 13, 18, 4, 0, 4), (1, 13, 18, 4, 33, 4), (1, 13, 18, 3, 1, 4),
                (1, 13, 18, 4, 1, 2), (1, 13, 18, 42, 1, 4)):
        assert L.pdwt_ext2db_adjoint_tmp_elems(*bad) == -1, bad
    # 1-D: 0 when all levels run in one launch, else the halo cells of a level and two approximation stacks
    assert L.pdwt_ext1d_adjoint_tmp_elems(2, 4099, 8, 5, 8) == 0 and L.pdwt_ext1d_adjoint_tmp_elems(5, 77, 2, 3, 4) == 0
    assert L.pdwt_ext1d_fused(40037, 8, 3, 4) == 0
    assert L.pdwt_ext1d_adjoint_tmp_elems(2, 40037, 8, 3, 4) == 2 * 13 + 2 * 2 * 20022
    assert L.pdwt_ext1d_adjoint_tmp_elems(2, 40037, 8, 1, 4) == 2 * 13
    # (a row that the forward transform still fuses but whose adjoint pipeline, one padded detail line more, does not fit)
    n = 26000
    assert L.pdwt_ext1d_fused(n, 8, 2, 4) == 1 and L.pdwt_ext1d_adjoint_tmp_elems(3, n, 8, 2, 4) == 3 * 13 + 2 * 3 * ((n + 7) // 2)
    for bad in ((0, 77, 2, 3, 4), (2, 6, 8, 1, 4), (2, 77, 2, 0, 4), (2, 77, 2, 33, 4), (2, 77, 5, 1, 4), (2, 77, 2, 1, 3)):
        assert L.pdwt_ext1d_adjoint_tmp_elems(*bad) == -1, bad


@pytest.mark.parametrize("sfx", ["f32", "f64"])
def test_every_adjoint_driver_refuses_bad_arguments_before_it_touches_anything(sfx):
    L = pdwt_amd.hip()
    f = (nat.Filters32 if sfx == "f32" else nat.Filters64)()
    f.hlen = getattr(L, "pdwt_compute_filters_separable_" + sfx)(b"db4", 0, C.byref(f))
    assert f.hlen == 8
    fp = C.byref(f)
    p = FAKE
    g = lambda name: getattr(L, "pdwt_%s_%s" % (name, sfx))
    tab2 = (C.c_void_p * 7)(*[p] * 7)
    hole2 = (C.c_void_p * 7)(p, p, p, None, p, p, p)
    tab1 = (C.c_void_p * 3)(p, p, p)
    hole1 = (C.c_void_p * 3)(p, None, p)
    lev2, all2, inv2 = g("ext2db_forward_adjoint_level"), g("ext2db_forward_adjoint"), g("ext2db_inverse_adjoint")
    lev1, all1, inv1 = g("ext1d_forward_adjoint_level"), g("ext1d_forward_adjoint"), g("ext1d_inverse_adjoint")
    refused = [
        # mode -1 or 5
        lev2(p, p, p, p, p, 3, 61, 67, -1, fp, p), lev2(p, p, p, p, p, 3, 61, 67, 5, fp, p),
        all2(p, tab2, 3, 61, 67, 2, -1, fp, p), all2(p, tab2, 3, 61, 67, 2, 5, fp, p),
        lev1(p, p, p, 3, 77, -1, fp, p), lev1(p, p, p, 3, 77, 5, fp, p), all1(p, tab1, 3, 77, 2, -1, fp, p), all1(p, tab1, 3, 77, 2, 5, fp, p),
        # B 0 or 65536 (1-D: no rows)
        lev2(p, p, p, p, p, 0, 61, 67, 2, fp, p), lev2(p, p, p, p, p, 65536, 61, 67, 2, fp, p),
        all2(p, tab2, 0, 61, 67, 2, 2, fp, p), all2(p, tab2, 65536, 61, 67, 2, 2, fp, p),
        inv2(p, tab2, 0, 61, 67, 2, fp, p), inv2(p, tab2, 65536, 61, 67, 2, fp, p),
        lev1(p, p, p, 0, 77, 2, fp, p), all1(p, tab1, 0, 77, 2, 2, fp, p), inv1(p, tab1, 0, 77, 2, fp, p),
        # an axis shorter than hlen - 1, at the first or at a deeper level ((7, 7) db4 has 7 samples at every level; 6 is too short)
        lev2(p, p, p, p, p, 3, 6, 67, 2, fp, p), lev2(p, p, p, p, p, 3, 61, 6, 2, fp, p),
        all2(p, tab2, 3, 6, 67, 2, 2, fp, p), all2(p, tab2, 3, 61, 6, 2, 2, fp, p), inv2(p, tab2, 3, 6, 67, 2, fp, p), inv2(p, tab2, 3, 61, 6, 2, fp, p),
        lev1(p, p, p, 3, 6, 2, fp, p), all1(p, tab1, 3, 6, 2, 2, fp, p), inv1(p, tab1, 3, 6, 2, fp, p),
        # 0 or 33 levels
        all2(p, tab2, 3, 61, 67, 0, 2, fp, p), all2(p, tab2, 3, 61, 67, 33, 2, fp, p), inv2(p, tab2, 3, 61, 67, 0, fp, p), inv2(p, tab2, 3, 61, 67, 33, fp, p),
        all1(p, tab1, 3, 77, 0, 2, fp, p), all1(p, tab1, 3, 77, 33, 2, fp, p), inv1(p, tab1, 3, 77, 0, fp, p), inv1(p, tab1, 3, 77, 33, fp, p),
        # a NULL bank or pointer (the scratch of a call that folds included)
        lev2(p, p, p, p, p, 3, 61, 67, 2, None, p), lev2(None, p, p, p, p, 3, 61, 67, 2, fp, p), lev2(p, p, None, p, p, 3, 61, 67, 2, fp, p),
        lev2(p, p, p, p, p, 3, 61, 67, 2, fp, None),
        all2(p, tab2, 3, 61, 67, 2, 2, None, p), all2(None, tab2, 3, 61, 67, 2, 2, fp, p), all2(p, None, 3, 61, 67, 2, 2, fp, p),
        all2(p, tab2, 3, 61, 67, 2, 2, fp, None),
        inv2(p, tab2, 3, 61, 67, 2, None, p), inv2(None, tab2, 3, 61, 67, 2, fp, p), inv2(p, None, 3, 61, 67, 2, fp, p),
        lev1(p, p, p, 3, 77, 2, None, p), lev1(None, p, p, 3, 77, 2, fp, p), lev1(p, None, p, 3, 77, 2, fp, p), lev1(p, p, p, 3, 77, 2, fp, None),
        all1(p, tab1, 3, 77, 2, 2, None, p), all1(None, tab1, 3, 77, 2, 2, fp, p), all1(p, None, 3, 77, 2, 2, fp, p),
        all1(p, tab1, 2, 40037, 2, 2, fp, None),  # (per level: the scratch is needed)
        inv1(p, tab1, 3, 77, 2, None, p), inv1(None, tab1, 3, 77, 2, fp, p), inv1(p, None, 3, 77, 2, fp, p),
        # a hole in the table
        all2(p, hole2, 3, 61, 67, 2, 2, fp, p), inv2(p, hole2, 3, 61, 67, 2, fp, p), all1(p, hole1, 3, 77, 2, 2, fp, p), inv1(p, hole1, 3, 77, 2, fp, p),
    ]
    assert refused == [-1] * len(refused), [k for k, rc in enumerate(refused) if rc != -1]
    # a bank of a bad length
    f.hlen = 7
    assert lev2(p, p, p, p, p, 3, 61, 67, 2, fp, p) == -1 and inv2(p, tab2, 3, 61, 67, 2, fp, p) == -1 and inv1(p, tab1, 3, 77, 2, fp, p) == -1
