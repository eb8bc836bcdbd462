"""Pin tests/ref2d.py, the float64 reference tests/test_all_banks_gpu.py holds every 1-D / 2-D kernel family to (CPU only).

  * every PyWavelets golden of tests/golden/ (2-D and SWT ones fix the band order, H versus V included; the batched 1-D and SWT 1-D
    ones the 1-D forms the reference dispatches to), bands and pywt's reconstruction;
  * the oracle in float64 on odd and even shapes, several levels, every kind, orthogonal and biorthogonal banks -- an independent
    statement of the same sums, so the two agree to rounding (1e-13 here);
  * perfect reconstruction of the orthogonal banks, and impulse responses that tell H from V in closed form."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import ref2d, ref3d
from tests.helpers import GOLDEN_CASES, KIND, band_err, golden_bands, load_golden

# float32 goldens were computed by PyWavelets in float32: they sit at float32 rounding from any float64 statement
GOLDEN_TOL = {np.dtype(np.float32): 2e-6, np.dtype(np.float64): 1e-12}


@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_pywt_goldens_fix_bands_order_and_reconstruction(name):
    d = load_golden(name)
    x = d["input"]
    kind = d["kind"]
    L = ref2d.levels_of(x.shape, d["wname"], d["levels"], kind)
    assert L == d["levels"]
    got = ref2d.forward(kind, x, d["wname"], L)
    exp = golden_bands(d)
    assert len(got) == len(exp)
    tol = GOLDEN_TOL[x.dtype]
    for k, (g, e) in enumerate(zip(got, exp)):
        assert g.shape == e.shape, (name, k)
        assert band_err(g, e) <= tol, (name, "band", k, band_err(g, e))
    if kind in ("dwt2", "swt2"):  # H and V swapped must NOT pass: the goldens really tell the two apart
        assert band_err(got[1], exp[2]) > 1e-2, name
    rec = ref2d.inverse(kind, exp, x.shape, d["wname"])
    assert band_err(rec, d["recon"]) <= tol, (name, band_err(rec, d["recon"]))


ORACLE_CASES = [
    # kind, shape, bank, levels
    ("dwt2", (64, 96), "db4", 3), ("dwt2", (63, 65), "db2", 2), ("dwt2", (45, 77), "bior2.4", 2), ("dwt2", (50, 37), "rbio3.3", 2),
    ("dwt2", (81, 94), "bior3.9", 2), ("dwt2", (160, 171), "sym20", 2), ("dwt2", (37, 51), "haar", 3), ("dwt2", (96, 101), "rbio6.8", 2),
    ("swt2", (48, 80), "db2", 3), ("swt2", (45, 51), "bior2.2", 2), ("swt2", (64, 72), "rbio3.1", 3), ("swt2", (99, 80), "bior6.8", 2),
    ("swt2", (33, 40), "haar", 3), ("swt2", (160, 157), "sym20", 2),
    ("dwt1", (3, 77), "db3", 2), ("dwt1", (5, 256), "bior4.4", 4), ("dwt1", (2, 201), "rbio2.8", 3), ("dwt1", (4, 65), "haar", 3),
    ("swt1", (6, 128), "sym4", 3), ("swt1", (3, 77), "rbio1.5", 2), ("swt1", (2, 90), "bior5.5", 3),
]


@pytest.mark.parametrize("kind,shape,wname,levels", ORACLE_CASES, ids=["%s-%dx%d-%s-L%d" % (k, s[0], s[1], w, l) for k, s, w, l in ORACLE_CASES])
def test_float64_oracle_on_odd_and_even_shapes(kind, shape, wname, levels):
    x = np.random.RandomState(sum(shape) + levels).uniform(-100, 100, shape)
    O = orc.OracleWavelets(x, wname, levels, **KIND[kind])
    L = O.info.nlevels
    assert L == levels == ref2d.levels_of(shape, wname, levels, kind)
    O.forward()
    want = O.coeffs
    got = ref2d.forward(kind, x, wname, L)
    assert len(got) == len(want)
    for k, (g, o) in enumerate(zip(got, want)):
        assert g.shape == o.shape, (k, g.shape, o.shape)
        assert band_err(g, o) <= 1e-13, (k, band_err(g, o))
    O.inverse()
    rec = ref2d.inverse(kind, want, shape, wname)
    assert rec.shape == tuple(shape)
    assert band_err(rec, O.get_image()) <= 1e-13, band_err(rec, O.get_image())


@pytest.mark.parametrize("kind,shape,wname,levels", ORACLE_CASES, ids=["%s-%dx%d-%s-L%d" % (k, s[0], s[1], w, l) for k, s, w, l in ORACLE_CASES])
def test_matrix_form_equals_the_composition_of_the_primitives(kind, shape, wname, levels):
    """ref2d.forward / inverse (one matrix per axis and level, written from the index formulas) against the compositions of the
    ref3d primitives: the same sums in another order"""
    x = np.random.RandomState(sum(shape)).uniform(-100, 100, shape)
    a, b = ref2d.forward(kind, x, wname, levels), ref2d.forward_direct(kind, x, wname, levels)
    assert len(a) == len(b)
    for g, o in zip(a, b):
        assert g.shape == o.shape and band_err(g, o) <= 1e-14
    assert band_err(ref2d.inverse(kind, b, shape, wname), ref2d.inverse_direct(kind, b, shape, wname)) <= 1e-14


def test_lines_too_long_for_a_matrix_run_the_primitives():
    x = np.random.RandomState(1).uniform(-100, 100, (2, 8192))
    for kind in ("dwt1", "swt1"):
        c = ref2d.forward(kind, x, "bior2.4", 2)
        d = ref2d.forward_direct(kind, x, "bior2.4", 2)
        assert np.array_equal(c[1], d[1])  # the level of 8192 samples: the primitives themselves
        for g, o in zip(c, d):
            assert band_err(g, o) <= 1e-14
        assert band_err(ref2d.inverse(kind, c, x.shape, "bior2.4"), x) <= 1e-12


def test_level_clamp_matches_the_oracle():
    for kind, shape, wname in (("dwt2", (64, 200), "db4"), ("dwt2", (37, 51), "haar"), ("swt2", (100, 57), "db3"), ("dwt1", (3, 300), "sym8"),
                               ("swt1", (2, 77), "db2"), ("dwt2", (39, 39), "db20"), ("dwt2", (38, 80), "db20")):
        O_L = orc.OracleWavelets(np.zeros(shape), wname, 99, **KIND[kind]).info.nlevels
        assert ref2d.levels_of(shape, wname, 99, kind) == O_L, (kind, shape, wname)
    assert ref2d.levels_of((64, 64), "db4", 0) == 1


ORTHO = ["haar", "db2", "db7", "db12", "db20", "sym5", "coif1", "coif3", "coif5"]


@pytest.mark.parametrize("wname", ORTHO)
def test_perfect_reconstruction_of_orthogonal_banks(wname):
    """db*, coif* and the short sym* banks of the table are orthogonal to better than 1e-12 (the long sym* banks are not: their defect
    is measured per bank in tests/test_all_banks_gpu.py); even and odd-sized decimated, stationary, and the 1-D forms"""
    m = len(ref3d.bank(wname)[0]) - 1
    rs = np.random.RandomState(m)
    for kind, shape in (("dwt2", (4 * m + 4, 4 * m + 8)), ("swt2", (4 * m + 1, 4 * m + 3)), ("dwt1", (3, 4 * m + 4)), ("swt1", (2, 4 * m + 5))):
        x = rs.uniform(-100, 100, shape)
        c = ref2d.forward(kind, x, wname, 2)
        assert band_err(ref2d.inverse(kind, c, shape, wname), x) <= 1e-11, (kind, wname)
    # odd decimated sizes reconstruct too (the repeated sample is dropped again)
    x = rs.uniform(-100, 100, (4 * m + 3, 4 * m + 5))
    assert band_err(ref2d.inverse("dwt2", ref2d.forward("dwt2", x, wname, 2), x.shape, wname), x) <= 1e-11, wname


def test_h_is_high_pass_along_the_columns_and_v_along_the_rows():
    """closed form: an image that varies along axis 0 only (every row constant) has no V and no D band; one that varies along axis 1
    only has no H and no D band -- for the decimated and the stationary transform, orthogonal and biorthogonal banks"""
    rs = np.random.RandomState(3)
    for wname in ("db3", "bior2.4", "rbio3.3"):
        col = rs.uniform(-1, 1, (40, 1)) * np.ones((1, 48))
        row = np.ones((40, 1)) * rs.uniform(-1, 1, (1, 48))
        for kind in ("dwt2", "swt2"):
            A, H, V, D = ref2d.forward(kind, col, wname, 1)
            assert np.abs(H).max() > 1e-2 and np.abs(V).max() < 1e-12 and np.abs(D).max() < 1e-12, (wname, kind)
            A, H, V, D = ref2d.forward(kind, row, wname, 1)
            assert np.abs(V).max() > 1e-2 and np.abs(H).max() < 1e-12 and np.abs(D).max() < 1e-12, (wname, kind)
