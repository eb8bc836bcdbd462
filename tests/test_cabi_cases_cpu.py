"""The bar of the C-ABI buffer tests (case matrix: tests/cabi_cases.py) is reachable: they hold a float32 kernel to
TOL[float32] = 1e-5 against a FLOAT64 reference (the rest of the suite compares with the float32 oracle).  Here, on the CPU, the
float32 oracle -- the reference's own arithmetic in float32 -- is compared with the float64 oracle on every transform case of the
matrix: every band and the reconstruction must stay within TOL[float32] / 4, so a kernel with the oracle's accuracy has a factor of
four to spare.  The 3-D cases use tests/ref3d.py with float32 taps, products and accumulators against the same sums in float64."""
import numpy as np
import pytest

from tests import cabi_cases as M
from tests.helpers import TOL, band_err

F32, F64 = np.dtype(np.float32), np.dtype(np.float64)
BAR = TOL[F32] / 4
_CASES = [c for c in M.TRANSFORM_CASES if "f32" in c["dtypes"] and not c["fam"].startswith("haar")]


def _f32_results(case):
    if case["fam"] in ("dwt3", "swt3"):
        from tests import ref3d
        x = M.case_input(case)
        L = ref3d.levels_of(case["shape"], case["wname"], case["levels"])
        if case["fam"] == "dwt3":
            c = ref3d.dwt3_forward(x, case["wname"], L, np.float32)
            return c, ref3d.dwt3_inverse(c, x.shape, case["wname"], L, np.float32)
        c = ref3d.swt3_forward(x, case["wname"], L, np.float32)
        return c, ref3d.swt3_inverse(c, case["wname"], L, np.float32)
    O = M.oracle_for(case, np.float32)
    c = O.coeffs
    O.inverse()
    return c, O.get_image()


@pytest.mark.parametrize("case", _CASES, ids=[c["id"] for c in _CASES])
def test_float32_oracle_is_within_a_quarter_of_the_bar(case):
    """Largest ratio error / (TOL / 4) observed over all cases: 0.24 (lds97x131-sym13-L1 and swt96x128-db20-L1); see docs/EXPERIMENTS.md."""
    _, _, rbands, rrec = M.reference(case, F64)
    bands, rec = _f32_results(case)
    assert len(bands) == len(rbands)
    worst = 0.0
    for k, (b, r) in enumerate(zip(bands, rbands)):
        assert b.dtype == np.float32
        e = band_err(b, r)
        worst = max(worst, e)
        assert e <= BAR, (case["id"], "band", k, e)
    e = band_err(rec, rrec)
    worst = max(worst, e)
    print("%s: worst ratio %.3f" % (case["id"], worst / BAR))
    assert e <= BAR, (case["id"], "reconstruction", e)


def test_case_table_is_consistent():
    ids = [c["id"] for c in M.TRANSFORM_CASES]
    assert len(set(ids)) == len(ids)
    assert {c["fam"] for c in M.TRANSFORM_CASES} == set(M.FAMILIES)
    for fam in M.FAMILIES:  # every family in both precisions
        for sfx in ("f32", "f64"):
            assert [c for c in M.TRANSFORM_CASES if c["fam"] == fam and sfx in c["dtypes"]], (fam, sfx)
    for c in M.TRANSFORM_CASES:
        assert set(c["dtypes"]) <= {"f32", "f64"} and c["dtypes"]
    for g in M.GATES:
        assert g["case"] in M.CASE_BY_ID and g["dt"] in M.CASE_BY_ID[g["case"]]["dtypes"], g
        assert g["dir"] in ("fwd", "inv") and g["flips"] and set(g["flips"]) <= set(M.LAYOUTS) - {"aligned"}
        assert g["fast"] and g["slow"]
    for branch, cases in M.VEC_BRANCHES.items():
        assert cases and all(c in M.CASE_BY_ID for c in cases), branch


def test_layouts_misalign_what_they_say():
    names = ["image", "tmp", "band0", "band1", "band2", "band6"]
    got = {l: [M.misalign(l, n, 2, 6) for n in names] for l in M.LAYOUTS}
    assert got == {"aligned": [0] * 6, "packed": [0] * 6, "image+1": [1, 0, 0, 0, 0, 0], "tmp+1": [0, 1, 0, 0, 0, 0], "bands+1": [0, 0, 1, 1, 1, 1],
                   "band0+1": [0, 0, 1, 0, 0, 0], "fine+1": [0, 0, 0, 0, 1, 0], "coarse+1": [0, 0, 0, 0, 0, 1], "all+1": [1] * 6, "all+2": [2] * 6}
    assert M.misalign("coarse+1", "i1_band6", 2, 6) == 1 and M.misalign("image+1", "i1_image", 2, 6) == 1


def test_packed_layouts_misalign_by_themselves():
    """the packed layout lays the bands back to back from a 256-byte boundary (band 0 at its level-1 allocation): in each precision at
    least one 2-D and one 1-D case must put a band at an address that is no multiple of 16 bytes by packing alone"""
    from oracle.oracle import band_shapes
    for sfx, item in (("f32", 4), ("f64", 8)):
        for fam, ndim in (("dwt2", 2), ("dwt1", 1)):
            odd = []
            for c in M.TRANSFORM_CASES:
                if c["fam"] != fam or sfx not in c["dtypes"]:
                    continue
                levels = M.reference(c, F64)[0]
                sizes = [r * k for r, k in band_shapes(c["shape"][0], c["shape"][1], levels, 0, ndim)]
                sizes[0] = sizes[1]  # the allocation of band 0
                starts = np.cumsum([0] + sizes[:-1]) * item
                if (starts % 16).any():
                    odd.append(c["id"])
            assert odd, (sfx, fam)
