"""tests/bank_matrix.py (the kernel-family x filter-bank matrix of tests/test_all_banks_gpu.py) is tied to the sources, complete, and
its float32 bar reachable (CPU only):

  * every length list of the matrix equals the `#define PDWT_*_HLENS(X)` list (or the `case N:` lines of inv2d_casc3_f32) it names,
    parsed out of pdwt_amd/csrc, and no such list exists in the sources that the matrix does not know: an instantiation added later
    without a case fails here;
  * every instantiation of every kernel template that a transform can reach (per template and precision: one list feeds several
    templates) is proved to run by the launch evidence of at least one case, and every bank has a case in every row that accepts its length;
  * the geometry rules replayed in the matrix (LDS budget of the tiled kernels, the cascade launchers) say what its rows assume;
  * for every case shape the reference's own float32 evaluation -- the oracle in float32 -- stays within a quarter of the float32
    bound from the float64 reference tests/ref2d.py, forward and inverse (the check tests/test_cabi_cases_cpu.py makes for its matrix)."""
import functools
import glob
import os
import re

import numpy as np
import pytest

from oracle import oracle as orc
from tests import bank_matrix as M
from tests import ref2d
from tests.helpers import KIND, ROOT, TOL, band_err

CSRC = os.path.join(ROOT, "pdwt_amd", "csrc")
F32 = np.dtype(np.float32)
BAR = TOL[F32] / 4


def _lists_of(fname, macro):
    """every `#define macro(X) X(a) X(b) ...` of a file, in order"""
    text = open(os.path.join(CSRC, fname)).read()
    return [[int(v) for v in re.findall(r"X\((\d+)\)", m.group(1))]
            for m in re.finditer(r"^\s*#\s*define\s+%s\(X\)((?:\s*X\(\d+\))+)" % re.escape(macro), text, re.M)]


def _source_list(key):
    fname, name, branch = M.FAMILY_SOURCES[key]
    if branch == "switch":  # the hand-written switch of inv2d_casc3_f32
        text = open(os.path.join(CSRC, fname)).read()
        body = text[text.index("int %s(" % name):]
        body = body[body.index("switch (hlen)"):]
        body = body[:body.index("default:")]
        return sorted(int(v) for v in re.findall(r"case\s+(\d+)\s*:", body))
    lists = _lists_of(fname, name)
    if branch is None:
        assert len(lists) == 1, (key, lists)
        return lists[0]
    # lists behind #if: dwt_casc.hip (#ifdef PDWT_CASC_ONLY8, an inspection build / #else: the shipped one), swt_fused.inc (#if PART 1 or 2 /
    # #elif PART 3 / #else: parts 4 and 5 -- all five are compiled, see the swt_fused_*.hip units)
    assert len(lists) == (3 if fname == "swt_fused.inc" else 2), (key, lists)
    return lists[{"if": 0, "elif": 1, "else": -1}[branch]]


@pytest.mark.parametrize("key", sorted(M.FAMILY_LENGTHS))
def test_length_lists_equal_the_sources(key):
    assert M.FAMILY_LENGTHS[key] == _source_list(key), key


def test_no_length_list_of_the_sources_is_unknown_to_the_matrix():
    """every PDWT_*_HLENS macro defined under pdwt_amd/csrc is a key of FAMILY_SOURCES (the 3-D, boundary-mode and packet kernels have
    none: their lists are run-time loops over the tap count)"""
    known = {(f, m) for f, m, _ in M.FAMILY_SOURCES.values()}
    for path in sorted(glob.glob(os.path.join(CSRC, "*"))):
        for m in re.finditer(r"^\s*#\s*define\s+(PDWT_\w*HLENS)\(X\)", open(path, errors="replace").read(), re.M):
            assert (os.path.basename(path), m.group(1)) in known, (path, m.group(1))
    # the shipped build compiles all five parts of swt_fused.inc and does not define the inspection-build switches
    parts = sorted(int(re.search(r"PDWT_SWTF_PART (\d)", open(p).read()).group(1)) for p in glob.glob(os.path.join(CSRC, "swt_fused_*.hip"))
                   if "PDWT_SWTF_PART" in open(p).read())
    assert parts == [1, 2, 3, 4, 5]
    build_py = open(os.path.join(ROOT, "pdwt_amd", "build.py")).read()
    assert "PDWT_CASC_ONLY8" not in build_py and "PDWT_1D_HLENS" not in build_py and "PDWT_SWTF_HLENS" not in build_py


def test_rows_are_consistent():
    ids = [r["id"] for r in M.ROWS]
    assert len(set(ids)) == len(ids)
    assert len(M.ALL72) == 72 and sorted({M.hlen_of(b) for b in M.ALL72}) == list(range(2, 42, 2))
    assert len(M.PER_LENGTH) == 20 and sum(b.startswith(("bior", "rbio")) for b in M.PER_LENGTH) >= 9
    for r in M.ROWS:
        assert r["kind"] in ref2d.KINDS and r["dtypes"] and r["levels"] != r["levels2"]
        assert (r["pad_check"] is None) == (r["pad_evidence"] is None)
        for d in ("fwd", "inv"):
            for e in r["inst"][d]:
                assert e["key"] in M.FAMILY_LENGTHS and e["mapping"] in ("exact", "generic", "pad8", "pad_l2") and e["template"] in M.TEMPLATES, e
        for b in M.row_banks(r):
            h = M.hlen_of(b)
            for L in (r["levels"], r["levels2"]):
                for shape in r["shapes"](h, L):
                    assert ref2d.levels_of(shape, b, L, r["kind"]) == L, (r["id"], b, shape, L)  # the level clamp leaves L alone
                    for d in ("fwd", "inv"):
                        ran, quiet = r["evidence"](r, h, L, shape, d)
                        assert ran and not set(ran) & set(quiet), (r["id"], b, d)


def test_every_reachable_instantiation_of_every_template_is_proved_by_a_case():
    """coverage is counted per (kernel template, precision, instantiated length), not per length list (one list feeds several
    templates): the union of what the cases of the GPU module can prove equals bank_matrix.EXPECTED_REACH, which is every length of
    every list for the templates and precisions it serves, minus what no transform can reach (asserted below)"""
    reach = set()
    for r in M.ROWS:
        cases = M.row_cases(r)
        banks = {b for b, _, _ in cases}
        want = [b for b in (M.PER_LENGTH if r["banks"] == "per_length" else (r["banks"] or M.ALL72)) if r["accepts"](M.hlen_of(b))]
        assert banks == set(want) and banks, r["id"]
        for b, shape, L in cases + M.row_cases(r, r["levels2"]):
            for dt in r["dtypes"]:
                reach |= M.case_reaches(r, b, dt, shape, L)
    assert reach == M.EXPECTED_REACH, (sorted(M.EXPECTED_REACH - reach), sorted(reach - M.EXPECTED_REACH))
    # every row takes every bank of the table whose length it accepts, except the ones that say why (banks=...)
    assert [r["id"] for r in M.ROWS if r["banks"] is not None] == ["lat", "haar2d", "dwt1d_one_buffer", "dwt1d_one_buffer_inv", "haar1d"]
    # every length of every list is expected for at least one template, and the only (template, length) pairs left out of TEMPLATES are
    # the ones the gates exclude: tiled fused kernels over the LDS budget, the forward one-buffer kernel above 20 taps
    served = {}
    for r in M.ROWS:
        for entries in r["inst"].values():
            for e in entries:
                served.setdefault(e["key"], set()).add(e["template"])
    assert set(served) == set(M.FAMILY_LENGTHS)
    for key, lens in M.FAMILY_LENGTHS.items():
        for t in served[key]:
            for dname, have in M.TEMPLATES[t].items():
                missing = sorted(set(lens) - set(have))
                other_lists = set().union(*[set(M.FAMILY_LENGTHS[k2]) for k2 in served if t in served[k2]])
                assert set(have) - {0} <= other_lists, (t, dname)
                allowed = {"k_fwd2d_fused": {30, 40}, "k_inv2d_fused": {40}, "k_fwd1d_fused_ip": set(range(22, 42, 2))}.get(t, set())
                assert set(missing) <= allowed, (key, t, dname, missing)
    # and every bank is in at least one row of every transform kind in both precisions
    for b in M.ALL72:
        for kind in ref2d.KINDS:
            for dt in (M.F32, M.F64):
                assert [r["id"] for r in M.ROWS if r["kind"] == kind and dt in r["dtypes"] and b in M.row_banks(r)], (b, kind, dt.name)


def test_replayed_gates_say_what_the_rows_assume():
    # tiled fused kernels: float32 forward up to 26 taps, inverse up to 34; never in double precision
    assert [h for h in range(4, 42, 2) if M.tiled_fused_takes(h, 4, False)] == list(range(4, 28, 2))
    assert [h for h in range(4, 42, 2) if M.tiled_fused_takes(h, 4, True)] == list(range(4, 36, 2))
    assert not any(M.tiled_fused_takes(h, 8, inv) for h in range(4, 42, 2) for inv in (False, True))
    # the streamed inverse cascades decline 512 x 1024 and take the shapes of their rows; inv2d_casc_f32 takes 512 x 1024
    # (default knobs: declined; knob casc_iwaves of the two rows: taken)
    for h in M.FAMILY_LENGTHS["inv2d_casc3_f32"]:
        nr, nc = M.casc_shape("inv3", h)
        assert (nr, nc) == (max(512, 32 * h), 1024) and M.inv3_fits(nr, nc, h) is None and M.inv3_fits(nr, nc, h, M.CASC_IWAVES // 16) is not None
    for h in M.FAMILY_LENGTHS["PDWT_CASCW_INV_HLENS"]:
        nr, nc = M.casc_shape("invw", h)
        assert (nr, nc) == (max(512, 32 * h), 1024) and M.invw_fits(nr, nc, h, False) is None
        assert M.invw_fits(nr, nc, h, False, M.CASC_IWAVES // 8) is not None and (M.invw_fits(nr, nc, h, True, M.CASC_IWAVES // 8) is not None) == (h <= 12)
    assert M.ROW_BY_ID["casc_inv3"]["knobs"]["casc_iwaves"] == M.ROW_BY_ID["casc_invw"]["knobs"]["casc_iwaves"] == M.CASC_IWAVES
    for h in M.FAMILY_LENGTHS["PDWT_CASC_INV_HLENS"]:
        assert M.casc_shape("inv2", h) == (512, 1024)
    for form in ("inv3", "invw", "inv2"):
        for h in range(4, 22, 2):
            if M.ROW_BY_ID["casc_" + form]["accepts"](h):
                nr, nc = M.casc_shape(form, h)
                assert M.casc_fwd_takes(nr, nc, h) and nr % 8 == 0 and nr * nc <= 640 * 1024, (form, h, nr, nc)


# ---- the float32 bar is reachable --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def _reference(kind, wname, shape, L):
    x = M.case_input(wname, shape).astype(np.float64)
    return ref2d.forward(kind, x, wname, L)


def _oracle_f32(kind, wname, shape, L):
    O = orc.OracleWavelets(M.case_input(wname, shape), wname, L, **KIND[kind])
    assert O.info.nlevels == L
    O.forward()
    c = O.coeffs
    O.inverse()
    return c, O.get_image()


@pytest.mark.parametrize("rid", [r["id"] for r in M.ROWS if F32 in r["dtypes"]])
def test_float32_oracle_is_within_a_quarter_of_the_bar(rid):
    """every case shape of the row, both level counts: the float32 oracle against the float64 reference, every band within TOL / 4 and
    its inverse within 10 TOL / 4 of the reference inverse of its own bands (the two bounds of the GPU module, quartered)"""
    row = M.ROW_BY_ID[rid]
    worst = [0.0, 0.0]
    for wname, shape, L in M.row_cases(row) + M.row_cases(row, row["levels2"]):
        want = _reference(row["kind"], wname, shape, L)
        got, rec = _oracle_f32(row["kind"], wname, shape, L)
        assert len(got) == len(want)
        for k, (g, o) in enumerate(zip(got, want)):
            e = band_err(g, o)
            worst[0] = max(worst[0], e)
            assert e <= BAR, (rid, wname, shape, L, "band", k, e)
        e = band_err(rec, ref2d.inverse(row["kind"], got, shape, wname))
        worst[1] = max(worst[1], e)
        assert e <= 10 * BAR, (rid, wname, shape, L, "inverse", e)
    print("%s: worst forward %.2e (%.2f of TOL / 4), inverse %.2e" % (rid, worst[0], worst[0] / BAR, worst[1]))
