"""Every filter bank of the table through every kernel family of ``pdwt_amd.Wavelets`` (2-D DWT, batched 1-D DWT, 2-D / 1-D SWT,
float32 and float64) against the float64 direct-sum reference tests/ref2d.py (pinned on the CPU by tests/test_ref2d_cpu.py), with
proof of which kernel ran.  The matrix -- one row per kernel family: knobs, accepted lengths, shape rule, launch evidence -- is
tests/bank_matrix.py; tests/test_bank_matrix_cpu.py ties it to the X-macro lists of the sources.  The rest of the suite compares a
few banks per family with the oracle in the same precision (equality with a restatement of the same arithmetic); this module asserts
accuracy against a high-precision statement of the operation for all 72 banks, the biorthogonal ones included, where synthesis taps
are not the time-reversed analysis taps.

Per (row, bank, precision), for every shape of the row, under the row's knobs with pdwt_ktime_enable(1)
(TOL = 1e-5 float32, 1e-12 float64; band-normalised, helpers.band_err; input uniform(-100, 100) rounded to float32, one seed per bank):
  forward      every band against the reference <= TOL; forward() leaves the image bit-unchanged
  inverse      the image against the reference inverse of THE BANDS THE GPU PRODUCED <= 10 TOL
  from ref     one more inverse from the reference's coefficients (cast to the precision, written with set_coeff) against the
               reference's own reconstruction <= 10 TOL  (the cast moves a float32 band by 6e-8 of its scale: 1 / 1600 of that bound)
  round trip   <= 10 TOL + 4 D, D = the reconstruction defect of the float64 reference itself on that input
  evidence     the row's kernels / stat_* counters show a launch in the direction tested, the ones it excludes none; a family that
               declined fails the case
  padding      rows whose banks run a longer zero-padded instantiation: once more under the knob that sends them to kernels taking
               the bank at its own length (f64_lds = 3: tiled / two-pass; swtf_long = 0: two-pass SWT), launch evidence of that,
               bands bit-identical, the reconstruction bit-identical (decimated) or within 10 TOL (SWT: another summation order)
One bank per length (bank_matrix.PER_LENGTH, biorthogonal where there is one) also runs the row's second level count and an image of
five impulses (the four corners and the centre): nothing outside the support of the bands (ref2d.support), exactly.  The closing test counts the cases.

How far the arithmetic the kernels restate (the oracle, in the precision under test) sits from this reference: measured on a CPU by
running every case of this module with the oracle in the place of the GPU class (``check(..., cls=OracleWavelets)``), worst case per
group -- forward / inverse of its own bands / inverse of the reference's bands / round trip:
  decimated 2-D   float32 5.4e-7 / 6.1e-7 / 6.5e-7 / 9.9e-7      float64 8.4e-16 / 8.5e-16 / 8.5e-16 / D
  batched 1-D     float32 5.3e-7 / 4.1e-7 / 3.8e-7 / 6.9e-7      float64 8.9e-16 / 8.5e-16 / 8.5e-16 / D
  stationary 2-D  float32 6.3e-7 / 6.4e-7 / 5.7e-7 / 7.6e-7      float64 1.1e-15 / 1.1e-15 / 1.0e-15 / D
  stationary 1-D  float32 5.3e-7 / 4.3e-7 / 3.8e-7 / 5.3e-7      float64 1.2e-15 / 1.0e-15 / 8.6e-16 / D
  Haar            float32 1.2e-7 / 1.1e-7 / 1.6e-7 / 1.6e-7      float64 6.2e-16 / 5.8e-16 / 7.1e-16 / 5.8e-16
The worst float32 figure is a factor 15 inside its bar (forward) and every float64 one a factor 800; tests/test_bank_matrix_cpu.py
asserts a quarter of the float32 bar for every case.  The reference's own reconstruction defect D (the table's sym* and some bior
banks do not reconstruct exactly) reaches 7.6e-11 in the decimated 2-D cases, 4.8e-11 in the 1-D ones and 8.3e-11 in the stationary
ones (sym20 in each); the float64 round trips above are that defect.

On an MI355X the worst figures of the module are, in the same order (the forward kernels restate the oracle's sums, most of them bit
for bit, so the forward column is the oracle's):
  decimated 2-D   float32 5.4e-7 / 6.1e-7 / 6.5e-7 / 9.9e-7      float64 9.5e-16 / 1.1e-15 / 1.0e-15 / D  (the lattice kernels of db20)
  batched 1-D     float32 5.3e-7 / 4.1e-7 / 3.8e-7 / 6.9e-7      float64 8.9e-16 / 8.5e-16 / 8.5e-16 / D
  stationary 2-D  float32 6.3e-7 / 5.8e-7 / 6.1e-7 / 6.9e-7      float64 1.1e-15 / 8.5e-16 / 1.1e-15 / D
  stationary 1-D  float32 5.3e-7 / 3.9e-7 / 4.2e-7 / 5.3e-7      float64 1.2e-15 / 1.0e-15 / 8.5e-16 / D
Wall time there: 15 s for the 1989 tests of this module (the slowest case 0.25 s, the cascade cases 0.05 - 0.08 s), against 48 s for
the 304 tests of tests/test_gpu_parity.py in the same visit (both on this tree: its only product change are the launch counters).
"""
import ctypes as C
import functools
import time

import numpy as np
import pytest

import pdwt_amd
from pdwt_amd import W_CREATION_ERROR, W_FORWARD, W_INVERSE
from pdwt_amd.wavelets import W_FORWARD_ERROR, W_INVERSE_ERROR
from tests import bank_matrix as M
from tests import ref2d
from tests.helpers import KIND, band_err, knobs

pytestmark = pytest.mark.gpu

F32, F64 = M.F32, M.F64
TOL = {F32: 1e-5, F64: 1e-12}
T0 = time.time()

# what ran, for the closing test
DONE = {"sweep": set(), "levels2": set(), "impulses": set()}  # (row, bank, dtype)
REACHED = set()  # (kernel template, precision, instantiated length) that a passed case proved to have run: bank_matrix.case_reaches
WORST = {}


def _note(rid, dt, what, val):
    key = (rid, dt.name)
    WORST.setdefault(key, {})
    WORST[key][what] = max(WORST[key].get(what, 0.0), float(val))


# ---- launch evidence -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _kernel_ids():
    L = pdwt_amd.hip()
    L.pdwt_kernel_name.restype = C.c_char_p
    return {L.pdwt_kernel_name(i).decode(): i for i in range(L.pdwt_kernel_count())}


def _count(name):
    """launches so far: a timer name (since the last pdwt_ktime_reset) or a stat_* counter (since the process started)"""
    L = pdwt_amd.hip()
    v = C.c_int()
    if name.startswith("stat_"):
        assert L.pdwt_debug_get(name.encode(), C.byref(v)) == 0, name
    else:
        assert L.pdwt_ktime_read(_kernel_ids()[name], C.byref(v), None) == 0, name
    return v.value


class launches:
    """with launches(ran, quiet, dt, what): ...  -- the kernels of `ran` each show a launch inside the block, those of `quiet` none"""

    def __init__(self, ran, quiet, dt, what):
        self.ran, self.quiet, self.what = M.resolve(ran, dt), M.resolve(quiet, dt), what

    def __enter__(self):
        pdwt_amd.hip().pdwt_ktime_reset()
        self.before = {n: _count(n) for n in self.ran + self.quiet if n.startswith("stat_")}
        return self

    def __exit__(self, et, ev, tb):
        if et is None:
            got = {n: _count(n) - self.before.get(n, 0) for n in self.ran + self.quiet}
            assert all(got[n] >= 1 for n in self.ran) and not any(got[n] for n in self.quiet), (self.what, "ran", self.ran, "quiet", self.quiet, got)
        return False


class no_evidence:
    def __init__(self, *a):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


# ---- the reference side ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def reference(kind, wname, shape, L, impulses=False):
    """(input as float32, float64 bands, float64 reconstruction of those bands, its defect D, for impulses the support of the bands):
    once per (bank, kind, shape, levels)"""
    x = impulse_image(shape) if impulses else M.case_input(wname, shape)
    want = ref2d.forward(kind, x, wname, L)
    rec = ref2d.inverse(kind, want, shape, wname)
    return x, want, rec, band_err(rec, x), (ref2d.support(kind, x, wname, L) if impulses else None)


def impulse_image(shape):
    """five impulses of different heights: the four corners and the centre (rows of a 1-D batch: the two ends and the centre)"""
    x = np.zeros(shape, np.float32)
    nr, nc = shape
    for (r, c), v in zip([(0, 0), (0, nc - 1), (nr - 1, 0), (nr - 1, nc - 1), (nr // 2, nc // 2)], (100.0, -50.0, 25.0, 75.0, -100.0)):
        x[r, c] = v
    return x


def _ran(W, state, where):
    """a driver that returned an error code (a launch or the device failed) ends the session: nothing more is launched on a device
    that may have faulted, and the case is reported"""
    if W.state in (W_FORWARD_ERROR, W_INVERSE_ERROR):
        pytest.exit("device error in %r: %s" % (where, (pdwt_amd.hip().pdwt_last_error_string() or b"").decode()), returncode=3)
    assert W.state == state, where


def check(row, wname, dt, shape, L, group, impulses=False, cls=None):
    """all the assertions of one case; cls: a stand-in with the class's interface (the oracle, on a CPU) -- no launch evidence then"""
    gpu = cls is None
    cls = cls or pdwt_amd.Wavelets
    watch = launches if gpu else no_evidence
    kind, rid, h = row["kind"], row["id"], M.hlen_of(wname)
    x32, want, rec_ref, defect, sup = reference(kind, wname, tuple(shape), L, impulses)
    x = x32.astype(dt)
    where = (rid, wname, dt.name, tuple(shape), L, group)
    with knobs(**(row["knobs"] if gpu else {})):
        if gpu:
            pdwt_amd.hip().pdwt_ktime_enable(1)
        try:
            W = cls(x, wname, L, dtype=dt, **KIND[kind])
            assert W.state != W_CREATION_ERROR and W.info.nlevels == L, where
            with watch(*row["evidence"](row, h, L, shape, "fwd"), dt, where + ("forward",)):
                W.forward()
            _ran(W, W_FORWARD, where)
            assert np.array_equal(W.get_image(), x), where + ("forward() changed the image",)
            got = W.coeffs
            assert len(got) == len(want), where
            for k, (g, o) in enumerate(zip(got, want)):
                assert g.dtype == dt and g.shape == o.shape, where + (k, g.shape, o.shape)
                e = band_err(g, o)
                _note(rid, dt, "forward", e)
                assert e <= TOL[dt], where + ("band", k, e)
                if impulses:  # a sum of products with zeros is zero in any precision: nothing may leak outside the support
                    assert not np.any(o[sup[k] == 0]) and (sup[k] == 0).any() and not np.any(g[sup[k] == 0]), where + ("band", k, "non-zero outside the support")
            with watch(*row["evidence"](row, h, L, shape, "inv"), dt, where + ("inverse",)):
                W.inverse()
            _ran(W, W_INVERSE, where)
            rec = W.get_image()
            e_inv = band_err(rec, ref2d.inverse(kind, got, shape, wname))
            e_rt = band_err(rec, x)
            _note(rid, dt, "inverse", e_inv)
            _note(rid, dt, "round trip", e_rt)
            _note(rid, dt, "defect D", defect)
            assert e_inv <= 10 * TOL[dt], where + ("inverse", e_inv)
            # 4 D and not D: D is itself a rounded figure and the kernel's own rounding adds to the defect (tests/test_3d_all_banks_gpu.py)
            assert e_rt <= 10 * TOL[dt] + 4 * defect, where + ("round trip", e_rt, defect)
            # the synthesis on its own, from coefficients the analysis kernels never saw
            W.forward()
            for k, o in enumerate(want):
                W.set_coeff(o.astype(dt), k)
            with watch(*row["evidence"](row, h, L, shape, "inv"), dt, where + ("inverse of the reference's bands",)):
                W.inverse()
            _ran(W, W_INVERSE, where)
            e_ref = band_err(W.get_image(), rec_ref)
            _note(rid, dt, "inverse of ref bands", e_ref)
            assert e_ref <= 10 * TOL[dt], where + ("inverse of the reference's bands", e_ref)
            if hasattr(W, "close"):
                W.close()
            # padded instantiations against the kernels that take the bank at its own length
            if gpu and row["pad_check"] and not impulses and any(M.instantiation(e["key"], e["mapping"], h) != h for e in row["inst"]["fwd"]):
                with knobs(**{row["pad_check"][0]: row["pad_check"][1]}):
                    W = cls(x, wname, L, dtype=dt, **KIND[kind])
                    with watch(*row["pad_evidence"](row, h, dt, "fwd"), dt, where + ("forward, other kernels",)):
                        W.forward()
                    _ran(W, W_FORWARD, where)
                    for k, g in enumerate(got):
                        assert np.array_equal(W.get_coeff(k), g), where + ("band", k, "padded and exact-length kernels differ")
                    with watch(*row["pad_evidence"](row, h, dt, "inv"), dt, where + ("inverse, other kernels",)):
                        W.inverse()
                    _ran(W, W_INVERSE, where)
                    if kind == "dwt2":  # the same sums in the same order
                        assert np.array_equal(W.get_image(), rec), where + ("inverse: padded and exact-length kernels differ",)
                    else:  # (the fused SWT inverse sums rows before columns, the two-pass one columns first: to rounding)
                        assert band_err(W.get_image(), rec) <= 10 * TOL[dt], where + ("inverse: padded and two-pass kernels", band_err(W.get_image(), rec))
                    W.close()
        finally:
            if gpu:
                pdwt_amd.hip().pdwt_ktime_enable(0)
    if gpu:  # (every assertion of the case held, its launch evidence included)
        REACHED.update(M.case_reaches(row, wname, dt, shape, L))


# ---- 1. every bank through every row that accepts it ---------------------------------------------------------------------------------
SWEEP = [(r["id"], b, d) for r in M.ROWS for b in M.row_banks(r) for d in r["dtypes"]]  # (row, bank) outermost, the precision innermost


@pytest.mark.parametrize("rid,wname,dt", SWEEP, ids=["%s-%s-%s" % (r, b, d.name) for r, b, d in SWEEP])
def test_every_bank_in_every_family(rid, wname, dt):
    row = M.ROW_BY_ID[rid]
    for shape in row["shapes"](M.hlen_of(wname), row["levels"]):
        check(row, wname, dt, shape, row["levels"], "sweep")
    DONE["sweep"].add((rid, wname, dt.name))


# ---- 2. one bank per length: a second level count, and impulses ------------------------------------------------------------------------
EXTRA = [(r["id"], b, d) for r in M.ROWS for b in M.row_banks(r) if b in M.PER_LENGTH for d in r["dtypes"]]


@pytest.mark.parametrize("rid,wname,dt", EXTRA, ids=["%s-%s-%s" % (r, b, d.name) for r, b, d in EXTRA])
def test_second_level_count_one_bank_per_length(rid, wname, dt):
    row = M.ROW_BY_ID[rid]
    for shape in row["shapes"](M.hlen_of(wname), row["levels2"]):
        check(row, wname, dt, shape, row["levels2"], "levels2")
    DONE["levels2"].add((rid, wname, dt.name))


@pytest.mark.parametrize("rid,wname,dt", EXTRA, ids=["%s-%s-%s" % (r, b, d.name) for r, b, d in EXTRA])
def test_impulses_at_the_corners_and_the_centre(rid, wname, dt):
    """a max-normalised error on noise says little about WHERE an error sits; impulses have an exactly known answer -- products of taps
    at the wrapped positions -- and exact zeros everywhere else"""
    row = M.ROW_BY_ID[rid]
    for shape in row["shapes"](M.hlen_of(wname), row["levels"]):
        check(row, wname, dt, shape, row["levels"], "impulses", impulses=True)
    DONE["impulses"].add((rid, wname, dt.name))


# ---- the closing count -----------------------------------------------------------------------------------------------------------------
def test_no_case_was_left_out():
    """a condition, not a measurement: every instantiation of every kernel template that a transform can reach (bank_matrix.TEMPLATES:
    per template and precision, not per shared length list) ran in a case that passed and whose launch evidence proves it, every bank
    ran in every row that accepts it, nothing was skipped.  It counts what the tests above recorded in this process, so it holds for a run of the
    whole module only."""
    for key in sorted(WORST):
        print("worst %-18s %-8s" % key, "  ".join("%s %.2e" % kv for kv in sorted(WORST[key].items())))
    print("wall time of the module so far: %.0f s, %d + %d + %d cases" % (time.time() - T0, len(SWEEP), len(EXTRA), len(EXTRA)))
    want = {(r, b, d.name) for r, b, d in SWEEP}
    assert DONE["sweep"] == want, sorted(want - DONE["sweep"])
    want = {(r, b, d.name) for r, b, d in EXTRA}
    assert DONE["levels2"] == want, sorted(want - DONE["levels2"])
    assert DONE["impulses"] == want, sorted(want - DONE["impulses"])
    uncovered = sorted(M.EXPECTED_REACH - REACHED)  # (kernel template, precision, instantiated length), proved by launch evidence
    assert not uncovered, uncovered
    left_out = [(r["id"], b) for r in M.ROWS if r["banks"] is None for b in M.ALL72
                if r["accepts"](M.hlen_of(b)) and not all((r["id"], b, d.name) in DONE["sweep"] for d in r["dtypes"])]
    assert not left_out, left_out
    for b in M.ALL72:  # every bank, every kind of transform, both precisions
        for kind in ref2d.KINDS:
            for d in (F32, F64):
                assert any(M.ROW_BY_ID[r]["kind"] == kind for r, bb, dn in DONE["sweep"] if bb == b and dn == d.name), (b, kind, d.name)
    print("0 uncovered (template, precision, length) triples of %d, 0 banks left out" % len(M.EXPECTED_REACH))
