"""Every filter bank of the table through the three newest classes -- pdwt_amd.WaveletPackets2D (wpt2d.hip), BoundaryWavelets2D
(dwt_ext.hip / dwt_ext.hpp) and BoundaryWavelets1D (dwt_ext1d.hip / dwt_ext1d.hpp) -- in both precisions, forward and inverse,
against float64 statements of the operations: tests/refext.py and tests/refext1d.py for the boundary-mode classes and, for the packet
tree, the one-level transform of tests/ref2d.py applied to every node again (pinned to tests/refwpt.py on the CPU).  The modules
of the classes themselves run 5 to 7 of the 20 filter lengths and one short biorthogonal bank; this one runs all 72 banks -- each of
the ~230 kernel instantiations -- on shapes derived from the tile constants, the lengths either side of every 64 KiB LDS opt-in
threshold, packs of several rows for every length, and rows either side of the two LDS thresholds of the one-launch 1-D kernels.
The cases are data: tests/newer_bank_matrix.py (tied to the sources by tests/test_newer_bank_matrix_cpu.py).

What is asserted, per case and precision (TOL = 1e-5 float32, 1e-12 float64, band- or node-normalised: helpers.band_err):
  forward      every band / node against the float64 reference                                  <= TOL
  inverse      the image against the reference inverse of THE BANDS THE GPU PRODUCED            <= 10 TOL
               the image from THE REFERENCE'S bands (set_coeff / set_node / the band table)     <= 10 TOL
  round trip   the image against the input                                                      <= 10 TOL + 4 D
               D = the reconstruction defect of the float64 reference itself on that case (the table's sym* and long bior banks
               reconstruct to ~1e-11 only, in exact arithmetic)
  state        W.levels, the band and node shapes, `fused` (1-D) as the matrix predicts
  1-D          the one-launch kernels and the level drivers chained by hand give the same bits (sweep and fixed-point rows)
  impulses     one bank per length: an impulse at each corner and at the centre; nothing outside the support, exact zeros stay zero
  (the fixed-point rows of the 1-D class alone judge every band over the largest value of all bands: see newer_bank_matrix.py)
One test per bank and group of cases (376 tests); every assertion names its case and precision.  The closing test counts what ran: 72 banks x 3 classes x 2 precisions in the sweep, every other case, every (kernel family,
direction, precision, length) and both sides of each LDS threshold; 0 left out.

How far float32 arithmetic of the reference's own order sits from the float64 reference, measured on a CPU by running every case of
this module with the float32 restatement (refext / refext1d with dtype=float32, the oracle's one-level transform on float32 for the
packets) in the place of the GPU -- tests/test_newer_bank_matrix_cpu.py asserts a quarter of the float32 bounds for it -- worst band,
forward / inverse of its own bands / inverse of the reference's bands / round trip, and the largest defect D of the float64 reference:
  packets  sweep (72 banks, one level)        3.8e-7 / 4.1e-7 / 4.1e-7 / 6.9e-7   D 4.3e-11
           two levels (one bank per length)   5.6e-7 / 5.7e-7 / 6.0e-7 / 9.9e-7   D 9.5e-11
           one node of hlen x (hlen + 1)      3.6e-7 / 3.7e-7 / 4.4e-7 / 5.3e-7   D 4.2e-11
  2-D      sweep                              4.3e-7 / 5.3e-7 / 5.1e-7 / 8.0e-7   D 4.2e-11
           two levels, five modes             6.5e-7 / 5.7e-7 / 6.7e-7 / 1.1e-6   D 7.0e-11
           folded (hlen - 1) x hlen           4.7e-7 / 4.3e-7 / 4.4e-7 / 6.1e-7   D 4.3e-11
  1-D      sweep (two levels)                 3.7e-7 / 3.5e-7 / 3.5e-7 / 6.9e-7   D 4.0e-11
           three levels, five modes           4.7e-7 / 3.4e-7 / 4.5e-7 / 6.1e-7   D 4.4e-11
           opt-in rows / edge rows            4.2e-7 / 5.2e-7 / 4.3e-7 / 7.6e-7   D 4.4e-11
           fixed point (common scale)         5.8e-7 / 2.9e-7 / 3.3e-7 / 7.0e-7   D 4.7e-11
The worst forward figure is a factor 15 inside its bar of 1e-5 and a factor 3.8 inside the quarter bar; the worst round trip is a factor
90 inside 1e-4.  In float64 4 D (at most 3.8e-10) is what decides the round-trip bound for the sym* and long bior banks.
"""
import ctypes as C

import numpy as np
import pytest

import pdwt_amd
from pdwt_amd import BoundaryWavelets1D, BoundaryWavelets2D, WaveletPackets2D
from pdwt_amd import _native as nat
from pdwt_amd.wavelets import W_INIT
from tests import newer_bank_matrix as M

pytestmark = pytest.mark.gpu

F32, F64 = M.F32, M.F64
DONE = set()    # (case id, precision) of every case that ran to the end of its checks
REACHED = set()  # (kernel family, direction, precision, length)
WORST = {}


def _noter(case, dt):
    key = (case["cls"], case["group"], dt.name)

    def note(what, val):
        WORST.setdefault(key, {})
        WORST[key][what] = max(WORST[key].get(what, 0.0), float(val))
    return note


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


class _Dev:
    """a few device buffers of the library's allocator, freed by free()"""

    def __init__(self):
        self.L, self.ptrs = pdwt_amd.hip(), []

    def put(self, arr):
        a = np.ascontiguousarray(arr)
        p = self.L.pdwt_malloc(a.nbytes)
        assert p
        self.ptrs.append(p)
        assert self.L.pdwt_memcpy_h2d(p, a.ctypes.data, a.nbytes) == 0
        return p

    def nan(self, shape, dt):
        return self.put(np.full(shape, np.nan, dt))

    def get(self, p, shape, dt):
        out = np.empty(shape, dt)
        assert self.L.pdwt_sync() == 0 and self.L.pdwt_memcpy_d2h(out.ctypes.data, p, out.nbytes) == 0
        return out

    def free(self):
        self.L.pdwt_sync()
        for p in self.ptrs:
            self.L.pdwt_free(p)
        self.ptrs = []


def _bank(wname, dt):
    L = pdwt_amd.hip()
    sfx = "f32" if np.dtype(dt) == np.float32 else "f64"
    f = (nat.Filters32 if sfx == "f32" else nat.Filters64)()
    h = getattr(L, "pdwt_compute_filters_separable_" + sfx)(wname.encode(), 0, C.byref(f))
    assert h == M.hlen_of(wname)
    f.hlen = h
    return L, sfx, f


# ---- the GPU backends of newer_bank_matrix.check ------------------------------------------------------------------------------------------
class PacketsClass:
    def __init__(self, case, x):
        self.case, self.x, L = case, x, case["levels"]
        self.W = W = WaveletPackets2D(x, case["wname"], L)
        assert W.state == W_INIT and W.dtype == x.dtype and W.levels == L and W.shape == case["shape"], (case["id"], W.state, W.levels)
        shapes = M.band_shapes(case)
        assert [W.node_shape(d) for d in range(1, L + 1) for _ in range(4 ** d)] == shapes

    def forward(self):
        self.W.forward()
        return [n for d in range(1, self.case["levels"] + 1) for n in self.W.get_level(d)]

    def inverse_own(self):
        self.W.inverse()
        return self.W.get_image()

    def inverse_of(self, bands):
        W, L = self.W, self.case["levels"]
        W.set_image(np.zeros(self.case["shape"], self.x.dtype))  # the image must come from the nodes, not from what it still held
        W.forward()
        for i, b in enumerate(bands[len(bands) - 4 ** L:]):
            W.set_node((L, i), b)
        W.inverse()
        return W.get_image()

    def close(self):
        self.W.close()


class PacketsDrivers:
    """one parent node through pdwt_wpt2d_forward_level_* / pdwt_wpt2d_inverse_level_* (all parents: no node list)"""

    def __init__(self, case, x):
        self.case, self.x, self.D = case, x, _Dev()
        self.L, self.sfx, self.f = _bank(case["wname"], x.dtype)
        self.cshape = M.band_shapes(case)[0]

    def forward(self):
        D, dt, (nr, nc) = self.D, self.x.dtype, self.case["shape"]
        src, child = D.put(self.x), D.nan((4,) + self.cshape, dt)
        assert getattr(self.L, "pdwt_wpt2d_forward_level_" + self.sfx)(src, child, nr, nc, None, 1, C.byref(self.f)) == 0
        self.got = list(D.get(child, (4,) + self.cshape, dt))
        assert _same_bits(D.get(src, (nr, nc), dt), self.x)
        return self.got

    def inverse_of(self, bands):
        D, dt, (nr, nc) = self.D, self.x.dtype, self.case["shape"]
        child, dst = D.put(np.stack(bands)), D.nan((nr, nc), dt)
        assert getattr(self.L, "pdwt_wpt2d_inverse_level_" + self.sfx)(dst, child, nr, nc, None, 1, C.byref(self.f)) == 0
        return D.get(dst, (nr, nc), dt)

    def inverse_own(self):
        return self.inverse_of(self.got)

    def close(self):
        self.D.free()


class Boundary2DClass:
    cls = BoundaryWavelets2D

    def __init__(self, case, x):
        self.case, self.x, L = case, x, case["levels"]
        self.W = W = self.cls(x, case["wname"], L, case["mode"])
        assert W.state == W_INIT and W.dtype == x.dtype and W.levels == L and W.mode == case["mode"] and W.nbands == len(M.band_shapes(case)), (case["id"], W.state, W.levels)
        assert [W.coeff_shape(k) for k in range(W.nbands)] == M.band_shapes(case)

    def forward(self):
        self.W.forward()
        return self.W.coeffs

    def inverse_own(self):
        self.W.inverse()
        return self.W.get_image()

    def inverse_of(self, bands):
        W = self.W
        W.set_image(np.zeros(self.case["shape"], self.x.dtype))
        assert W.state == W_INIT
        for k, b in enumerate(bands):
            W.set_coeff(b, k)
        W.inverse()
        return W.get_image()

    def close(self):
        self.W.close()


class Boundary2DDrivers(PacketsDrivers):
    """one level through pdwt_ext2d_forward_level_* / pdwt_ext2d_inverse_level_*"""

    def forward(self):
        D, dt, (nr, nc) = self.D, self.x.dtype, self.case["shape"]
        src, b = D.put(self.x), [D.nan(self.cshape, dt) for _ in range(4)]
        assert getattr(self.L, "pdwt_ext2d_forward_level_" + self.sfx)(src, b[0], b[1], b[2], b[3], nr, nc, M.MODES.index(self.case["mode"]), C.byref(self.f)) == 0
        self.got = [D.get(p, self.cshape, dt) for p in b]
        return self.got

    def inverse_of(self, bands):
        D, dt, (nr, nc) = self.D, self.x.dtype, self.case["shape"]
        b, dst = [D.put(v) for v in bands], D.nan((nr, nc), dt)
        assert getattr(self.L, "pdwt_ext2d_inverse_level_" + self.sfx)(dst, b[0], b[1], b[2], b[3], nr, nc, C.byref(self.f)) == 0
        return D.get(dst, (nr, nc), dt)


def _chain_forward(D, L, sfx, f, x, h, levels, mode):
    """[A_L, D_1, ..., D_L] by chaining pdwt_ext1d_forward_level_* by hand"""
    dt, (nr, n) = x.dtype, x.shape
    src, det = D.put(x), []
    for _ in range(levels):
        N = (n + h - 1) // 2
        a, d = D.nan((nr, N), dt), D.nan((nr, N), dt)
        assert getattr(L, "pdwt_ext1d_forward_level_" + sfx)(src, a, d, nr, n, M.MODES.index(mode), C.byref(f)) == 0
        det.append(D.get(d, (nr, N), dt))
        src, n = a, N
    return [D.get(src, (nr, n), dt)] + det


def _chain_inverse(D, L, sfx, f, bands, n0, h):
    dt, levels, nr = bands[0].dtype, len(bands) - 1, bands[0].shape[0]
    lens = M.R1.level_lens(n0, h, levels)
    a = D.put(bands[0])
    for l in range(levels, 0, -1):
        out = D.nan((nr, lens[l - 1]), dt)
        assert getattr(L, "pdwt_ext1d_inverse_level_" + sfx)(out, a, D.put(bands[l]), nr, lens[l - 1], C.byref(f)) == 0
        a = out
    return D.get(a, (nr, n0), dt)


class Boundary1DClass(Boundary2DClass):
    """the class; on the sweep also the level drivers chained by hand, which must give the same bits as the one launch"""
    cls = BoundaryWavelets1D

    def __init__(self, case, x):
        Boundary2DClass.__init__(self, case, x)
        assert self.W.fused == M.case_fused(case, x.dtype), (case["id"], self.W.fused)
        self.chain = case["group"] == "sweep"
        if self.chain:
            assert self.W.fused
            self.D = _Dev()
            self.L, self.sfx, self.f = _bank(case["wname"], x.dtype)

    def forward(self):
        got = Boundary2DClass.forward(self)
        if self.chain:
            c = self.case
            for k, (a, b) in enumerate(zip(got, _chain_forward(self.D, self.L, self.sfx, self.f, self.x, c["hlen"], c["levels"], c["mode"]))):
                assert _same_bits(a, b), (c["id"], "one launch against the level drivers, band", k)
        self.got = got
        return got

    def inverse_own(self):
        rec = Boundary2DClass.inverse_own(self)
        if self.chain:
            assert _same_bits(rec, _chain_inverse(self.D, self.L, self.sfx, self.f, self.got, self.case["shape"][1], self.case["hlen"])), self.case["id"]
        return rec

    def close(self):
        if self.chain:
            self.D.free()
        self.W.close()


class Boundary1DCabi(PacketsDrivers):
    """the whole-transform entries pdwt_ext1d_forward_* / pdwt_ext1d_inverse_* on a band table of the caller (the rows the class
    clamps away), bit for bit against the level drivers chained by hand"""

    def __init__(self, case, x):
        PacketsDrivers.__init__(self, case, x)
        h, (nr, nc), lv, es = case["hlen"], case["shape"], case["levels"], x.dtype.itemsize
        assert self.L.pdwt_ext1d_fused(nc, h, lv, es) == 1 == int(M.case_fused(case, x.dtype)) and self.L.pdwt_ext1d_tmp_elems(nr, nc, h, lv, es) == 0
        self.shapes = M.band_shapes(case)

    def _table(self, ptrs):
        return (C.c_void_p * len(ptrs))(*ptrs)

    def forward(self):
        D, dt, c, (nr, nc) = self.D, self.x.dtype, self.case, self.case["shape"]
        src, b = D.put(self.x), [D.nan(s, dt) for s in self.shapes]
        rc = getattr(self.L, "pdwt_ext1d_forward_" + self.sfx)(src, self._table(b), nr, nc, c["levels"], M.MODES.index(c["mode"]), C.byref(self.f), None)
        assert rc == 1, rc  # PDWT_EXT1D_FUSED
        self.got = [D.get(p, s, dt) for p, s in zip(b, self.shapes)]
        for k, (a, o) in enumerate(zip(self.got, _chain_forward(D, self.L, self.sfx, self.f, self.x, c["hlen"], c["levels"], c["mode"]))):
            assert _same_bits(a, o), (c["id"], "one launch against the level drivers, band", k)
        return self.got

    def inverse_of(self, bands):
        D, dt, c, (nr, nc) = self.D, self.x.dtype, self.case, self.case["shape"]
        b, dst = [D.put(v) for v in bands], D.nan((nr, nc), dt)
        assert getattr(self.L, "pdwt_ext1d_inverse_" + self.sfx)(dst, self._table(b), nr, nc, c["levels"], C.byref(self.f), None) == 1
        rec = D.get(dst, (nr, nc), dt)
        assert _same_bits(rec, _chain_inverse(D, self.L, self.sfx, self.f, bands, nc, c["hlen"])), c["id"]
        return rec


BACKENDS = {("wpt", "class"): PacketsClass, ("wpt", "drivers"): PacketsDrivers, ("ext2d", "class"): Boundary2DClass,
            ("ext2d", "drivers"): Boundary2DDrivers, ("ext1d", "class"): Boundary1DClass, ("ext1d", "cabi"): Boundary1DCabi}


def backend(case, x):
    return BACKENDS[(case["cls"], case["via"])](case, x)


def run(case, dt):
    M.check(case, dt, backend, M.TOL[dt], _noter(case, dt))
    DONE.add((case["id"], dt.name))
    REACHED.update(M.case_reaches(case, dt))


def _banks(*groups):
    """the banks of the groups, in table order: one test per bank, short ids (the case and the precision are named by every assertion)"""
    have = {c["wname"] for g in groups for c in g}
    return [w for w in M.ALL72 if w in have]


def _run_bank(wname, *groups):
    """every case of the bank in the groups, the precision innermost: the two precisions of a case share one float64 reference"""
    n = 0
    for g in groups:
        for c in g:
            if c["wname"] == wname:
                for d in c["dtypes"]:
                    run(c, d)
                    n += 1
    assert n


# ---- 1. every bank, the sweep ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wname", M.ALL72)
def test_packets_every_bank(wname):
    _run_bank(wname, M.WP_SWEEP)


@pytest.mark.parametrize("wname", M.ALL72)
def test_boundary_2d_every_bank(wname):
    _run_bank(wname, M.E2_SWEEP)


@pytest.mark.parametrize("wname", M.ALL72)
def test_boundary_1d_every_bank_one_launch_and_level_drivers(wname):
    _run_bank(wname, M.E1_SWEEP)


# ---- 2. one bank per length ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wname", _banks(M.WP_TWO, M.WP_NODE))
def test_packets_two_levels_and_a_node_as_small_as_the_bank(wname):
    _run_bank(wname, M.WP_TWO, M.WP_NODE)


@pytest.mark.parametrize("wname", _banks(M.E2_TWO, M.E2_FOLD))
def test_boundary_2d_every_mode_two_levels_and_a_folded_image(wname):
    _run_bank(wname, M.E2_TWO, M.E2_FOLD)


@pytest.mark.parametrize("wname", _banks(M.E1_MODES))
def test_boundary_1d_every_mode_three_levels(wname):
    _run_bank(wname, M.E1_MODES)


@pytest.mark.parametrize("wname", _banks(M.E1_OPTIN, M.E1_EDGE))
def test_boundary_1d_rows_either_side_of_the_lds_thresholds(wname):
    """opt-in: both one-launch kernels above 64 KiB; edge: the longest row of one launch, and one sample more (per level)"""
    _run_bank(wname, M.E1_OPTIN, M.E1_EDGE)


@pytest.mark.parametrize("wname", _banks(M.E1_FIXED))
def test_boundary_1d_fixed_point_rows_through_the_c_abi(wname):
    _run_bank(wname, M.E1_FIXED)


IMPULSE_GROUPS = {"wpt": M.WP_TWO, "ext2d": M.E2_TWO, "ext1d": M.E1_MODES}
assert sum(len(g) for g in IMPULSE_GROUPS.values()) == len(M.IMPULSE_CASES)


@pytest.mark.parametrize("wname", M.PER_LENGTH)
@pytest.mark.parametrize("cls", sorted(IMPULSE_GROUPS))
def test_impulses_at_the_corners_and_the_centre(cls, wname):
    for case in IMPULSE_GROUPS[cls]:
        if case["wname"] == wname:
            for dt in case["dtypes"]:
                M.check_impulses(case, dt, backend, M.TOL[dt], _noter(dict(case, group="impulses"), dt))
                DONE.add(("impulses-" + case["id"], dt.name))


# ---- the closing count -----------------------------------------------------------------------------------------------------------------
def test_no_case_was_left_out():
    """a condition, not a measurement: every case ran to the end of its checks in every precision it has, and with them every kernel
    family, direction, precision and filter length 2 .. 40 and both sides of every LDS threshold.  It counts what the tests above
    recorded in this process, so it holds for a run of the whole module only."""
    for key in sorted(WORST):
        print("worst %-6s %-12s %-8s" % key, "  ".join("%s %.2e" % kv for kv in sorted(WORST[key].items())))
    sweep = {(c["id"], d.name) for cases in M.SWEEPS.values() for c in cases for d in c["dtypes"]}
    assert len(sweep) == 72 * 3 * 2 and sweep <= DONE, sorted(sweep - DONE)
    want = {(c["id"], d.name) for c in M.CASES for d in c["dtypes"]} | {("impulses-" + c["id"], d.name) for c in M.IMPULSE_CASES for d in c["dtypes"]}
    left_out = sorted(want - DONE)
    uncovered = sorted(M.EXPECTED_REACH - REACHED)
    print("%d cases ran, %d left out; %d (family, direction, precision, length) reached, %d uncovered" % (len(DONE), len(left_out), len(REACHED), len(uncovered)))
    assert not left_out and DONE == want, left_out
    assert not uncovered and REACHED == M.EXPECTED_REACH, uncovered
    cross = M.lds_crossings()
    sides = M.lds_sides(REACHED)
    assert cross
    for key, h in sorted(cross.items()):
        below, above = sides[key]
        assert h - 2 in below and h in above, (key, h, below, above)
        print("LDS opt-in of %s %s %s: from %d taps; ran %d lengths below and %d above" % (key + (h, len(below), len(above))))
    for t in M.DTYPES:  # the one-launch 1-D kernels: rows on both sides of 64 KiB and of the 160 KiB ceiling
        assert sum((c["id"], t.name) in DONE for c in M.E1_OPTIN + M.E1_EDGE if t in c["dtypes"]) == 20 * 3
