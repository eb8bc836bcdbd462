"""The cases of tests/test_newer_all_banks_gpu.py as plain data, importable without a GPU: every filter bank of the table through the
three newest classes -- ``WaveletPackets2D`` (wpt2d.hip), ``BoundaryWavelets2D`` (dwt_ext.hip / dwt_ext.hpp) and ``BoundaryWavelets1D``
(dwt_ext1d.hip / dwt_ext1d.hpp) -- against float64 statements of the operations.  tests/test_newer_bank_matrix_cpu.py ties the
constants below to the sources, checks that the cases reach every (kernel family, direction, precision, filter length) and both sides
of every 64 KiB LDS opt-in threshold, and runs every case with the float32 restatement of the reference in the place of the GPU.

The kernels are instantiated once per even length 2 .. 40 (``with_filter_length``), so the dispatch of a case is decided by the bank
length alone; what differs between the cases of one length is the geometry, and every shape here is DERIVED from the tile constants
of the sources (one Python copy below, compared with the sources on the CPU) and the bank length:

  packets   sweep       all 72 banks, 1 level, (max(2 WIY + 3, 2 hlen - 1), 2 WIX + 4): odd rows, even columns, more than one inverse
                        tile per axis with a partial last one, more than one forward tile per axis
            two levels  one bank per length, even rows and odd columns, four parents in blockIdx.z at the second level, every
                        level with more than one tile per axis
            one node    one bank per length, a node of exactly hlen x (hlen + 1) through the level drivers: the window of the only
                        tile wraps on both sides of both axes
  2-D       sweep       all 72 banks, 1 level, mode = bank index mod 5; the forward tile (ky, kx) is the first whose window starts
                        inside the image and the shape is the smallest odd one that holds it with border tiles on all four sides
            two levels  one bank per length, all five modes, odd rows and even columns
            folded      one bank per length, all five modes, the image (hlen - 1) x hlen through the level drivers: the halo of
                        hlen - 2 samples folds the whole line
  1-D       sweep       all 72 banks, 2 levels, Nc = 4 (hlen - 1) + 37, Nr = 2 R + 1 (two full packs of R rows and a partial one),
                        mode = bank index mod 5; through the class (one launch) and through the level drivers chained by hand
            modes       one bank per length, all five modes, 3 levels, odd Nc
            opt-in      one bank per length and precision: 2 rows of the smallest Nc whose one-launch kernels BOTH need more than
                        64 KiB of LDS, plus 3
            edge        one bank per length and precision: 2 rows of the largest Nc that still runs in one launch, and Nc + 1,
                        which cannot
            fixed point one bank per length, all five modes, rows of hlen - 1 and of hlen samples, 3 levels, through the
                        whole-transform entries of the C ABI (the class clamps these away): N_l = hlen - 1 at every level
"""
import functools

import numpy as np

from tests import bank_matrix
from tests import ref2d
from tests import refext as R
from tests import refext1d as R1
from tests.helpers import band_err

F32, F64 = np.dtype(np.float32), np.dtype(np.float64)
DTYPES = (F32, F64)
TOL = {F32: 1e-5, F64: 1e-12}
ALL72 = bank_matrix.ALL72
PER_LENGTH = bank_matrix.one_bank_per_length()
MODES = R.MODES
hlen_of = bank_matrix.hlen_of
LENGTHS = list(range(2, 42, 2))

# ---- the geometry constants of the sources (compared with them by tests/test_newer_bank_matrix_cpu.py) ------------------------------
WFX, WFY, WIX, WIY = 32, 16, 64, 32   # wpt2d.hip: forward tile (child positions), inverse tile (parent samples)
EFX, EFY, EIX, EIY = 32, 16, 64, 32   # dwt_ext.hip: forward tile (band positions), inverse tile (parent samples)
kExt1dThreads, kExt1dTile = 256, 1024  # dwt_ext1d.hpp
kExt1dLdsMax, kExt1dPackLds = 160 * 1024, 32 * 1024  # dwt_ext1d.hip
LDS_OPT_IN = 64 * 1024  # what a kernel may use without the opt-in (`lds > 64 * 1024` in every launcher)


# ---- the LDS formulas and the plan of the one-launch 1-D path, restated ------------------------------------------------------------
def wp_fwd_lds(elem, h):
    return elem * ((2 * WFY + h - 2) * (2 * WFX + h - 2) + 2 * (2 * WFY + h - 2) * WFX)


def wp_inv_lds(elem, h):
    return elem * (4 * (WIY // 2 + h // 2) * (WIX // 2 + h // 2) + 2 * WIY * (WIX // 2 + h // 2))


def ext_fwd_lds(elem, h):
    ri, ci = 2 * EFY + h - 2, 2 * EFX + h - 2
    return elem * (ri * ci + 2 * ri * EFX) + 4 * (ri + ci)


def ext_inv_lds(elem, h):
    wr, wc = EIY // 2 + h // 2 - 1, EIX // 2 + h // 2 - 1
    return elem * (4 * wr * wc + 2 * EIY * wc)


TILE_LDS = {("wpt", "fwd"): wp_fwd_lds, ("wpt", "inv"): wp_inv_lds, ("ext2d", "fwd"): ext_fwd_lds, ("ext2d", "inv"): ext_inv_lds}


def ext_half(n, h):
    return (n + h - 1) >> 1


def ext1d_ru4(v):
    return (v + 3) & ~3


def ext1d_stride(n, h):
    return ext1d_ru4(ext1d_ru4(h - 2) + n + h - 1)


def ext1d_plan(nc, h, elem):
    """Ext1dPlan of dwt_ext1d.hip: (fused, R, LDS bytes of a forward workgroup, of an inverse workgroup)"""
    n1 = ext_half(nc, h)
    fwd, inv = (ext1d_stride(nc, h) + ext1d_stride(n1, h)) * elem, 3 * ext1d_ru4(n1) * elem
    row = max(fwd, inv)
    if row > kExt1dLdsMax:
        return False, 1, fwd, inv
    r = 1
    while r < 64 and r * n1 < kExt1dThreads and 2 * r * row <= kExt1dPackLds:
        r *= 2
    return True, r, r * fwd, r * inv


def _first(pred, lo, hi):
    """the smallest n in lo .. hi with pred(n), pred monotone"""
    while lo < hi:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if pred(mid) else (mid + 1, hi)
    return lo


def ext1d_opt_in_nc(h, elem):
    """the smallest row whose one-launch kernels both need more than 64 KiB (the strides only grow with the row)"""
    return _first(lambda n: min(ext1d_plan(n, h, elem)[2:]) > LDS_OPT_IN, h, 1 << 20)


def ext1d_last_fused_nc(h, elem):
    return _first(lambda n: not ext1d_plan(n, h, elem)[0], h, 1 << 20) - 1


# ---- the cases -------------------------------------------------------------------------------------------------------------------
# A case is a dict: cls ("wpt" | "ext2d" | "ext1d"), group, wname, shape, levels, mode (None for packets), via ("class" | "drivers" |
# "cabi"), dtypes, common_scale (the fixed-point rows only, see there).
def _case(cls, group, wname, shape, levels, mode=None, via="class", dtypes=DTYPES, common_scale=False):
    c = dict(cls=cls, group=group, wname=wname, hlen=hlen_of(wname), shape=tuple(int(v) for v in shape), levels=levels, mode=mode, via=via,
             dtypes=tuple(dtypes), common_scale=common_scale)
    c["id"] = "%s-%s-%s-%dx%d-L%d%s" % ((cls, group.replace(" ", "_"), wname) + c["shape"] + (levels, "-" + mode if mode else ""))
    return c


def mode_of(wname):
    return MODES[ALL72.index(wname) % 5]


def wp_sweep_shape(h):
    return max(2 * WIY + 3, 2 * h - 1), 2 * WIX + 4


def wp_two_shape(h):
    """even rows, odd columns; >= 4 (hlen - 1) for two levels of the class; the parents of the second level hold more than one
    forward tile (of 2 WFY x 2 WFX samples) and more than one inverse tile per axis"""
    return max(4 * (h - 1), 4 * WFY + 4), max(4 * (h - 1), 4 * WFX) + 1


def ext2d_interior_tile(h):
    """(ky, kx): the first forward tile whose window starts inside the image, 2 E k + 2 - hlen >= 0 per axis"""
    return -(-(h - 2) // (2 * EFY)), -(-(h - 2) // (2 * EFX))


def ext2d_sweep_shape(h):
    ky, kx = ext2d_interior_tile(h)
    return 2 * EFY * ky + 2 * EFY + 5, 2 * EFX * kx + 2 * EFX + 5


def ext2d_tile_is_interior(ky, kx, shape, h):
    """the condition of ext_stage_window (dwt_ext.hpp) for forward tile (ky, kx) of an image of `shape`"""
    ri, ci = 2 * EFY + h - 2, 2 * EFX + h - 2
    gy0, gx0 = 2 * EFY * ky + 2 - h, 2 * EFX * kx + 2 - h
    return gy0 >= 0 and gx0 >= 0 and gy0 + ri <= shape[0] and gx0 + ci <= shape[1]


def ext2d_tiles(shape, h):
    return -(-ext_half(shape[0], h) // EFY), -(-ext_half(shape[1], h) // EFX)


def ext2d_two_shape(h):
    return max(4 * (h - 1), 4 * EFY + 4) + 1, max(4 * (h - 1), 4 * EFX) + 2


def ext1d_sweep_shape(h):
    """elem-independent: R of the plan is the same in both precisions here (asserted on the CPU)"""
    nc = 4 * (h - 1) + 37
    return 2 * ext1d_plan(nc, h, 4)[1] + 1, nc


def ext1d_modes_shape(h):
    return 3, 8 * (h - 1) + 5  # three rows: one partial pack


WP_SWEEP = [_case("wpt", "sweep", w, wp_sweep_shape(hlen_of(w)), 1) for w in ALL72]
WP_TWO = [_case("wpt", "two levels", w, wp_two_shape(hlen_of(w)), 2) for w in PER_LENGTH]
WP_NODE = [_case("wpt", "one node", w, (hlen_of(w), hlen_of(w) + 1), 1, via="drivers") for w in PER_LENGTH]
E2_SWEEP = [_case("ext2d", "sweep", w, ext2d_sweep_shape(hlen_of(w)), 1, mode_of(w)) for w in ALL72]
E2_TWO = [_case("ext2d", "two levels", w, ext2d_two_shape(hlen_of(w)), 2, m) for w in PER_LENGTH for m in MODES]
E2_FOLD = [_case("ext2d", "folded", w, (hlen_of(w) - 1, hlen_of(w)), 1, m, via="drivers") for w in PER_LENGTH for m in MODES]
E1_SWEEP = [_case("ext1d", "sweep", w, ext1d_sweep_shape(hlen_of(w)), 2, mode_of(w)) for w in ALL72]
E1_MODES = [_case("ext1d", "modes", w, ext1d_modes_shape(hlen_of(w)), 3, m) for w in PER_LENGTH for m in MODES]
E1_OPTIN = [_case("ext1d", "opt-in", w, (2, ext1d_opt_in_nc(hlen_of(w), d.itemsize) + 3), 2, mode_of(w), dtypes=(d,)) for w in PER_LENGTH for d in DTYPES]
E1_EDGE = [_case("ext1d", "edge", w, (2, ext1d_last_fused_nc(hlen_of(w), d.itemsize) + k), 2, mode_of(w), dtypes=(d,))
           for w in PER_LENGTH for d in DTYPES for k in (0, 1)]
# At the fixed point N_l = hlen - 1 of every level the detail bands of `reflect` shrink to rounding noise and those of `periodic`
# towards it: the error of such a band over ITS OWN largest value is no measure (1e+9 for arithmetic that is correct to the last
# bit).  These cases alone judge every band over the largest value of all bands of the transform, at the same TOL.
E1_FIXED = [_case("ext1d", "fixed point", w, (3, hlen_of(w) - 1 + k), 3, m, via="cabi", common_scale=True) for w in PER_LENGTH for m in MODES for k in (0, 1)]

SWEEPS = {"wpt": WP_SWEEP, "ext2d": E2_SWEEP, "ext1d": E1_SWEEP}
PER_LENGTH_CASES = WP_TWO + WP_NODE + E2_TWO + E2_FOLD + E1_MODES + E1_OPTIN + E1_EDGE + E1_FIXED
CASES = WP_SWEEP + E2_SWEEP + E1_SWEEP + PER_LENGTH_CASES
IMPULSE_CASES = WP_TWO + E2_TWO + E1_MODES
FAMILIES = ("wpt", "ext2d", "ext1d_fused", "ext1d_level")  # ext1d_level: the length is a run-time argument of its four kernels


def case_fused(case, dt):
    return case["cls"] == "ext1d" and ext1d_plan(case["shape"][1], case["hlen"], np.dtype(dt).itemsize)[0]


def case_reaches(case, dt):
    """{(kernel family, direction, precision, bank length)} that a run of the case in `dt` launches"""
    if case["cls"] != "ext1d":
        fams = [case["cls"]]
    else:  # the class chains the level kernels when it is not fused; the sweep and the fixed-point rows run BOTH forms
        fams = ["ext1d_fused"] if case_fused(case, dt) else ["ext1d_level"]
        if case["group"] in ("sweep", "fixed point"):
            fams.append("ext1d_level")
    return {(f, d, np.dtype(dt).name, case["hlen"]) for f in fams for d in ("fwd", "inv")}


EXPECTED_REACH = {(f, d, t.name, h) for f in FAMILIES for d in ("fwd", "inv") for t in DTYPES for h in LENGTHS}


def lds_sides(reach):
    """{(family, direction, precision): (lengths reached at or below 64 KiB, lengths reached above)} of the two tile-kernel classes"""
    out = {}
    for (fam, d), fn in TILE_LDS.items():
        for t in DTYPES:
            hs = sorted(h for f, dd, tn, h in reach if (f, dd, tn) == (fam, d, t.name))
            out[(fam, d, t.name)] = ([h for h in hs if fn(t.itemsize, h) <= LDS_OPT_IN], [h for h in hs if fn(t.itemsize, h) > LDS_OPT_IN])
    return out


def lds_crossings():
    """{(family, direction, precision): the first length above 64 KiB} where the formulas cross it at all"""
    out = {}
    for (fam, d), fn in TILE_LDS.items():
        for t in DTYPES:
            above = [h for h in LENGTHS if fn(t.itemsize, h) > LDS_OPT_IN]
            if above:
                out[(fam, d, t.name)] = above[0]
    return out


# ---- inputs and the float64 reference ------------------------------------------------------------------------------------------------
def case_input(case):
    """uniform(-100, 100), one seed per bank, rounded to float32: both precisions transform the same values, so the float64 reference
    of a case (and its defect D) is computed once for the two"""
    return np.random.RandomState(1000 + ALL72.index(case["wname"])).uniform(-100, 100, case["shape"]).astype(np.float32)


def band_shapes(case):
    h, L, s = case["hlen"], case["levels"], case["shape"]
    if case["cls"] == "wpt":
        out, cur = [], s
        for d in range(1, L + 1):
            cur = ((cur[0] + 1) // 2, (cur[1] + 1) // 2)
            out += [cur] * 4 ** d
        return out
    if case["cls"] == "ext2d":
        return R.band_shapes(s, h, L)
    return [(s[0], n) for n in R1.band_lens(s[1], h, L)]


def band_gains(case):
    """per band, in the order of ref_forward: the product of the L2 norms of the analysis filters along the band's path -- the factor
    by which the band scales white noise.  1 for every band of an orthonormal bank; the bior3.x banks are far from it (|lo| = 2 |hi|
    for bior3.1: a factor 16 between the aa and the dd node of a two-level packet tree)."""
    taps = R.bank(case["wname"])[1]
    lo, hi = float(np.linalg.norm(taps["L"])), float(np.linalg.norm(taps["H"]))
    L = case["levels"]
    if case["cls"] == "wpt":  # digit q of a node: column high = q & 1, row high = q >> 1; one factor per axis and depth
        out, cur = [], [1.0]
        for _ in range(L):
            cur = [g * (hi if q & 1 else lo) * (hi if q >> 1 else lo) for g in cur for q in range(4)]
            out += cur
        return out
    if case["cls"] == "ext2d":
        return [lo ** (2 * L)] + [lo ** (2 * (l - 1)) * g for l in range(1, L + 1) for g in (lo * hi, lo * hi, hi * hi)]
    return [lo ** L] + [lo ** (l - 1) * hi for l in range(1, L + 1)]


def _wp_split(nodes, wname, mag=False):
    out = []
    for n in nodes:
        A, H, V, D = ref2d.dwt2_forward(n, wname, 1, mag)
        out += [A, H, V, D]
    return out


def ref_forward(case, x, mag=False):
    """the float64 bands of the case.  Packets: the nodes of depth 1, then of depth 2, ...: ref2d's one-level transform applied to every
    node again.  mag: with |x| and the magnitudes of the taps (positive wherever any product reaches a coefficient, exactly 0 elsewhere)"""
    x = np.asarray(x, np.float64)
    w, L = case["wname"], case["levels"]
    if mag:
        x = np.abs(x)
    if case["cls"] == "wpt":
        out, cur = [], [x]
        for _ in range(L):
            cur = _wp_split(cur, w, mag)
            out += cur
        return out
    if not mag:
        return R.wavedec2(x, w, L, case["mode"]) if case["cls"] == "ext2d" else R1.wavedec(x, w, L, case["mode"])
    taps = {k: np.abs(v) for k, v in R.bank(w)[1].items()}
    a, det = x, []
    for _ in range(L):
        if case["cls"] == "ext2d":
            a, h, v, d = R.dwt2(a, taps, case["mode"])
            det += [h, v, d]
        else:
            a, d = R.analysis(a, taps["L"], taps["H"], case["mode"])
            det.append(d)
    return [a] + det


def ref_inverse(case, bands):
    """the float64 image of the case's shape from `bands` (packets: from the nodes of the last depth)"""
    bands = [np.asarray(b, np.float64) for b in bands]
    w, L, s = case["wname"], case["levels"], case["shape"]
    if case["cls"] == "ext2d":
        return R.waverec2(bands, s, w)
    if case["cls"] == "ext1d":
        return R1.waverec(bands, s[1], w)
    shapes = [s]
    for _ in range(L):
        shapes.append(((shapes[-1][0] + 1) // 2, (shapes[-1][1] + 1) // 2))
    cur = bands[len(bands) - 4 ** L:]
    for d in range(L, 0, -1):
        cur = [ref2d.dwt2_inverse(cur[4 * i:4 * i + 4], shapes[d - 1], w) for i in range(4 ** (d - 1))]
    return cur[0]


@functools.lru_cache(maxsize=4)
def _reference(cid):
    case = BY_ID[cid]
    x = case_input(case).astype(np.float64)
    want = ref_forward(case, x)
    rec = ref_inverse(case, want)
    for a in want + [rec]:
        a.setflags(write=False)
    return want, rec, band_err(rec, x)


def reference(case):
    """(float64 bands, the reference's reconstruction from them, its defect D against the input); shared, not to be modified"""
    return _reference(case["id"])


BY_ID = {c["id"]: c for c in CASES}
assert len(BY_ID) == len(CASES)


# ---- the checks, shared by the GPU module and the float32 restatement on the CPU --------------------------------------------------------
# A backend is made by backend(case, x) with x in the precision under test, and has
#   forward() -> the bands in that precision, in the order of ref_forward     inverse_own() -> the image from those bands
#   inverse_of(bands) -> the image from bands given by the caller              close()
def _errs(got, want, dt, common_scale):
    assert len(got) == len(want), (len(got), len(want))
    scale = max(float(np.abs(b).max()) for b in want)
    out = []
    for k, (g, o) in enumerate(zip(got, want)):
        assert g.dtype == dt and g.shape == o.shape, (k, g.dtype, g.shape, o.shape)
        out.append(float(np.abs(g.astype(np.float64) - o).max()) / scale if common_scale else band_err(g, o))
    return out


def check(case, dt, backend, tol, note=lambda what, val: None):
    """forward, the two inverses and the round trip of one case; tol: the forward bound (TOL[dt] on the GPU)"""
    dt = np.dtype(dt)
    x = case_input(case).astype(dt)
    want, rec_ref, defect = reference(case)
    what = (case["id"], dt.name)
    be = backend(case, x)
    try:
        got = be.forward()
        for k, e in enumerate(_errs(got, want, dt, case["common_scale"])):
            note("forward", e)
            assert e <= tol, what + ("forward, band", k, e)
        rec = be.inverse_own()
        assert rec.dtype == dt
        e_inv, e_rt = band_err(rec, ref_inverse(case, got)), band_err(rec, x)
        note("inverse of its own bands", e_inv)
        note("round trip", e_rt)
        note("defect D", defect)
        assert e_inv <= 10 * tol, what + ("inverse of its own bands", e_inv)
        # 4 D and not D: D is itself a rounded figure, and the kernel's own rounding adds to the defect (tests/test_3d_all_banks_gpu.py)
        assert e_rt <= 10 * tol + 4 * defect, what + ("round trip", e_rt, defect)
        given = [b.astype(dt) for b in want]
        target = rec_ref if dt == F64 else ref_inverse(case, given)
        e_ref = band_err(be.inverse_of(given), target)
        note("inverse of the reference's bands", e_ref)
        assert e_ref <= 10 * tol, what + ("inverse of the reference's bands", e_ref)
    finally:
        be.close()


IMPULSE = 64.0  # a power of two: every product with a tap is exact in either precision


def impulse_positions(shape):
    return [(0, 0), (0, shape[1] - 1), (shape[0] - 1, 0), (shape[0] - 1, shape[1] - 1), (shape[0] // 2, shape[1] // 2)]


@functools.lru_cache(maxsize=8)
def _impulse_reference(cid, pos):
    case = BY_ID[cid]
    x = np.zeros(case["shape"])
    x[pos] = IMPULSE
    want = ref_forward(case, x)
    return want, ref_forward(case, x, mag=True), band_err(ref_inverse(case, want), x)


def check_impulses(case, dt, backend, tol, note=lambda what, val: None):
    """one impulse at each corner and at the centre: the fold of every border separately, and exact zeros.  Where no product of the
    impulse with non-zero taps reaches a coefficient -- the transform of |x| with the magnitudes of the taps is exactly zero there --
    the coefficient is zero in any precision and summation order, and must be exactly zero; a band that nothing reaches is zero as
    a whole.  A band that is zero in the float64 reference by CANCELLATION is another matter (bior1.5 at an odd size: the repeated
    last sample meets the taps c, -c, and the second level sees c v - c v of a v that is no power of two): the float32 oracle itself
    leaves rounding residue there, so it is not held to exact zeros.  A band below 0.15 of the largest band of the transform (such
    bands, and the ones an impulse barely reaches) is judged over that largest value, every other band over its own."""
    dt = np.dtype(dt)
    for pos in impulse_positions(case["shape"]):
        x = np.zeros(case["shape"], dt)
        x[pos] = IMPULSE
        want, support, defect = _impulse_reference(case["id"], pos)
        be = backend(case, x)
        try:
            got = be.forward()
            own, common = _errs(got, want, dt, False), _errs(got, want, dt, True)
            top = max(float(np.abs(b).max()) for b in want)
            for k in range(len(want)):
                e = own[k] if float(np.abs(want[k]).max()) >= 0.15 * top else common[k]
                note("forward", e)
                assert e <= tol, (case["id"], dt.name, pos, "band", k, e)
                assert not np.any(got[k][support[k] == 0]), (case["id"], dt.name, pos, "band", k, "leaks outside the support")
            e_rt = band_err(be.inverse_own(), x)
            note("round trip", e_rt)
            assert e_rt <= 10 * tol + 4 * defect, (case["id"], dt.name, pos, "round trip", e_rt, defect)
        finally:
            be.close()
