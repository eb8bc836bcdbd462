"""Every filter bank of the table through both 3-D classes (pdwt_amd.Wavelets3D / dwt3d.hip, pdwt_amd.StationaryWavelets3D /
swt3d.hip), in both precisions, forward and inverse, against the float64 direct-sum reference tests/ref3d.py (pinned on the CPU
by tests/test_ref3d_cpu.py).  tests/test_wavelets3d_gpu.py and tests/test_swt3d_gpu.py assert bit parity with the oracle for a
few orthogonal banks; this module asserts accuracy against a high-precision statement of the operation for all 72 banks --
every one of the 20 kernel instantiations per precision, the biorthogonal banks included -- and for shapes whose tile and chunk
grids are many blocks wide along one axis.

What is asserted, per case (TOL = 1e-5 float32, 1e-12 float64, band-normalised: helpers.band_err):
  forward     every band against ref3d                                                        <= TOL
  inverse     the volume against ref3d's inverse of THE BANDS THE GPU PRODUCED                <= 10 TOL
  round trip  the volume against the input                                                    <= 10 TOL + 4 D
              D = the reconstruction defect of the float64 reference itself on that volume (the table's sym* and bior4.4 /
              5.5 / 6.8 banks reconstruct to ~1e-11 only, in exact arithmetic)
  stationary  the bands bit-identical after inverse()
  (the ramp input alone normalises its detail bands by the largest band of the transform: they vanish by construction, see there)
  W.levels    as expected in every case; the closing test counts the cases: 72 banks x 2 classes x 2 precisions = 288, 0 left out.

How far the arithmetic the kernels are bit-identical to (the float32 / float64 oracle composition of test_wavelets3d_gpu.py, the
numpy composition of test_swt3d_gpu.py in the precision under test) sits from this reference, measured on a CPU by running every
case of this module with those compositions in the place of the GPU classes (worst band, forward / inverse):
  one level, all 72 banks        decimated   float32 5.0e-7 / 6.4e-7    float64 6.8e-16 / 1.9e-15
                                 stationary  float32 5.1e-7 / 7.7e-7    float64       - / 1.7e-15
  two levels, one bank / length  decimated   float32 7.6e-7 / 7.2e-7    float64 1.3e-15 / 2.3e-15
                                 stationary  float32 5.8e-7 / 6.6e-7    float64       - / 1.8e-15
  long axis, tile + 1, impulses, decimated   float32 2.7e-7 / 4.8e-7    float64 6.5e-16 / 1.1e-15
  ramp                           stationary  float32 3.1e-7 / 3.3e-7    float64       - / 7.1e-16
(-: the float64 numpy composition of the stationary analysis is this reference's own arithmetic, the figure is 0.)  The worst one
is a factor 13 inside the forward bar and every one below a fifth of its bar; the reference's own reconstruction defect D reaches
6.9e-11 at one level and 1.0e-10 at two (sym20)."""
import functools
import itertools

import numpy as np
import pytest

import pdwt_amd
from pdwt_amd import W_CREATION_ERROR, W_FORWARD, W_INVERSE
from tests import ref3d
from tests.helpers import band_err, load_golden

pytestmark = pytest.mark.gpu

TOL = {np.dtype(np.float32): 1e-5, np.dtype(np.float64): 1e-12}
F32, F64 = np.dtype(np.float32), np.dtype(np.float64)
ALL72 = [str(n) for n in load_golden("all72_1d_2x256_L1")["names"]]
KINDS = ("dwt", "swt")  # Wavelets3D, StationaryWavelets3D


def hlen_of(wname):
    return len(ref3d.bank(wname)[0])


def one_bank_per_length():
    """the first bior / rbio bank of every filter length that has one (4 .. 20), otherwise the first sym bank, otherwise haar"""
    by_len = {}
    for n in ALL72:
        by_len.setdefault(hlen_of(n), []).append(n)
    out = []
    for h in sorted(by_len):
        pick = [n for n in by_len[h] if n.startswith(("bior", "rbio"))] or [n for n in by_len[h] if n.startswith("sym")] or by_len[h]
        out.append(pick[0])
    return out


PER_LENGTH = one_bank_per_length()

# what ran, for the closing tests: (kind, wname, dtype) of every finished case, and the worst figures per (set, kind, dtype)
DONE = {"one_level": set(), "multi_level": set()}
WORST = {}


def _note(group, kind, dt, what, val):
    key = (group, kind, dt.name)
    WORST.setdefault(key, {})
    WORST[key][what] = max(WORST[key].get(what, 0.0), float(val))


# ---- the reference side -----------------------------------------------------------------------------------
def ref_forward(kind, vol, wname, L):
    return ref3d.dwt3_forward(vol, wname, L) if kind == "dwt" else ref3d.swt3_forward(vol, wname, L)


def ref_inverse(kind, bands, shape, wname, L):
    return ref3d.dwt3_inverse(bands, shape, wname, L) if kind == "dwt" else ref3d.swt3_inverse(bands, wname, L)


def random_volume(wname, shape):
    """uniform(-100, 100), one fixed seed per bank, rounded to float32: both precisions transform the same values, so the float64
    reference of a case (and its defect D) is computed once for the two"""
    seed = 1000 + ALL72.index(wname)
    return np.random.RandomState(seed).uniform(-100, 100, shape).astype(np.float32)


@functools.lru_cache(maxsize=1)
def _random_case_reference(kind, wname, shape, L):
    vol = random_volume(wname, shape).astype(np.float64)
    want = ref_forward(kind, vol, wname, L)
    defect = band_err(ref_inverse(kind, want, shape, wname, L), vol)
    return want, defect


def check(kind, wname, dtype, vol, levels, expect_L, group, want=None, defect=0.0, zeros_stay_zero=False, common_scale=False):
    """forward, inverse and round trip of one volume; `want` / `defect`: the float64 reference bands and its own reconstruction
    defect D where the caller has them (defect 0: the plain 10 TOL bound, which is the stricter one).  common_scale: the error
    of every band over the largest value of ALL bands instead of its own (the ramp only, see there)"""
    dt = np.dtype(dtype)
    vol = np.ascontiguousarray(vol, dtype=dt)
    cls = pdwt_amd.Wavelets3D if kind == "dwt" else pdwt_amd.StationaryWavelets3D
    W = cls(vol, wname, levels)
    assert W.state != W_CREATION_ERROR, (kind, wname, vol.shape)
    L = W.levels
    assert L == expect_L == ref3d.levels_of(vol.shape, wname, levels) and W.nbands == 7 * L + 1, (kind, wname, vol.shape, L)
    if want is None:
        want = ref_forward(kind, vol, wname, L)
    W.forward()
    assert W.state == W_FORWARD
    got = W.coeffs
    assert len(got) == len(want)
    for k, (g, o) in enumerate(zip(got, want)):
        assert g.dtype == dt and g.shape == o.shape, (k, g.shape, o.shape)
        e = band_err(g, o)
        if common_scale and k > 0:
            e = np.abs(g.astype(np.float64) - o).max() / max(np.abs(b).max() for b in want)
        _note(group, kind, dt, "forward", e)
        assert e <= TOL[dt], (kind, wname, dt.name, vol.shape, L, k, e)
        if zeros_stay_zero:  # a sum of products with zeros is zero in any precision: nothing may leak outside the support
            assert not np.any(g[o == 0]), (kind, wname, dt.name, vol.shape, k)
    W.inverse()
    assert W.state == W_INVERSE
    rec = W.get_image()
    e_inv = band_err(rec, ref_inverse(kind, got, vol.shape, wname, L))
    e_rt = band_err(rec, vol)
    _note(group, kind, dt, "inverse", e_inv)
    _note(group, kind, dt, "round trip", e_rt)
    _note(group, kind, dt, "defect D", defect)
    assert e_inv <= 10 * TOL[dt], (kind, wname, dt.name, vol.shape, L, e_inv)
    # 4 D and not D: D is itself a rounded figure (a max over ~1e6 samples of a difference near 1e-11 of values near 100), and the
    # kernel's own rounding adds to the defect; the factor only keeps that from deciding the result
    assert e_rt <= 10 * TOL[dt] + 4 * defect, (kind, wname, dt.name, vol.shape, L, e_rt, defect)
    if kind == "swt":  # the stationary inverse leaves every band intact, bit for bit
        for k, g in enumerate(got):
            assert np.array_equal(W.coeff_view(k).numpy(), g), (wname, k)
    W.close()
    return L


def check_random(kind, wname, dtype, shape, expect_L, group):
    want, defect = _random_case_reference(kind, wname, tuple(shape), expect_L)
    return check(kind, wname, dtype, random_volume(wname, shape), 99, expect_L, group, want, defect)


# ---- 2. every bank, one level -------------------------------------------------------------------------------
def shape_one_level(wname):
    """three different sides, not all of one parity, the smallest the level clamp allows plus a little: one level for every bank,
    and the window of every tile wraps"""
    m = hlen_of(wname) - 1
    return (5, 3, 7) if m == 1 else (2 * m + 1, 2 * m + 3, 4 * m + 2)


# (kind, bank) outermost, the precision innermost: the two precisions of a case share one reference
ONE_LEVEL = [(k, w, d) for k in KINDS for w in ALL72 for d in (F32, F64)]


@pytest.mark.parametrize("kind,wname,dtype", ONE_LEVEL, ids=["%s-%s-%s" % (k, w, d.name) for k, w, d in ONE_LEVEL])
def test_one_level_every_bank(kind, wname, dtype):
    check_random(kind, wname, dtype, shape_one_level(wname), 1, "one level, 72 banks")
    DONE["one_level"].add((kind, wname, dtype.name))


# ---- 2b. two levels, an odd size on both, one bank of every length ---------------------------------------------
def shape_two_levels(wname):
    m = hlen_of(wname) - 1
    return (4 * m + 1, 4 * m + 6, 4 * m + 3)  # level 2: (2m+1, 2m+3, 2m+2)


# The float64 numpy reference of the stationary transform at two levels of a (4m+1)^3-sized volume is the slow part of this module
# for the banks of 30 taps and more (sym15 .. sym20).  With all of them the module took 104 s on an MI355X machine against 34 s for
# tests/test_wavelets3d_gpu.py and tests/test_swt3d_gpu.py together, so of those 12 stationary cases three are kept: sym15 and
# sym20 in float64, sym20 in float32 (60 s with that; nothing else is cut).  Left out: stationary sym15 in float32 and sym16 ..
# sym19 in both precisions, 9 cases.  Every one of these banks runs in the one-level sweep in both classes and precisions, and at
# two levels in the decimated class.
KEPT_LONG_SWT = {("sym15", F64), ("sym20", F64), ("sym20", F32)}
MULTI_LEVEL = [(k, w, d) for k in KINDS for w in PER_LENGTH for d in (F32, F64)
               if not (k == "swt" and hlen_of(w) >= 30 and (w, d) not in KEPT_LONG_SWT)]
assert len(MULTI_LEVEL) == 80 - 9


@pytest.mark.parametrize("kind,wname,dtype", MULTI_LEVEL, ids=["%s-%s-%s" % (k, w, d.name) for k, w, d in MULTI_LEVEL])
def test_two_levels_odd_sizes_one_bank_per_length(kind, wname, dtype):
    check_random(kind, wname, dtype, shape_two_levels(wname), 2, "two levels, 20 banks")
    DONE["multi_level"].add((kind, wname, dtype.name))


# ---- 3. shapes and inputs ----------------------------------------------------------------------------------
# a 4-tap, a 6-tap biorthogonal (float64) and a 10-tap biorthogonal bank
SHAPE_BANKS = [("db2", F32), ("bior2.2", F64), ("rbio2.4", F32)]


def long_axis_shapes(kind, wname):
    """one long axis beside short ones, each axis in turn: many x-y tiles or z chunks along one grid dimension, the last one
    ragged.  The stationary bands are full size (15 of them at two levels), so its long axis is 1001 for the 6- and 10-tap banks
    (32 tiles of 32 along x, 63 chunks of 16 along z) and its short sides 4m, to keep the float64 numpy reference affordable."""
    m = hlen_of(wname) - 1
    if kind == "swt" and m > 3:
        a, b, n = 4 * m, 4 * m + 1, 1001
    else:
        a, b, n = 6 * m, 6 * m + 1, 3001
    return [(a, b, n), (a, n, b), (n, b, a)]


LONG_AXIS = [(k, w, d, s) for k in KINDS for w, d in SHAPE_BANKS for s in long_axis_shapes(k, w)]


@pytest.mark.parametrize("kind,wname,dtype,shape", LONG_AXIS, ids=["%s-%s-%s-%dx%dx%d" % ((k, w, d.name) + s) for k, w, d, s in LONG_AXIS])
def test_one_long_axis(kind, wname, dtype, shape):
    vol = np.random.RandomState(sum(shape)).uniform(-100, 100, shape).astype(dtype)
    L = check(kind, wname, dtype, vol, 99, 2, "long axis")  # 4m .. 6m+1 over m: two levels at the clamp
    assert L == 2


# The tile constants of the kernels (copied from the sources, not imported):
#   dwt3d.hip  forward x-y tile FTX x FTY = 32 x 16 outputs = 64 x 32 input samples; inverse x-y tile ITX x ITY = 64 x 32 samples;
#              z pass ZC = 16 outputs per chunk: 32 input planes forward, 16 output planes inverse
#   swt3d.hip  x-y tile STX x STY = 32 x 16 samples of one sublattice (every 2^(lev-1)-th sample); z chunk swt_zc = 16 planes of one
#              sublattice (8 in float64 above 24 taps: the one-level sweep ends those chunks part-way for every such bank)
# (33, 33, 65): one forward tile (64 x 32) plus one sample in x and y and one forward z chunk (32) plus one plane; one inverse tile
#              (64 x 32) plus one; for the stationary class at level 2 (spacing 2) the sublattices have 17 / 17 / 33 samples: one
#              tile and one chunk plus one; its level 2 for the decimated class is (17, 17, 33)
# (17, 17, 33): one inverse z chunk (16) plus one plane; one stationary tile (32 x 16) and chunk (16) plus one at level 1.  The level
#              clamp refuses 17 samples for the 10-tap bank (17 // 9 < 2), which therefore runs the first shape only.
TILE_PLUS_ONE = [(33, 33, 65), (17, 17, 33)]
TILE_CASES = [(k, w, d, s) for k in KINDS for w, d in SHAPE_BANKS for s in TILE_PLUS_ONE if ref3d.levels_of(s, w, 99) >= 1]
assert len(TILE_CASES) == 10


@pytest.mark.parametrize("kind,wname,dtype,shape", TILE_CASES, ids=["%s-%s-%s-%dx%dx%d" % ((k, w, d.name) + s) for k, w, d, s in TILE_CASES])
def test_one_tile_and_one_chunk_plus_one(kind, wname, dtype, shape):
    vol = np.random.RandomState(sum(shape)).uniform(-100, 100, shape).astype(dtype)
    L = ref3d.levels_of(shape, wname, 99)
    assert L >= 1
    for levels in sorted({1, L}):
        check(kind, wname, dtype, vol, levels, levels, "tile + 1")


STRUCT_SHAPE = (19, 33, 65)  # (19: the fewest odd planes the level clamp takes for 10 taps)
STRUCT_CASES = [(k, w, d) for k in KINDS for w, d in SHAPE_BANKS]


@pytest.mark.parametrize("kind,wname,dtype", STRUCT_CASES, ids=["%s-%s-%s" % (k, w, d.name) for k, w, d in STRUCT_CASES])
def test_impulses_at_the_corners_and_the_centre(kind, wname, dtype):
    """a max-normalised error on noise says little about WHERE an error sits; a single impulse has an exactly known answer (products
    of three taps at the wrapped positions, pinned for ref3d in tests/test_ref3d_cpu.py): the wrap and the centre offset of every
    axis separately, and exact zeros everywhere else"""
    corners = list(itertools.product(*[(0, n - 1) for n in STRUCT_SHAPE])) + [tuple(n // 2 for n in STRUCT_SHAPE)]
    assert len(corners) == 9
    for pos in corners:
        vol = np.zeros(STRUCT_SHAPE, dtype)
        vol[pos] = 100.0
        check(kind, wname, dtype, vol, 1, 1, "impulses", zeros_stay_zero=True)


@pytest.mark.parametrize("kind,wname,dtype", STRUCT_CASES, ids=["%s-%s-%s" % (k, w, d.name) for k, w, d in STRUCT_CASES])
def test_ramp_with_one_decimal_place_per_axis(kind, wname, dtype):
    """vol[z, y, x] = 1e4 z + 1e2 y + x: mixing up two axes or two quadrants changes the leading digits of the bands.
    A sum of one function per axis is annihilated by every band with two or more high-pass letters, and a band with one keeps the
    (small) step of its own axis only: the true detail bands are zero or tiny beside the rounding of values near 2e5, and the
    error of a band over ITS OWN largest value is no measure there -- for the float64 reference against the float32 and float64
    compositions it is 1e0 .. 1e9 on those bands, in arithmetic that is correct to the last bit.  So on this input only the details
    are judged over the largest value of all bands (the approximation's, ~5e5), at the same TOL; the approximation, the inverse
    and the round trip keep the plain metric."""
    z, y, x = np.meshgrid(*[np.arange(n) for n in STRUCT_SHAPE], indexing="ij")
    vol = (1e4 * z + 1e2 * y + x).astype(dtype)  # <= 183264: exact in float32
    L = ref3d.levels_of(STRUCT_SHAPE, wname, 99)
    for levels in sorted({1, L}):
        check(kind, wname, dtype, vol, levels, levels, "ramp", common_scale=True)


# ---- the closing count -------------------------------------------------------------------------------------
def test_no_case_was_left_out():
    """a condition, not a measurement: every bank, class and precision ran to the end of its checks (none skipped, none in a
    creation-error branch), and with them every filter length 2 .. 40 in both precisions, both classes, forward and inverse.
    It counts what the tests above recorded in this process, so it holds for a run of the whole module only."""
    for key in sorted(WORST):
        print("worst %-22s %-4s %-8s" % key, "  ".join("%s %.2e" % kv for kv in sorted(WORST[key].items())))
    want = {(k, w, d.name) for k, w, d in ONE_LEVEL}
    assert len(want) == 288 and DONE["one_level"] == want, sorted(want - DONE["one_level"])
    for kind in KINDS:
        for d in (F32, F64):
            lengths = sorted({hlen_of(w) for k, w, dn in DONE["one_level"] if (k, dn) == (kind, d.name)})
            assert lengths == list(range(2, 42, 2)), (kind, d.name, lengths)
    want = {(k, w, d.name) for k, w, d in MULTI_LEVEL}
    assert len(want) == 71 and DONE["multi_level"] == want, sorted(want - DONE["multi_level"])
