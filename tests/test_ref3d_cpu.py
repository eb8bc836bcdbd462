"""CPU-only: pins tests/ref3d.py, the float64 direct-sum reference of tests/test_3d_all_banks_gpu.py, so that it cannot drift
with the kernels.  It is compared with (a) the oracle composition of tests/test_wavelets3d_gpu.py and the numpy a-trous
composition of tests/test_swt3d_gpu.py (both run on the CPU) for one bank of every filter length on odd sizes, (b) the
PyWavelets goldens that apply in 1-D, and (c) properties that need no second implementation: the operator matrices written out
entry by entry from the definition, impulses at the corners of an odd-sized volume, and energy conservation of the orthogonal banks."""
import itertools

import numpy as np
import pytest

from tests import ref3d
from tests.helpers import band_err, golden_bands, load_golden
from tests import test_swt3d_gpu as swt_comp
from tests import test_wavelets3d_gpu as dwt_comp

ALL72 = [str(n) for n in load_golden("all72_1d_2x256_L1")["names"]]
# agreement of the reference with a composition computed in `dtype` (the float32 figure is the rounding of the composition)
AGREE = {np.dtype(np.float64): 1e-12, np.dtype(np.float32): 1e-5}


def hlen_of(wname):
    return len(ref3d.bank(wname)[0])


def one_bank_per_length():
    """the first bior / rbio bank of every filter length that has one, otherwise the first sym bank, otherwise haar"""
    by_len = {}
    for n in ALL72:
        by_len.setdefault(hlen_of(n), []).append(n)
    out = []
    for h in sorted(by_len):
        names = by_len[h]
        pick = [n for n in names if n.startswith(("bior", "rbio"))] or [n for n in names if n.startswith("sym")] or names
        out.append(pick[0])
    return out


PER_LENGTH = one_bank_per_length()


def test_bank_table_has_all_20_lengths():
    assert len(ALL72) == 72 and sorted(hlen_of(n) for n in PER_LENGTH) == list(range(2, 42, 2))
    assert sum(n.startswith(("bior", "rbio")) for n in PER_LENGTH) == 9  # lengths 4 .. 20


def shape_one_level(wname, extra=2):
    m = hlen_of(wname) - 1
    return (5, 3, 7) if m == 1 else (2 * m + 1, 2 * m + 3, 4 * m + extra)


# ---- (a) against the two compositions --------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("wname", PER_LENGTH)
def test_decimated_vs_oracle_composition(wname, dtype):
    dt = np.dtype(dtype)
    m = hlen_of(wname) - 1
    for shape, L in ((shape_one_level(wname), 1), ((4 * m + 1, 4 * m + 6, 4 * m + 3), 2)):
        if L == 2 and m > 11 and m != 39:
            continue  # two levels: the short banks and the longest one (the oracle composition of the others repeats level 1)
        assert ref3d.levels_of(shape, wname, 99) == L == dwt_comp.clamp(shape, wname, 99)
        vol = np.random.RandomState(m).uniform(-100, 100, shape).astype(dt)
        want = dwt_comp.ref_forward(vol, wname, L)
        got = ref3d.dwt3_forward(vol, wname, L)
        assert len(got) == len(want) == 7 * L + 1
        for k, (g, o) in enumerate(zip(got, want)):
            assert g.dtype == np.float64 and g.shape == o.shape
            assert band_err(o, g) <= AGREE[dt], (wname, shape, k, band_err(o, g))
        rec = ref3d.dwt3_inverse(want, shape, wname, L)
        assert band_err(dwt_comp.ref_inverse(want, shape, wname, L), rec) <= AGREE[dt], (wname, shape)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("wname", PER_LENGTH)
def test_stationary_vs_numpy_composition(wname, dtype):
    dt = np.dtype(dtype)
    m = hlen_of(wname) - 1
    for shape, L in ((shape_one_level(wname, extra=0)[:2] + (2 * m + 6,), 1), ((4 * m + 1, 4 * m + 6, 4 * m + 3), 2)):
        if L == 2 and m > 7:
            continue  # the numpy composition is slow: two levels (spacing 2) for the short banks only
        assert ref3d.levels_of(shape, wname, 99) == L == swt_comp.clamp(shape, wname, 99)
        vol = np.random.RandomState(m + 100).uniform(-100, 100, shape).astype(dt)
        want = swt_comp.ref_forward(vol, wname, L)
        got = ref3d.swt3_forward(vol, wname, L)
        assert len(got) == len(want) == 7 * L + 1
        for k, (g, o) in enumerate(zip(got, want)):
            assert g.dtype == np.float64 and g.shape == o.shape == shape
            assert band_err(o, g) <= AGREE[dt], (wname, shape, k, band_err(o, g))
        assert band_err(swt_comp.ref_inverse(want, wname, L), ref3d.swt3_inverse(want, wname, L)) <= AGREE[dt], (wname, shape)


# ---- (b) against PyWavelets ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["b1d_3x77_db3_L2_odd", "b1d_5x256_sym8_L4", "swt1d_6x128_sym4_L3"])
def test_1d_functions_vs_pywavelets_goldens(name):
    d = load_golden(name)
    x, L, w = d["input"], d["levels"], d["wname"]
    tol = 1e-10 if x.dtype == np.float64 else 1e-6  # the goldens were stored in the dtype of their input
    swt = d["kind"] == "swt1"
    assert d["kind"] in ("dwt1", "swt1")
    got = ref3d.swt1d_forward(x, w, L) if swt else ref3d.dwt1d_forward(x, w, L)
    want = golden_bands(d)
    assert len(got) == len(want) == L + 1
    for k, (g, o) in enumerate(zip(got, want)):
        assert band_err(g, o) <= tol, (name, k, band_err(g, o))
    rec = ref3d.swt1d_inverse(want, w) if swt else ref3d.dwt1d_inverse(want, x.shape[-1], w)
    assert band_err(rec, d["recon"]) <= 10 * tol, (name, band_err(rec, d["recon"]))


def test_one_level_of_all_72_banks_vs_pywavelets():
    d = load_golden("all72_1d_2x256_L1")
    for n in ALL72:
        a, det = ref3d.dwt1d_forward(d["input"], n, 1)
        assert band_err(a, d["A_" + n]) <= 1e-10 and band_err(det, d["D_" + n]) <= 1e-10, n


# ---- (c) properties --------------------------------------------------------------------------------------------
def matrices(wname, n, kind, f=1):
    """the operators of one level on a line of n samples, entry by entry from the definition: analysis (lo, hi) and synthesis
    (from a, from d), as dense matrices [output, input]"""
    FL, FH, IL, IH = ref3d.bank(wname, kind == "swt")
    hlen = len(FL)
    if kind == "dwt":
        no, ne, c = (n + 1) // 2, n + (n & 1), hlen // 2 - 1
        lo, hi = np.zeros((no, n)), np.zeros((no, n))
        for i, j in itertools.product(range(no), range(hlen)):
            s = (2 * i - c + j) % ne
            s = n - 1 if s == n else s  # the repeated last sample of an odd line
            lo[i, s] += FL[hlen - 1 - j]
            hi[i, s] += FH[hlen - 1 - j]
        h2 = hlen // 2
        c, shift = h2 // 2, (0 if h2 % 2 else 1)
        sa, sd = np.zeros((n, no)), np.zeros((n, no))
        for g, j in itertools.product(range(n), range(h2)):
            p, off = (g + shift) // 2, 1 - ((g + shift) & 1)
            sa[g, (p - c + j) % no] += IL[hlen - 1 - (2 * j + off)]
            sd[g, (p - c + j) % no] += IH[hlen - 1 - (2 * j + off)]
        return lo, hi, sa, sd
    lo, hi, sa, sd = (np.zeros((n, n)) for _ in range(4))
    for g, k in itertools.product(range(n), range(hlen)):
        lo[g, (g - (hlen // 2 - 1) * f + f * k) % n] += FL[hlen - 1 - k]
        hi[g, (g - (hlen // 2 - 1) * f + f * k) % n] += FH[hlen - 1 - k]
        sa[g, (g - (hlen // 2) * f + f * k) % n] += IL[hlen - 1 - k] / 2
        sd[g, (g - (hlen // 2) * f + f * k) % n] += IH[hlen - 1 - k] / 2
    return lo, hi, sa, sd


IMPULSE_BANKS = ["haar", "db2", "bior2.2", "rbio3.1", "bior1.5", "sym7", "rbio3.9", "db15", "sym20"]  # h2 odd and even, zero-padded ends


@pytest.mark.parametrize("wname", IMPULSE_BANKS)
def test_every_impulse_of_a_line_gives_the_taps(wname):
    hlen = hlen_of(wname)
    for n in (2 * hlen - 1, 2 * hlen + 2):  # odd (the extension) and even
        eye = np.eye(n)
        lo, hi, sa, sd = matrices(wname, n, "dwt")
        F = ref3d.bank(wname, 0)
        glo, ghi = ref3d.dwt_ana(eye, 0, F)  # column s = the response to an impulse at s
        assert np.abs(glo - lo).max() <= 1e-15 and np.abs(ghi - hi).max() <= 1e-15, (wname, n)
        no = (n + 1) // 2
        z = np.zeros((no, no))
        assert np.abs(ref3d.dwt_syn(np.eye(no), z, 0, n, F) - sa).max() <= 1e-15, (wname, n)
        assert np.abs(ref3d.dwt_syn(z, np.eye(no), 0, n, F) - sd).max() <= 1e-15, (wname, n)
        for f in (1, 2):
            n2 = n + (hlen - 1) * (f - 1) + 1
            lo, hi, sa, sd = matrices(wname, n2, "swt", f)
            F = ref3d.bank(wname, 1)
            eye, z = np.eye(n2), np.zeros((n2, n2))
            glo, ghi = ref3d.swt_ana(eye, 0, F, f)
            assert np.abs(glo - lo).max() <= 1e-15 and np.abs(ghi - hi).max() <= 1e-15, (wname, n2, f)
            assert np.abs(ref3d.swt_syn(eye, z, 0, F, f) - sa).max() <= 1e-15, (wname, n2, f)
            assert np.abs(ref3d.swt_syn(z, eye, 0, F, f) - sd).max() <= 1e-15, (wname, n2, f)


@pytest.mark.parametrize("kind", ["dwt", "swt"])
@pytest.mark.parametrize("wname", IMPULSE_BANKS)
def test_corner_impulses_of_an_odd_volume_give_the_tap_products(wname, kind):
    """an impulse at each of the 8 corners (and the centre) of an odd-sized volume: every band is the outer product of the 1-D
    responses, i.e. products of three taps at the wrapped positions (sums of two where the odd extension repeats the corner)"""
    m = hlen_of(wname) - 1
    shape = (2 * m + 1, 2 * m + 3, 2 * m + 5)
    ops = [matrices(wname, n, kind)[:2] for n in shape]  # per axis (z, y, x): lo, hi
    fwd = ref3d.dwt3_forward if kind == "dwt" else ref3d.swt3_forward
    corners = list(itertools.product(*[(0, n - 1) for n in shape])) + [tuple(n // 2 for n in shape)]
    for pos in corners:
        vol = np.zeros(shape)
        vol[pos] = 1.0
        got = fwd(vol, wname, 1)
        for key, g in zip(("aaa",) + ref3d.BAND_KEYS, got):
            rz, ry, rx = (ops[ax]["ad".index(key[ax])][:, pos[ax]] for ax in range(3))
            want = rz[:, None, None] * ry[None, :, None] * rx[None, None, :]
            assert g.shape == want.shape and np.abs(g - want).max() <= 1e-15, (wname, kind, pos, key)
            assert key != "aaa" or np.count_nonzero(want) > 0  # (a Haar detail of the repeated last sample is a true zero)


@pytest.mark.parametrize("wname", [n for n in ALL72 if n.startswith(("haar", "db", "coif"))])
def test_orthogonal_banks_preserve_energy(wname):
    m = hlen_of(wname) - 1
    shape = (2 * m + 2, 2 * m + 4, 2 * m + 6)
    vol = np.random.RandomState(m).uniform(-100, 100, shape)
    e0 = (vol ** 2).sum()
    e1 = sum((b ** 2).sum() for b in ref3d.dwt3_forward(vol, wname, 1))
    assert abs(e1 - e0) <= 1e-12 * e0, (wname, abs(e1 - e0) / e0)
    # the stationary level is the decimated one at all 8 shifts: 8 times the energy
    e8 = sum((b ** 2).sum() for b in ref3d.swt3_forward(vol, wname, 1))
    assert abs(e8 - 8 * e0) <= 1e-12 * 8 * e0, (wname, abs(e8 - 8 * e0) / (8 * e0))


def test_perfect_reconstruction_defect_follows_the_table():
    """the table's db / coif banks reconstruct to rounding; sym20 does not (its tabulated taps carry ~1e-11): the reason
    tests/test_3d_all_banks_gpu.py takes its round-trip bound from this reference and not from a constant"""
    for wname, lo, hi in (("db4", 0, 1e-14), ("coif5", 0, 1e-14), ("bior2.2", 0, 1e-14), ("sym20", 1e-11, 1e-9)):
        shape = shape_one_level(wname)
        vol = np.random.RandomState(1).uniform(-100, 100, shape)
        for rec in (ref3d.dwt3_inverse(ref3d.dwt3_forward(vol, wname, 1), shape, wname, 1),
                    ref3d.swt3_inverse(ref3d.swt3_forward(vol, wname, 1), wname, 1)):
            assert lo <= band_err(rec, vol) <= hi, (wname, band_err(rec, vol))
