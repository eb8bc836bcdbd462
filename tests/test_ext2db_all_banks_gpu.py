"""All 72 banks through the batched 2-D transform with boundary modes (BoundaryImageBatch, dwt_ext2db.hip), both precisions, against
tests/refext.py per image (band-normalised 1e-5 / 1e-12, round trip 10x) and, bit for bit, against the per-image BoundaryWavelets2D.

Sweep: B = 2 on (2(F-1)+1) x (2(F-1)+3) at one level, mode = bank index mod 5.  At that size every bank length is fused in both
precisions (the worst case, 40 taps float64 on 79 x 81, needs about 127 KB of LDS), so all 80 instantiations of the fused kernels run.
Two levels: one bank per length on (4(F-1)+1) x (4(F-1)+3), on whichever form the plan picks (the test asserts that the class reports
the plan's choice; the long float64 banks run per level).

The round trip is compared with the REFERENCE's round trip (refext.waverec2 of refext.wavedec2), not with the input: several banks of the
table do not reconstruct to 1e-11 in exact arithmetic of their tabulated taps (the float64 reference itself returns sym3 at 1.2e-11,
sym18 at 9.7e-12 and sym20 at 3.0e-11 of the input on the sweep shapes), which is a property of the bank, not of the kernels."""
import numpy as np
import pytest

import pdwt_amd
from pdwt_amd import BoundaryImageBatch, BoundaryWavelets2D
from tests import bank_matrix
from tests import refext as R
from tests.helpers import band_err

pytestmark = pytest.mark.gpu

FWD = {np.dtype(np.float32): 1e-5, np.dtype(np.float64): 1e-12}
RT = {k: 10 * v for k, v in FWD.items()}
DTYPES = [np.float32, np.float64]
ALL72 = bank_matrix.ALL72
PER_LENGTH = bank_matrix.one_bank_per_length()
B = 2


def _images(Nr, Nc, dt):
    yy, xx = np.mgrid[0:Nr, 0:Nc]
    return (np.random.RandomState(Nr).standard_normal((B, Nr, Nc)) + ((3 * xx + 5 * yy) % 17 - 8.0)).astype(dt)


def _run(wname, shape, levels, mode, dt, want_fused=None):
    F, _ = R.bank(wname)
    Nr, Nc = shape
    x = _images(Nr, Nc, dt)
    W = BoundaryImageBatch(x, wname, levels, mode)
    assert W.levels == levels
    plan = bool(pdwt_amd.hip().pdwt_ext2db_fused(Nr, Nc, F, levels, np.dtype(dt).itemsize))
    assert W.fused == plan
    if want_fused is not None:
        assert plan == want_fused
    W.forward()
    got = W.coeffs
    W.inverse()
    back = W.get_image()
    worst = 0.0
    for b in range(B):
        ref = R.wavedec2(x[b], wname, levels, mode, np.float64)
        T = BoundaryWavelets2D(x[b], wname, levels, mode)
        T.forward()
        for k, (r, t) in enumerate(zip(ref, T.coeffs)):
            e = band_err(got[k][b], r)
            worst = max(worst, e)
            assert e <= FWD[np.dtype(dt)], (wname, "band", k, "image", b, e)
            assert np.array_equal(got[k][b], t), (wname, "band", k, "image", b)
        T.inverse()
        assert np.array_equal(back[b], T.get_image()), (wname, b)
        e = band_err(back[b], R.waverec2(ref, shape, wname, np.float64))
        assert e <= RT[np.dtype(dt)], (wname, "round trip", b, e)
    print("%s F=%d %s %s %s fused=%s: worst band %.3e" % (wname, F, shape, mode, np.dtype(dt).name, W.fused, worst))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("wname", ALL72)
def test_every_bank_one_level_fused(wname, dt):
    F = bank_matrix.hlen_of(wname)
    _run(wname, (2 * (F - 1) + 1, 2 * (F - 1) + 3), 1, R.MODES[ALL72.index(wname) % 5], dt, want_fused=True)


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("wname", PER_LENGTH)
def test_one_bank_per_length_two_levels(wname, dt):
    F = bank_matrix.hlen_of(wname)
    _run(wname, (4 * (F - 1) + 1, 4 * (F - 1) + 3), 2, R.MODES[PER_LENGTH.index(wname) % 5], dt)
