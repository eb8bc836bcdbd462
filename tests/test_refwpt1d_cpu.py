"""CPU-only: pins tests/refwpt1d.py (the packet-tree reference of the 1-D GPU tests) to the oracle's ordinary batched 1-D transform.

  * the all-"a" path equals band 0 of the ordinary L-level oracle transform (ndim = 1) and node 1 of depth l equals D_l, bit for bit,
    in both precisions, on odd sizes;
  * the numpy restatement of the Haar tree (used for the 4096-node case) has the oracle's bits;
  * round trips of the reference alone: float32 <= 6.1e-7, float64 <= 2.6e-15, float64 with sym8 1.09e-12 (the defect of the table's bank);
  * the Gray-code property: a sinusoid at the centre of frequency band r of a depth puts its energy maximum on the node of rank r;
  * the basis validator, and a best basis worked out by hand on a 2-level tree.
"""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import refwpt1d as R
from tests.helpers import band_err

PIN = [((5, 77), "haar", 6), ((2, 1031), "db3", 7), ((4, 200), "bior2.2", 5)]


def _rows(shape, dt):
    return np.random.RandomState(1).uniform(-100, 100, shape).astype(dt)


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("shape,wname,L", PIN)
def test_all_a_path_is_the_ordinary_transform(shape, wname, L, dt):
    x = _rows(shape, dt)
    assert R.clamp_levels(shape[1], wname, 9) == L
    tr = R.tree(x, wname, 9)
    assert len(tr) == L + 1 and [t.shape for t in tr] == [(shape[0], 2 ** d, n) for d, n in enumerate(R.lengths(shape[1], L))]
    O = orc.OracleWavelets(x, wname, L, ndim=1)
    O.forward()
    assert O.info.nlevels == L
    bands = O.coeffs  # [A_L, D_1, ..., D_L]
    assert np.array_equal(tr[L][:, 0], bands[0])
    for k in range(1, L + 1):
        assert R.index_of("a" * (k - 1) + "d") == (k, 1)
        assert np.array_equal(tr[k][:, 1], bands[k]), k


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("shape,L", [((5, 77), 6), ((3, 45), 4), ((2, 64), 6)])
def test_numpy_haar_tree_has_the_oracle_bits(shape, L, dt):
    x = _rows(shape, dt)
    a, b = R.tree(x, "haar", L), R.haar_tree(x, L)
    assert len(a) == len(b) == L + 1
    for ta, tb in zip(a, b):
        assert ta.dtype == tb.dtype and ta.shape == tb.shape and np.array_equal(ta, tb)


def test_paths_levels_and_frequency_order():
    assert R.index_of("") == (0, 0) and R.index_of("ad") == (2, 1) and R.index_of("d") == (1, 1) and R.index_of("dda") == (3, 6)
    for d in range(5):
        for i in range(2 ** d):
            assert R.index_of(R.path_of(d, i)) == (d, i)
    assert R.clamp_levels(96, "db4", 9) == 3       # ilog2(96 / 7) = 3
    assert R.clamp_levels(2 ** 14, "haar", 20) == 12  # the cap
    assert R.clamp_levels(4096, "haar", 12) == 12
    assert R.clamp_levels(6, "db4", 2) == 0        # too short for one level
    assert R.clamp_levels(64, "db2", 0) == 1
    assert [R.path_of(2, i) for i in R.frequency_order(2)] == ["aa", "ad", "dd", "da"]  # PyWavelets' order='freq'
    assert list(R.frequency_order(3)) == [0, 1, 3, 2, 6, 7, 5, 4]
    for d in range(0, 13):
        f = R.frequency_order(d)
        assert sorted(f) == list(range(2 ** d))


@pytest.mark.parametrize("wname,depth,floor", [("sym8", 4, 0.6), ("db4", 4, 0.55), ("db20", 3, 0.6), ("haar", 4, 0.3)])
def test_gray_code_is_the_frequency_order(wname, depth, floor):
    """sinusoids at the band centres of a 1024-sample row: the energy maximum of depth `depth` falls on the node of rank r"""
    n, nb = 1024, 2 ** depth
    t = np.arange(n)
    rows = np.stack([np.sin(2 * np.pi * (r + 0.5) * (n / (2.0 * nb)) * t / n + 0.3) for r in range(nb)])
    lev = R.tree(rows, wname, depth)[depth]
    energy = (lev.astype(np.float64) ** 2).sum(axis=2)  # (row = rank, node)
    order = R.frequency_order(depth)
    share = []
    for r in range(nb):
        assert int(np.argmax(energy[r])) == order[r], (wname, r)
        share.append(energy[r, order[r]] / energy[r].sum())
    print("%s depth %d: smallest share of the energy in the node of its rank %.3f" % (wname, depth, min(share)))
    assert min(share) >= floor


@pytest.mark.parametrize("dt,bound", [(np.float32, 6.1e-7), (np.float64, 2.6e-15)])
@pytest.mark.parametrize("shape,wname,L", PIN + [((3, 64), "db2", 4), ((6, 48), "coif1", 3)])
def test_inverse_round_trip(shape, wname, L, dt, bound):
    x = _rows(shape, dt)
    tr = R.tree(x, wname, L)
    full = {(L, i): tr[L][:, i] for i in range(2 ** L)}
    e1 = band_err(R.inverse(full, shape, wname, L), x)
    mixed = {(1, 1): tr[1][:, 1], (2, 0): tr[2][:, 0]}
    mixed.update({(3, 2 + q): tr[3][:, 2 + q] for q in range(2)})
    e2 = band_err(R.inverse(mixed, shape, wname, L), x)
    print("%s %s %s: round trip %.3e / mixed basis %.3e" % (shape, wname, np.dtype(dt).name, e1, e2))
    assert max(e1, e2) <= bound


def test_sym8_round_trip_shows_the_defect_of_its_bank():
    x = _rows((2, 1000), np.float64)
    tr = R.tree(x, "sym8", 9)
    L = len(tr) - 1
    assert L == 6
    e = band_err(R.inverse({(L, i): tr[L][:, i] for i in range(2 ** L)}, x.shape, "sym8", L), x)
    print("sym8 float64 round trip %.3e" % e)
    assert 1e-13 <= e <= 2e-12  # 1.09e-12: the table's sym8 does not reconstruct exactly


def test_basis_validator():
    R.check_basis([(0, 0)], 2)
    R.check_basis([(1, 0), (2, 2), (2, 3)], 2)
    with pytest.raises(ValueError):
        R.check_basis([(1, 0)], 2)                       # incomplete
    with pytest.raises(ValueError):
        R.check_basis([(1, 0), (1, 1), (2, 3)], 2)       # a node below another
    with pytest.raises(ValueError):
        R.check_basis([(1, 0), (1, 0), (1, 1)], 2)       # twice
    with pytest.raises(ValueError):
        R.check_basis([(3, 0)], 2)                       # outside the tree
    with pytest.raises(ValueError):
        R.check_basis([(1, 2)], 2)


def test_best_basis_by_hand():
    # depth 0: 10; depth 1: 4, 7; depth 2: 1, 2 | 3, 5.  "a": children 3 < 4 -> split (best 3); "d": children 8 > 7 -> keep (7);
    # root: 3 + 7 = 10 <= ... the parent is kept on a tie (cost <= children)
    basis, margin = R.best_basis([np.array([10.0]), np.array([4.0, 7.0]), np.array([1.0, 2.0, 3.0, 5.0])])
    assert basis == [(0, 0)] and margin == 0.0
    basis, margin = R.best_basis([np.array([10.5]), np.array([4.0, 7.0]), np.array([1.0, 2.0, 3.0, 5.0])])
    assert basis == [(1, 1), (2, 0), (2, 1)]
    assert abs(margin - 0.5 / 10.5) < 1e-15
    R.check_basis(basis, 2)
    # per-row costs add up to the summed ones, in row order
    tr = R.tree(_rows((3, 64), np.float64), "db2", 2)
    for kind in ("l1", "shannon"):
        pr, sm = R.node_costs(tr, kind, per_row=True), R.node_costs(tr, kind)
        for p, s in zip(pr, sm):
            assert p.shape == (3, len(s)) and np.array_equal((p[0] + p[1]) + p[2], s)
