"""CPU-only: pins tests/refwpt.py (the packet-tree reference of the GPU tests) to the oracle's ordinary transform.

  * depth 1 equals the oracle's one-level bands;
  * the all-"a" path equals band 0 of the ordinary L-level oracle transform, bit for bit;
  * "a..a" followed by h / v / d equals its H / V / D bands of that level, bit for bit;
  * the costs are additive over a partition; the best-basis search never costs more than any basis it could have chosen;
  * the numpy restatement of the Haar tree (used for the 16384-node case) has the oracle's bits;
  * the basis validator rejects overlapping and incomplete sets;
  * the inverse from the full-depth basis and from a mixed basis gives the image back.
"""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import refwpt as R
from tests.helpers import band_err

CASES = [((64, 64), "db2", 3), ((33, 47), "haar", 3), ((61, 67), "db2", 3), ((40, 72), "coif1", 2)]


def _img(shape, dt):
    return np.random.RandomState(1).uniform(-100, 100, shape).astype(dt)


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("shape,wname,L", CASES)
def test_tree_matches_the_ordinary_transform(shape, wname, L, dt):
    x = _img(shape, dt)
    tr = R.tree(x, wname, L)
    assert len(tr) == L + 1 and [t.shape[0] for t in tr] == [4 ** d for d in range(L + 1)]
    O1 = orc.OracleWavelets(x, wname, 1)
    O1.forward()
    for q in range(4):
        assert np.array_equal(tr[1][q], O1.coeffs[q])
    O = orc.OracleWavelets(x, wname, L)
    O.forward()
    assert O.info.nlevels == L
    bands = O.coeffs  # [A_L, H1, V1, D1, ..., H_L, V_L, D_L]
    assert np.array_equal(tr[L][0], bands[0])
    for k in range(1, L + 1):  # level k (1 = finest): the node "a" * (k-1) + h / v / d of depth k
        for q, letter in ((1, "h"), (2, "v"), (3, "d")):
            d, i = R.index_of("a" * (k - 1) + letter)
            assert (d, i) == (k, q)
            assert np.array_equal(tr[d][i], bands[3 * (k - 1) + q]), (k, letter)


@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("shape,L", [((33, 47), 3), ((45, 51), 4), ((16, 16), 4)])
def test_numpy_haar_tree_has_the_oracle_bits(shape, L, dt):
    x = _img(shape, dt)
    a, b = R.tree(x, "haar", L), R.haar_tree(x, L)
    assert len(a) == len(b) == L + 1
    for ta, tb in zip(a, b):
        assert ta.dtype == tb.dtype and np.array_equal(ta, tb)


def test_paths_and_levels():
    assert R.index_of("") == (0, 0) and R.index_of("ahd") == (3, 7) and R.index_of("d") == (1, 3) and R.index_of("va") == (2, 8)
    for d in range(4):
        for i in range(4 ** d):
            assert R.index_of(R.path_of(d, i)) == (d, i)
    assert R.clamp_levels((96, 80), "db4", 9) == 3      # ilog2(80 / 7) = 3
    assert R.clamp_levels((256, 256), "haar", 9) == 7   # the cap
    assert R.clamp_levels((128, 128), "haar", 7) == 7
    assert R.clamp_levels((6, 64), "db4", 2) == 0       # too small for one level
    assert R.clamp_levels((64, 64), "db2", 0) == 1


@pytest.mark.parametrize("kind", ["l1", "shannon"])
def test_costs_are_additive_and_the_search_is_optimal(kind):
    yy, xx = np.mgrid[0:64, 0:64]
    x = 50 * np.sin(2 * np.pi * 19 * xx / 64) + 0.2 * (xx + yy) + 2 * np.random.RandomState(5).randn(64, 64)
    tr = R.tree(x, "db2", 3)
    costs = R.node_costs(tr, kind)
    # additive: the cost of a set of nodes is the sum over the nodes, whatever the grouping
    both = np.concatenate([tr[2][3].ravel(), tr[2][9].ravel()])
    assert abs(R.cost(both, kind) - (costs[2][3] + costs[2][9])) <= 1e-12 * (abs(costs[2][3]) + abs(costs[2][9]))
    basis, margin = R.best_basis(costs)
    R.check_basis(basis, 3)
    total = sum(costs[d][i] for d, i in basis)
    for other in ([(0, 0)], [(1, q) for q in range(4)], [(2, i) for i in range(16)], [(3, i) for i in range(64)],
                  [(1, 0)] + [(2, i) for i in range(4, 8)] + [(1, 2), (1, 3)]):
        R.check_basis(other, 3)
        assert total <= sum(costs[d][i] for d, i in other) * (1 + 1e-12) + 1e-9
    assert margin > 0


def test_basis_validator():
    R.check_basis([(0, 0)], 2)
    R.check_basis([(1, 0), (1, 1), (1, 2)] + [(2, i) for i in range(12, 16)], 2)
    with pytest.raises(ValueError):
        R.check_basis([(1, 0), (1, 1), (1, 2)], 2)                                     # incomplete
    with pytest.raises(ValueError):
        R.check_basis([(1, q) for q in range(4)] + [(2, 5)], 2)                         # a node below another
    with pytest.raises(ValueError):
        R.check_basis([(1, 0), (1, 0), (1, 1), (1, 2), (1, 3)], 2)                      # twice
    with pytest.raises(ValueError):
        R.check_basis([(3, 0)], 2)                                                      # outside the tree
    with pytest.raises(ValueError):
        R.check_basis([(1, 4)], 2)


@pytest.mark.parametrize("dt,bound", [(np.float32, 1e-5), (np.float64, 1e-12)])
@pytest.mark.parametrize("shape,wname,L", CASES)
def test_inverse_round_trip(shape, wname, L, dt, bound):
    x = _img(shape, dt)
    tr = R.tree(x, wname, L)
    full = {(L, i): tr[L][i] for i in range(4 ** L)}
    assert band_err(R.inverse(full, shape, wname, L), x) <= bound
    mixed = {(1, 0): tr[1][0], (1, 2): tr[1][2], (1, 3): tr[1][3]}
    mixed.update({(2, 4 + q): tr[2][4 + q] for q in range(4)})
    assert band_err(R.inverse(mixed, shape, wname, L), x) <= bound
