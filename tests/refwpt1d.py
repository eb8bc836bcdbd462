"""Reference of the batched 1-D wavelet packet transform for the tests: the packet tree of every row built by applying the oracle's
ONE-level batched 1-D transform (``OracleWavelets(node, wname, 1, ndim=1)``) to every node again, the inverse through ``set_coeff``
on a one-level instance, and the cost functions, the bottom-up best-basis search, the basis validator and the Gray-code frequency
order in numpy.  Nothing here touches pdwt_amd.

Layout: depth l is an array (Nr, 2^l, n_l); a node is ``tree[l][:, i]``, shape (Nr, n_l).  Node index: one digit per depth, a=0 d=1,
the first level the most significant; node i of depth l has the children 2i (a) and 2i + 1 (d) of depth l + 1, the oracle's band
order [A, D] of one level.  tests/test_refwpt1d_cpu.py pins it to the ordinary multi-level oracle transform.
"""
import numpy as np

from oracle import oracle as orc

MAX_LEVELS = 12
DIGITS = "ad"


def hlen_of(wname):
    if wname.lower() in ("haar", "db1", "bior1.1", "rbior1.1"):
        return 2
    return orc.filters(wname, np.float64)[0]


def clamp_levels(nc, wname, levels):
    """ilog2(Nc / (hlen - 1)) as in Wavelets with ndim = 1 (the rows do not count), and at most MAX_LEVELS; at least one level is asked for"""
    return max(0, min(max(int(levels), 1), orc.ilog2(int(nc) // (hlen_of(wname) - 1)), MAX_LEVELS))


def lengths(nc, levels):
    out = [int(nc)]
    for _ in range(levels):
        out.append((out[-1] + 1) // 2)
    return out


def index_of(path):
    i = 0
    for ch in path:
        i = 2 * i + DIGITS.index(ch)
    return len(path), i


def path_of(depth, idx):
    return "".join(DIGITS[(idx >> (depth - 1 - k)) & 1] for k in range(depth))


def frequency_order(depth):
    """f[r] = r ^ (r >> 1): the natural index of the node of frequency rank r"""
    r = np.arange(2 ** depth)
    return r ^ (r >> 1)


def split(node, wname):
    """[A, D] of one level of one node (Nr, n), in the node's precision"""
    W = orc.OracleWavelets(node, wname, 1, ndim=1)
    assert W.info.nlevels == 1, (node.shape, wname)
    W.forward()
    return W.coeffs


def merge(children, shape, wname):
    """the node of `shape` = (Nr, n) whose one-level bands are `children` = [A, D]"""
    W = orc.OracleWavelets(np.zeros(shape, children[0].dtype), wname, 1, ndim=1)
    assert W.info.nlevels == 1, (shape, wname)
    for k in range(2):
        W.set_coeff(children[k], k)
    W.inverse()
    return W.get_image()


def tree(rows, wname, levels):
    """[array (Nr, 2^l, n_l) for depth l = 0 .. L], L = the clamped depth; computed in the precision of `rows`"""
    rows = np.ascontiguousarray(rows)
    assert rows.ndim == 2
    L = clamp_levels(rows.shape[1], wname, levels)
    assert L >= 1
    out = [rows[:, None, :].copy()]
    for _ in range(L):
        t = out[-1]
        kids = [c for i in range(t.shape[1]) for c in split(np.ascontiguousarray(t[:, i]), wname)]
        out.append(np.ascontiguousarray(np.stack(kids, axis=1)))
    return out


def haar_tree(rows, levels):
    """`tree(rows, "haar", levels)` with the reference's 1-D Haar level restated in numpy over all nodes of a depth at once: the same
    IEEE operations in the same order -- s * (x0 +- x1) with s the double 0.70710678118654746, the product evaluated in double and
    rounded once, x1 clamped to the last sample of an odd node -- so the same bits (pinned in tests/test_refwpt1d_cpu.py); for the deep
    trees whose thousands of tiny nodes would cost one oracle call each."""
    rows = np.ascontiguousarray(rows)
    L = clamp_levels(rows.shape[1], "haar", levels)
    out, s, dt = [rows[:, None, :].copy()], np.float64(0.70710678118654746), rows.dtype
    for _ in range(L):
        t = out[-1]
        n = t.shape[2]
        i0 = np.arange(0, n, 2)
        i1 = np.minimum(i0 + 1, n - 1)
        a, b = t[:, :, i0], t[:, :, i1]
        lo = (s * (a + b).astype(np.float64)).astype(dt)
        hi = (s * (a - b).astype(np.float64)).astype(dt)
        out.append(np.ascontiguousarray(np.stack([lo, hi], axis=2).reshape(t.shape[0], 2 * t.shape[1], len(i0))))
    return out


def inverse(nodes, shape, wname, levels):
    """The batch from a basis given as {(depth, idx): array (Nr, n_depth)}: climbs one depth at a time, merging two siblings into their parent."""
    check_basis(nodes.keys(), levels)
    have = {k: np.asarray(v) for k, v in nodes.items()}
    n = lengths(shape[1], levels)
    for d in range(levels, 0, -1):
        for i in sorted({k[1] // 2 for k in have if k[0] == d}):
            have[(d - 1, i)] = merge([have.pop((d, 2 * i + q)) for q in range(2)], (shape[0], n[d - 1]), wname)
    return have[(0, 0)]


# ---- costs and bases (float64) -------------------------------------------------------------------------
def cost(x, kind):
    """additive cost of a set of coefficients: "l1" = sum |c|;  "shannon" = -sum c^2 ln c^2 over the non-zero c"""
    x = np.asarray(x, np.float64).ravel()
    if kind == "l1":
        return float(np.abs(x).sum())
    assert kind == "shannon", kind
    v2 = x * x
    v2 = v2[v2 > 0]
    return float(-(v2 * np.log(v2)).sum())


def node_costs(tr, kind, per_row=False):
    """per depth: the costs of the 2^l nodes summed over the rows in row order (per_row: the (Nr, 2^l) costs of every row's node)"""
    out = []
    for lev in tr:
        pr = np.array([[cost(lev[r, i], kind) for i in range(lev.shape[1])] for r in range(lev.shape[0])], np.float64)
        if per_row:
            out.append(pr)
        else:
            s = np.zeros(lev.shape[1], np.float64)
            for r in range(lev.shape[0]):
                s = s + pr[r]
            out.append(s)
    return out


def best_basis(costs):
    """Bottom-up search over per-depth (summed) cost arrays: a parent is kept when its cost is <= the sum of its two children's best
    costs.  Returns (sorted list of (depth, idx), the smallest relative margin |parent - children| / max(|parent|, |children|))."""
    L = len(costs) - 1
    best = [np.array(c, np.float64) for c in costs]
    keep = [np.ones(len(c), bool) for c in costs]
    margin = np.inf
    for d in range(L - 1, -1, -1):
        for i in range(2 ** d):
            below = best[d + 1][2 * i] + best[d + 1][2 * i + 1]
            margin = min(margin, abs(best[d][i] - below) / max(abs(best[d][i]), abs(below), 1e-300))
            if not best[d][i] <= below:
                keep[d][i] = False
                best[d][i] = below
    basis, todo = [], [(0, 0)]
    while todo:
        d, i = todo.pop()
        if keep[d][i]:
            basis.append((d, i))
        else:
            todo += [(d + 1, 2 * i + q) for q in range(2)]
    return sorted(basis), margin


def check_basis(nodes, levels):
    """ValueError unless every root-to-leaf path of a tree of `levels` depths meets exactly one of `nodes` ((depth, idx) pairs)"""
    leaf = np.zeros(2 ** levels, np.int64)
    for d, i in nodes:
        if not (0 <= d <= levels and 0 <= i < 2 ** d):
            raise ValueError("node (%d, %d) outside the tree" % (d, i))
        leaf[i * 2 ** (levels - d):(i + 1) * 2 ** (levels - d)] += 1
    if (leaf > 1).any():
        raise ValueError("overlapping nodes")
    if (leaf < 1).any():
        raise ValueError("incomplete basis")
