"""Reference of the 2-D wavelet packet transform for the tests: the packet tree built by applying the oracle's ONE-level 2-D transform
(``OracleWavelets(node, wname, 1)``) to every node again, the inverse through ``set_coeff`` on a one-level instance, and the cost
functions, the bottom-up best-basis search and the basis validator in float64 numpy.  Nothing here touches pdwt_amd.

Node index: one digit per depth, a=0 h=1 v=2 d=3, the first level the most significant; node i of depth l has the children
4i .. 4i+3 of depth l + 1, in the oracle's band order [A, H, V, D] of one level.  tests/test_refwpt_cpu.py pins it to the ordinary
multi-level oracle transform.
"""
import numpy as np

from oracle import oracle as orc

MAX_LEVELS = 7
DIGITS = "ahvd"


def hlen_of(wname):
    if wname.lower() in ("haar", "db1", "bior1.1", "rbior1.1"):
        return 2
    return orc.filters(wname, np.float64)[0]


def clamp_levels(shape, wname, levels):
    """ilog2(min(Nr, Nc) / (hlen - 1)) as in Wavelets, and at most MAX_LEVELS; at least one level is asked for"""
    return max(0, min(max(int(levels), 1), orc.ilog2(min(shape) // (hlen_of(wname) - 1)), MAX_LEVELS))


def index_of(path):
    i = 0
    for ch in path:
        i = 4 * i + DIGITS.index(ch)
    return len(path), i


def path_of(depth, idx):
    return "".join(DIGITS[(idx >> (2 * (depth - 1 - k))) & 3] for k in range(depth))


def split(node, wname):
    """[A, H, V, D] of one level of one node, in the node's precision"""
    W = orc.OracleWavelets(node, wname, 1)
    assert W.info.nlevels == 1, (node.shape, wname)
    W.forward()
    return W.coeffs


def merge(children, shape, wname):
    """the node of `shape` whose one-level bands are `children` = [A, H, V, D]"""
    W = orc.OracleWavelets(np.zeros(shape, children[0].dtype), wname, 1)
    assert W.info.nlevels == 1, (shape, wname)
    for k in range(4):
        W.set_coeff(children[k], k)
    W.inverse()
    return W.get_image()


def tree(img, wname, levels):
    """[array (4^l, nr_l, nc_l) for depth l = 0 .. L], L = the clamped depth; computed in the precision of `img`"""
    img = np.ascontiguousarray(img)
    L = clamp_levels(img.shape, wname, levels)
    assert L >= 1
    out = [img[None].copy()]
    for _ in range(L):
        out.append(np.stack([c for node in out[-1] for c in split(node, wname)]))
    return out


def haar_tree(img, levels):
    """`tree(img, "haar", levels)` with the clamped 2x2 butterfly restated in numpy over all nodes of a depth at once: the same IEEE
    operations in the same order, so the same bits (pinned in tests/test_refwpt_cpu.py) -- for the deep trees whose thousands of tiny
    nodes would cost one oracle call each."""
    img = np.ascontiguousarray(img)
    L = clamp_levels(img.shape, "haar", levels)
    out, h = [img[None].copy()], img.dtype.type(0.5)
    for _ in range(L):
        t = out[-1]
        nr, nc = t.shape[1:]
        y0, x0 = np.arange(0, nr, 2), np.arange(0, nc, 2)
        y1, x1 = np.minimum(y0 + 1, nr - 1), np.minimum(x0 + 1, nc - 1)
        a, b, c, d = t[:, y0][:, :, x0], t[:, y0][:, :, x1], t[:, y1][:, :, x0], t[:, y1][:, :, x1]
        kids = [h * ((a + c) + (b + d)), h * ((a - c) + (b - d)), h * ((a + c) - (b + d)), h * ((a - c) - (b - d))]  # A, H, V, D
        out.append(np.stack(kids, axis=1).reshape(4 * t.shape[0], len(y0), len(x0)))
    return out


def inverse(nodes, shape, wname, levels):
    """The image from a basis given as {(depth, idx): array}: climbs one depth at a time, merging four siblings into their parent."""
    check_basis(nodes.keys(), levels)
    have = {k: np.asarray(v) for k, v in nodes.items()}
    shapes = [tuple(shape)]
    for _ in range(levels):
        shapes.append(((shapes[-1][0] + 1) // 2, (shapes[-1][1] + 1) // 2))
    for d in range(levels, 0, -1):
        for i in sorted({k[1] // 4 for k in have if k[0] == d}):
            have[(d - 1, i)] = merge([have.pop((d, 4 * i + q)) for q in range(4)], shapes[d - 1], wname)
    return have[(0, 0)]


# ---- costs and bases (float64) -------------------------------------------------------------------------
def cost(x, kind):
    """additive cost of one node: "l1" = sum |c|;  "shannon" = -sum c^2 ln c^2 over the non-zero c"""
    x = np.asarray(x, np.float64).ravel()
    if kind == "l1":
        return float(np.abs(x).sum())
    assert kind == "shannon", kind
    v2 = x * x
    v2 = v2[v2 > 0]
    return float(-(v2 * np.log(v2)).sum())


def node_costs(tr, kind):
    return [np.array([cost(n, kind) for n in lev], np.float64) for lev in tr]


def best_basis(costs):
    """Bottom-up search over per-depth cost arrays: a parent is kept when its cost is <= the sum of its children's best costs.
    Returns (sorted list of (depth, idx), the smallest relative margin |parent - children| / max(|parent|, |children|) of any decision)."""
    L = len(costs) - 1
    best = [np.array(c, np.float64) for c in costs]
    keep = [np.ones(len(c), bool) for c in costs]
    margin = np.inf
    for d in range(L - 1, -1, -1):
        for i in range(4 ** d):
            c = best[d + 1][4 * i:4 * i + 4]
            below = ((c[0] + c[1]) + c[2]) + c[3]
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
            todo += [(d + 1, 4 * i + q) for q in range(4)]
    return sorted(basis), margin


def check_basis(nodes, levels):
    """ValueError unless every root-to-leaf path of a tree of `levels` depths meets exactly one of `nodes` ((depth, idx) pairs)"""
    leaf = np.zeros(4 ** levels, np.int64)
    for d, i in nodes:
        if not (0 <= d <= levels and 0 <= i < 4 ** d):
            raise ValueError("node (%d, %d) outside the tree" % (d, i))
        leaf[i * 4 ** (levels - d):(i + 1) * 4 ** (levels - d)] += 1
    if (leaf > 1).any():
        raise ValueError("overlapping nodes")
    if (leaf < 1).any():
        raise ValueError("incomplete basis")
