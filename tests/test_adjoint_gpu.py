"""The adjoint operators of the boundary-mode transforms on the GPU (include/pdwt_hip.h "Adjoints of the boundary-mode DWT") and the
differentiable functions of pdwt_amd.functional, against the float64 reference of tests/refadj.py.

Bounds: 1e-5 (float32) / 1e-12 (float64) of max|ref| for every case -- the family's; tests/test_refadj_cpu.py measures the float32
error of the kernels' order on each case (at most 3.1e-7, the 40-tap `constant` case 2.4e-7: below a quarter of the bound, so no
case has a bound of its own).  The operator identity <W x, c> = <x, W^T c> is asked to 1e-12 ||W x|| ||c|| in float64."""
import ctypes as C
import functools

import numpy as np
import pytest

import pdwt_amd
from pdwt_amd import _native as nat
from tests import refadj as A
from tests import refext as R
from tests.cabi_arena import Arena, Region

pytestmark = pytest.mark.gpu

BOUND = {"f32": 1e-5, "f64": 1e-12}
DT = {"f32": np.float32, "f64": np.float64}
B = 3


class Dev:
    """device buffers of one test through the library's own allocator"""

    def __init__(self):
        self.L = pdwt_amd.hip()
        self.ptrs = []

    def empty(self, elems, dt):
        p = self.L.pdwt_malloc(max(int(elems), 1) * np.dtype(dt).itemsize)
        assert p
        self.ptrs.append(p)
        return p

    def up(self, arr):
        a = np.ascontiguousarray(arr)
        p = self.empty(a.size, a.dtype)
        assert self.L.pdwt_memcpy_h2d(p, a.ctypes.data, a.nbytes) == 0
        return p

    def down(self, p, shape, dt):
        out = np.empty(shape, dt)
        assert self.L.pdwt_sync() == 0
        assert self.L.pdwt_memcpy_d2h(out.ctypes.data, p, out.nbytes) == 0
        return out

    def free(self):
        self.L.pdwt_sync()
        for p in self.ptrs:
            self.L.pdwt_free(p)
        self.ptrs = []


@pytest.fixture
def dev():
    d = Dev()
    yield d
    d.free()


def bank(sfx, wname):
    L = pdwt_amd.hip()
    f = (nat.Filters32 if sfx == "f32" else nat.Filters64)()
    f.hlen = getattr(L, "pdwt_compute_filters_separable_" + sfx)(wname.encode(), 0, C.byref(f))
    assert f.hlen >= 2
    return f


def fn(name, sfx):
    return getattr(pdwt_amd.hip(), "pdwt_%s_%s" % (name, sfx))


def table(ptrs):
    return (C.c_void_p * len(ptrs))(*ptrs)


# ---- references, computed once ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cot2(k):
    shape, w, L, _ = A.CASES_2D[k]
    return tuple(A.cotangent(R.band_shapes(shape, R.bank(w)[0], L), (B,), 10 + k))


@functools.lru_cache(maxsize=None)
def ref2(k, mode):
    shape, w, L, _ = A.CASES_2D[k]
    r = A.wavedec2_adjoint(list(cot2(k)), shape, w, mode)
    r.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def img2(k):
    return A.cotangent([A.CASES_2D[k][0]], (B,), 40 + k)[0]


@functools.lru_cache(maxsize=None)
def cot1(k):
    (rows, n), w, L, _, _ = A.CASES_1D[k]
    ns = A.lengths(n, R.bank(w)[0], L)
    return tuple(A.cotangent([(ns[L],)] + [(v,) for v in ns[1:]], (rows,), 20 + k))


@functools.lru_cache(maxsize=None)
def ref1(k, mode):
    (rows, n), w, L, _, _ = A.CASES_1D[k]
    r = A.wavedec1_adjoint(list(cot1(k)), n, w, mode)
    r.setflags(write=False)
    return r


CASES2 = [(k, m) for k, c in enumerate(A.CASES_2D) for m in c[3]]
CASES1 = [(k, m) for k, c in enumerate(A.CASES_1D) for m in c[3]]


def _id2(p):
    s, w, L, _ = A.CASES_2D[p[0]]
    return "%dx%d-%s-L%d-%s" % (s[0], s[1], w, L, p[1])


def _id1(p):
    s, w, L, _, form = A.CASES_1D[p[0]]
    return "%dx%d-%s-L%d-%s-%s" % (s[0], s[1], w, L, form, p[1])


# ---- 2-D forward adjoint ---------------------------------------------------------------------------------------------------------------
def run_adj2(dev, sfx, f, band_ptrs, out, nimg, shape, levels, mode, shapes, first=0, level_driver=False):
    """one call on images first .. first + nimg - 1 of the uploaded stacks"""
    L, dt = dev.L, np.dtype(DT[sfx])
    nr, nc = shape
    ptrs = [p + first * s[0] * s[1] * dt.itemsize for p, s in zip(band_ptrs, shapes)]
    dst = out + first * nr * nc * dt.itemsize
    m = R.MODES.index(mode)
    if level_driver:
        assert levels == 1
        tmp = dev.empty(nimg * ((nr + 2 * f.hlen - 3) * (nc + 2 * f.hlen - 3) - nr * nc), dt)
        rc = fn("ext2db_forward_adjoint_level", sfx)(dst, *ptrs, nimg, nr, nc, m, C.byref(f), tmp)
    else:
        elems = L.pdwt_ext2db_adjoint_tmp_elems(nimg, nr, nc, f.hlen, levels, dt.itemsize)
        assert elems > 0
        rc = fn("ext2db_forward_adjoint", sfx)(dst, table(ptrs), nimg, nr, nc, levels, m, C.byref(f), dev.empty(elems, dt))
    assert rc == 0, rc
    return rc


@pytest.mark.parametrize("sfx", ["f32", "f64"])
@pytest.mark.parametrize("case", CASES2, ids=_id2)
def test_forward_adjoint_2d(case, sfx, dev):
    k, mode = case
    shape, w, levels, _ = A.CASES_2D[k]
    dt = DT[sfx]
    f = bank(sfx, w)
    shapes = R.band_shapes(shape, f.hlen, levels)
    c = [b.astype(dt) for b in cot2(k)]
    ptrs = [dev.up(b) for b in c]
    lvl = levels == 1 and shape == (7, 7)
    out = dev.up(np.full((B,) + shape, 777, dt))
    run_adj2(dev, sfx, f, ptrs, out, B, shape, levels, mode, shapes, level_driver=lvl)
    x = dev.down(out, (B,) + shape, dt)
    e = A.rel_err(x, ref2(k, mode))
    print("adjoint 2-D %s %s: %.3e" % (_id2(case), sfx, e))
    assert e <= BOUND[sfx], e
    # the cotangents are intact
    for p, b in zip(ptrs, c):
        assert np.array_equal(dev.down(p, b.shape, dt), b)
    # a second run gives the same bits; so do three calls on one image each
    out2 = dev.up(np.full((B,) + shape, 555, dt))
    run_adj2(dev, sfx, f, ptrs, out2, B, shape, levels, mode, shapes, level_driver=lvl)
    assert np.array_equal(dev.down(out2, (B,) + shape, dt).view(np.uint8), x.view(np.uint8))
    out3 = dev.up(np.full((B,) + shape, 333, dt))
    for b in range(B):
        run_adj2(dev, sfx, f, ptrs, out3, 1, shape, levels, mode, shapes, first=b, level_driver=lvl)
    assert np.array_equal(dev.down(out3, (B,) + shape, dt).view(np.uint8), x.view(np.uint8))


@pytest.mark.parametrize("sfx", ["f32", "f64"])
@pytest.mark.parametrize("k", range(len(A.CASES_2D)), ids=lambda k: _id2((k, "inv")))
def test_inverse_adjoint_2d(k, sfx, dev):
    shape, w, levels, _ = A.CASES_2D[k]
    dt = DT[sfx]
    f = bank(sfx, w)
    shapes = R.band_shapes(shape, f.hlen, levels)
    y = img2(k).astype(dt)
    ref = A.waverec2_adjoint(img2(k), w, levels)
    src = dev.up(y)
    ptrs = [dev.up(np.full((B,) + s, 777, dt)) for s in shapes]
    L = dev.L
    tmp = L.pdwt_ext2db_tmp_elems(B, shape[0], shape[1], f.hlen, levels, np.dtype(dt).itemsize)
    rc = fn("ext2db_inverse_adjoint", sfx)(src, table(ptrs), B, shape[0], shape[1], levels, C.byref(f), dev.empty(tmp, dt) if tmp else None)
    assert rc == L.pdwt_ext2db_fused(shape[0], shape[1], f.hlen, levels, np.dtype(dt).itemsize), rc  # the code of the forward path that ran
    for n, (p, s, r) in enumerate(zip(ptrs, shapes, ref)):
        e = A.rel_err(dev.down(p, (B,) + s, dt), r)
        print("inverse adjoint 2-D %s %s band %d: %.3e" % (_id2((k, "inv")), sfx, n, e))
        assert e <= BOUND[sfx], (n, e)
    assert np.array_equal(dev.down(src, y.shape, dt), y)


# ---- 1-D -----------------------------------------------------------------------------------------------------------------------
def chain_adj1(dev, sfx, f, ptrs, rows, ns, mode):
    """the level entries one after the other, coarse to fine; returns the pointer of the result"""
    dt = np.dtype(DT[sfx])
    levels = len(ns) - 1
    tmp = dev.empty(rows * (2 * f.hlen - 3), dt)
    a = ptrs[0]
    for l in range(levels, 0, -1):
        out = dev.empty(rows * ns[l - 1], dt)
        assert fn("ext1d_forward_adjoint_level", sfx)(out, a, ptrs[l], rows, ns[l - 1], R.MODES.index(mode), C.byref(f), tmp) == 0
        a = out
    return a


@pytest.mark.parametrize("sfx", ["f32", "f64"])
@pytest.mark.parametrize("case", CASES1, ids=_id1)
def test_forward_adjoint_1d(case, sfx, dev):
    k, mode = case
    (rows, n), w, levels, _, form = A.CASES_1D[k]
    dt = DT[sfx]
    f = bank(sfx, w)
    ns = A.lengths(n, f.hlen, levels)
    c = [b.astype(dt) for b in cot1(k)]
    ptrs = [dev.up(b) for b in c]
    L = dev.L
    if form == "level-driver":
        out = chain_adj1(dev, sfx, f, ptrs, rows, ns, mode)
    else:
        out = dev.up(np.full((rows, n), 777, dt))
        elems = L.pdwt_ext1d_adjoint_tmp_elems(rows, n, f.hlen, levels, np.dtype(dt).itemsize)
        assert (elems == 0) == (form == "fused")
        rc = fn("ext1d_forward_adjoint", sfx)(out, table(ptrs), rows, n, levels, R.MODES.index(mode), C.byref(f), dev.empty(elems, dt) if elems else None)
        assert rc == (1 if form == "fused" else 0), rc
    x = dev.down(out, (rows, n), dt)
    e = A.rel_err(x, ref1(k, mode))
    print("adjoint 1-D %s %s: %.3e" % (_id1(case), sfx, e))
    assert e <= BOUND[sfx], e
    for p, b in zip(ptrs, c):
        assert np.array_equal(dev.down(p, b.shape, dt), b)
    if form != "level-driver":
        # the chain of level entries gives the same bits as the whole-transform entry, whichever form it ran; so does a second run
        y = dev.down(chain_adj1(dev, sfx, f, ptrs, rows, ns, mode), (rows, n), dt)
        assert np.array_equal(y.view(np.uint8), x.view(np.uint8))
        out2 = dev.up(np.full((rows, n), 555, dt))
        elems = L.pdwt_ext1d_adjoint_tmp_elems(rows, n, f.hlen, levels, np.dtype(dt).itemsize)
        assert fn("ext1d_forward_adjoint", sfx)(out2, table(ptrs), rows, n, levels, R.MODES.index(mode), C.byref(f), dev.empty(elems, dt) if elems else None) >= 0
        assert np.array_equal(dev.down(out2, (rows, n), dt).view(np.uint8), x.view(np.uint8))


@pytest.mark.parametrize("sfx", ["f32", "f64"])
@pytest.mark.parametrize("k", range(len(A.CASES_1D)), ids=lambda k: _id1((k, "inv")))
def test_inverse_adjoint_1d(k, sfx, dev):
    (rows, n), w, levels, _, _ = A.CASES_1D[k]
    dt = DT[sfx]
    f = bank(sfx, w)
    ns = A.lengths(n, f.hlen, levels)
    y64 = A.cotangent([(n,)], (rows,), 60 + k)[0]
    ref = A.waverec1_adjoint(y64, w, levels)
    y = y64.astype(dt)
    src = dev.up(y)
    lens = [ns[levels]] + ns[1:]
    ptrs = [dev.up(np.full((rows, v), 777, dt)) for v in lens]
    L = dev.L
    tmp = L.pdwt_ext1d_tmp_elems(rows, n, f.hlen, levels, np.dtype(dt).itemsize)
    rc = fn("ext1d_inverse_adjoint", sfx)(src, table(ptrs), rows, n, levels, C.byref(f), dev.empty(tmp, dt) if tmp else None)
    assert rc == L.pdwt_ext1d_fused(n, f.hlen, levels, np.dtype(dt).itemsize), rc
    for b, (p, v, r) in enumerate(zip(ptrs, lens, ref)):
        e = A.rel_err(dev.down(p, (rows, v), dt), r)
        print("inverse adjoint 1-D %s %s band %d: %.3e" % (_id1((k, "inv")), sfx, b, e))
        assert e <= BOUND[sfx], (b, e)
    assert np.array_equal(dev.down(src, y.shape, dt), y)


# ---- the operator identity on the device, float64 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,w,levels,mode", [((61, 67), "db4", 2, "symmetric"), ((33, 47), "haar", 3, "reflect"), ((48, 48), "bior2.2", 2, "periodic"),
                                                 ((13, 18), "db2", 2, "constant"), ((96, 80), "db20", 1, "constant")])
def test_operator_identity_2d(shape, w, levels, mode, dev):
    sfx, dt, L = "f64", np.float64, dev.L
    f = bank(sfx, w)
    shapes = R.band_shapes(shape, f.hlen, levels)
    rs = np.random.RandomState(8)
    x = rs.standard_normal((B,) + shape)
    c = [rs.standard_normal((B,) + s) for s in shapes]
    nr, nc = shape
    m = R.MODES.index(mode)
    # W x and W^T c
    wx = [dev.empty(B * s[0] * s[1], dt) for s in shapes]
    tmp = L.pdwt_ext2db_tmp_elems(B, nr, nc, f.hlen, levels, 8)
    assert fn("ext2db_forward", sfx)(dev.up(x), table(wx), B, nr, nc, levels, m, C.byref(f), dev.empty(tmp, dt) if tmp else None) >= 0
    Wx = [dev.down(p, (B,) + s, dt) for p, s in zip(wx, shapes)]
    cp = [dev.up(b) for b in c]
    out = dev.empty(B * nr * nc, dt)
    run_adj2(dev, sfx, f, cp, out, B, shape, levels, mode, shapes)
    Wtc = dev.down(out, (B,) + shape, dt)
    lhs, rhs = sum(float((u * v).sum()) for u, v in zip(Wx, c)), float((x * Wtc).sum())
    scale = np.sqrt(sum(float((u * u).sum()) for u in Wx)) * np.sqrt(sum(float((v * v).sum()) for v in c))
    print("<Wx, c> - <x, W^T c> = %.3e of %.3e" % (lhs - rhs, scale))
    assert abs(lhs - rhs) <= 1e-12 * scale
    # S c and S^T x
    sc = dev.empty(B * nr * nc, dt)
    assert fn("ext2db_inverse", sfx)(sc, table(cp), B, nr, nc, levels, C.byref(f), dev.empty(tmp, dt) if tmp else None) >= 0
    Sc = dev.down(sc, (B,) + shape, dt)
    st = [dev.empty(B * s[0] * s[1], dt) for s in shapes]
    assert fn("ext2db_inverse_adjoint", sfx)(dev.up(x), table(st), B, nr, nc, levels, C.byref(f), dev.empty(tmp, dt) if tmp else None) >= 0
    Stx = [dev.down(p, (B,) + s, dt) for p, s in zip(st, shapes)]
    lhs, rhs = float((Sc * x).sum()), sum(float((u * v).sum()) for u, v in zip(c, Stx))
    scale = np.sqrt(float((Sc * Sc).sum())) * np.sqrt(float((x * x).sum()))
    print("<Sc, x> - <c, S^T x> = %.3e of %.3e" % (lhs - rhs, scale))
    assert abs(lhs - rhs) <= 1e-12 * scale


@pytest.mark.parametrize("rows,n,w,levels,mode", [(2, 4099, "db4", 5, "periodic"), (5, 77, "haar", 3, "reflect"), (2, 40037, "db4", 3, "symmetric"),
                                                  (2, 96, "db20", 1, "constant")])
def test_operator_identity_1d(rows, n, w, levels, mode, dev):
    sfx, dt, L = "f64", np.float64, dev.L
    f = bank(sfx, w)
    ns = A.lengths(n, f.hlen, levels)
    lens = [ns[levels]] + ns[1:]
    rs = np.random.RandomState(9)
    x = rs.standard_normal((rows, n))
    c = [rs.standard_normal((rows, v)) for v in lens]
    m = R.MODES.index(mode)
    tmp = L.pdwt_ext1d_tmp_elems(rows, n, f.hlen, levels, 8)
    wx = [dev.empty(rows * v, dt) for v in lens]
    assert fn("ext1d_forward", sfx)(dev.up(x), table(wx), rows, n, levels, m, C.byref(f), dev.empty(tmp, dt) if tmp else None) >= 0
    Wx = [dev.down(p, (rows, v), dt) for p, v in zip(wx, lens)]
    cp = [dev.up(b) for b in c]
    out = dev.empty(rows * n, dt)
    atmp = L.pdwt_ext1d_adjoint_tmp_elems(rows, n, f.hlen, levels, 8)
    assert fn("ext1d_forward_adjoint", sfx)(out, table(cp), rows, n, levels, m, C.byref(f), dev.empty(atmp, dt) if atmp else None) >= 0
    Wtc = dev.down(out, (rows, n), dt)
    lhs, rhs = sum(float((u * v).sum()) for u, v in zip(Wx, c)), float((x * Wtc).sum())
    scale = np.sqrt(sum(float((u * u).sum()) for u in Wx)) * np.sqrt(sum(float((v * v).sum()) for v in c))
    print("<Wx, c> - <x, W^T c> = %.3e of %.3e" % (lhs - rhs, scale))
    assert abs(lhs - rhs) <= 1e-12 * scale
    sc = dev.empty(rows * n, dt)
    assert fn("ext1d_inverse", sfx)(sc, table(cp), rows, n, levels, C.byref(f), dev.empty(tmp, dt) if tmp else None) >= 0
    Sc = dev.down(sc, (rows, n), dt)
    st = [dev.empty(rows * v, dt) for v in lens]
    assert fn("ext1d_inverse_adjoint", sfx)(dev.up(x), table(st), rows, n, levels, C.byref(f), dev.empty(tmp, dt) if tmp else None) >= 0
    Stx = [dev.down(p, (rows, v), dt) for p, v in zip(st, lens)]
    lhs, rhs = float((Sc * x).sum()), sum(float((u * v).sum()) for u, v in zip(c, Stx))
    scale = np.sqrt(float((Sc * Sc).sum())) * np.sqrt(float((x * x).sum()))
    assert abs(lhs - rhs) <= 1e-12 * scale


# ---- guard zones and misaligned caller buffers: the level drivers ------------------------------------------------------------------------------
NAMES = ("a", "h", "v", "d")


@pytest.mark.parametrize("sfx", ["f32", "f64"])
@pytest.mark.parametrize("shape,wname,mode", [((61, 67), "db4", "symmetric"), ((33, 47), "haar", "reflect")])
def test_2d_level_driver_on_guarded_misaligned_buffers(shape, wname, mode, sfx):
    L = pdwt_amd.hip()
    dt = np.dtype(DT[sfx])
    f = bank(sfx, wname)
    hlen = f.hlen
    nr, nc = shape
    hr, hc = (nr + hlen - 1) // 2, (nc + hlen - 1) // 2
    c = A.cotangent([(hr, hc)] * 4, (2,), 31)
    ref = A.dwt2_adjoint(c, shape, R.bank(wname)[1], mode)
    frame = 2 * ((nr + 2 * hlen - 3) * (nc + 2 * hlen - 3) - nr * nc)
    regions = [Region("x", 2 * nr * nc, dt, "out", 1)] + [Region(n, 2 * hr * hc, dt, "in", k + 1) for k, n in enumerate(NAMES)] + [Region("tmp", frame, dt, "scratch", 3)]
    arena = Arena(L, regions, {n: b.astype(dt) for n, b in zip(NAMES, c)})
    adj = fn("ext2db_forward_adjoint_level", sfx)
    try:
        bands = [arena.ptr(n) for n in NAMES]
        x, tmp, fp = arena.ptr("x"), arena.ptr("tmp"), C.byref(f)
        # refusals first: nothing may be touched (x still holds the fill pattern afterwards)
        assert adj(x, *bands, 2, nr, nc, 5, fp, tmp) == -1 and adj(x, *bands, 2, nr, nc, -1, fp, tmp) == -1
        assert adj(x, *bands, 0, nr, nc, 2, fp, tmp) == -1 and adj(x, *bands, 65536, nr, nc, 2, fp, tmp) == -1
        if hlen > 2:
            assert adj(x, *bands, 2, hlen - 2, nc, 2, fp, tmp) == -1 and adj(x, *bands, 2, nr, hlen - 2, 2, fp, tmp) == -1
        assert adj(None, *bands, 2, nr, nc, 2, fp, tmp) == -1 and adj(x, *bands, 2, nr, nc, 2, fp, None) == -1 and adj(x, *bands, 2, nr, nc, 2, None, tmp) == -1
        arena.by_name["x"].role = arena.by_name["tmp"].role = "in"
        arena.check("refusals %s %s" % (wname, sfx))
        arena.by_name["x"].role, arena.by_name["tmp"].role = "out", "scratch"
        assert adj(x, *bands, 2, nr, nc, R.MODES.index(mode), fp, tmp) == 0
        img = arena.check("adjoint level %s %s %s" % (wname, mode, sfx))
        e = A.rel_err(arena.get(img, "x", shape=(2, nr, nc)), ref)
        print("guarded 2-D level adjoint %s %s %s: %.3e" % (wname, mode, sfx, e))
        assert e <= BOUND[sfx], e
    finally:
        arena.free()


@pytest.mark.parametrize("sfx", ["f32", "f64"])
@pytest.mark.parametrize("rows,n,wname,mode", [(3, 2051, "db4", "symmetric"), (7, 33, "haar", "reflect")])
def test_1d_level_driver_on_guarded_misaligned_buffers(rows, n, wname, mode, sfx):
    L = pdwt_amd.hip()
    dt = np.dtype(DT[sfx])
    f = bank(sfx, wname)
    hlen = f.hlen
    N = (n + hlen - 1) // 2
    c = A.cotangent([(N,), (N,)], (rows,), 32)
    taps = R.bank(wname)[1]
    ref = A.analysis_adjoint(c[0], c[1], taps["L"], taps["H"], n, mode)
    regions = [Region("x", rows * n, dt, "out", 1), Region("a", rows * N, dt, "in", 1), Region("d", rows * N, dt, "in", 2),
               Region("tmp", rows * (2 * hlen - 3), dt, "scratch", 3)]
    arena = Arena(L, regions, {"a": c[0].astype(dt), "d": c[1].astype(dt)})
    adj = fn("ext1d_forward_adjoint_level", sfx)
    try:
        x, a, d, tmp, fp = arena.ptr("x"), arena.ptr("a"), arena.ptr("d"), arena.ptr("tmp"), C.byref(f)
        assert adj(x, a, d, rows, n, 5, fp, tmp) == -1 and adj(x, a, d, rows, n, -1, fp, tmp) == -1 and adj(x, a, d, 0, n, 2, fp, tmp) == -1
        if hlen > 2:
            assert adj(x, a, d, rows, hlen - 2, 2, fp, tmp) == -1
        assert adj(None, a, d, rows, n, 2, fp, tmp) == -1 and adj(x, a, d, rows, n, 2, fp, None) == -1 and adj(x, a, d, rows, n, 2, None, tmp) == -1
        arena.by_name["x"].role = arena.by_name["tmp"].role = "in"
        arena.check("refusals %s %s" % (wname, sfx))
        arena.by_name["x"].role, arena.by_name["tmp"].role = "out", "scratch"
        assert adj(x, a, d, rows, n, R.MODES.index(mode), fp, tmp) == 0
        img = arena.check("adjoint level %s %s %s" % (wname, mode, sfx))
        e = A.rel_err(arena.get(img, "x", shape=(rows, n)), ref)
        print("guarded 1-D level adjoint %s %s %s: %.3e" % (wname, mode, sfx, e))
        assert e <= BOUND[sfx], e
    finally:
        arena.free()


# ---- autograd ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


def _randn(torch, shape, seed, dtype=None, grad=True):
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(shape, generator=g, dtype=torch.float64).to(dtype or torch.float64).cuda()
    return t.requires_grad_(grad)


@pytest.mark.parametrize("lead,shape,w,levels,mode", [((2,), (9, 11), "db2", 2, "symmetric"), ((), (7, 8), "bior2.2", 1, "periodic")])
def test_gradcheck_dwt2_and_idwt2(lead, shape, w, levels, mode, torch):
    F = pdwt_amd.functional
    x = _randn(torch, lead + shape, 1)
    assert torch.autograd.gradcheck(lambda t: tuple(F.dwt2(t, w, levels, mode)), (x,), eps=1e-6, atol=1e-7, rtol=1e-7)
    shapes = R.band_shapes(shape, R.bank(w)[0], levels)
    bands = [_randn(torch, lead + s, 2 + k) for k, s in enumerate(shapes)]
    assert torch.autograd.gradcheck(lambda *b: F.idwt2(list(b), shape, w), tuple(bands), eps=1e-6, atol=1e-7, rtol=1e-7)


def test_gradcheck_dwt1_and_idwt1(torch):
    F = pdwt_amd.functional
    x = _randn(torch, (3, 19), 3)
    assert torch.autograd.gradcheck(lambda t: tuple(F.dwt1(t, "db4", 2, "constant")), (x,), eps=1e-6, atol=1e-7, rtol=1e-7)
    ns = A.lengths(19, 8, 2)
    bands = [_randn(torch, (3, v), 4 + k) for k, v in enumerate([ns[2]] + ns[1:])]
    assert torch.autograd.gradcheck(lambda *b: F.idwt1(list(b), 19, "db4"), tuple(bands), eps=1e-6, atol=1e-7, rtol=1e-7)


@pytest.mark.parametrize("dtype,sfx", [("float32", "f32"), ("float64", "f64")])
def test_gradient_of_half_the_squared_norm_is_the_adjoint_of_the_transform(dtype, sfx, torch):
    F = pdwt_amd.functional
    shape, w, levels, mode = (61, 67), "db4", 2, "reflect"
    x = _randn(torch, (2,) + shape, 5, getattr(torch, dtype))
    bands = F.dwt2(x, w, levels, mode)
    assert all(b.requires_grad for b in bands) and tuple(bands[0].shape) == (2,) + R.band_shapes(shape, 8, levels)[0]
    (0.5 * sum((b * b).sum() for b in bands)).backward()
    xn = x.detach().cpu().numpy().astype(np.float64)
    fwd = R.wavedec2(xn, w, levels, mode)
    for b, r in zip(bands, fwd):
        assert A.rel_err(b.detach().cpu().numpy(), r) <= BOUND[sfx]
    ref = A.wavedec2_adjoint(fwd, shape, w, mode)
    e = A.rel_err(x.grad.cpu().numpy(), ref)
    print("grad of 0.5 |dwt2 x|^2, %s: %.3e" % (sfx, e))
    assert e <= BOUND[sfx], e
    # the bare operators agree with what autograd ran, and a round trip is the identity
    g = F.dwt2_adjoint([b.detach() for b in bands], shape, w, mode)
    assert torch.equal(g, x.grad)
    back = F.idwt2(bands, shape, w)
    assert A.rel_err(back.detach().cpu().numpy(), xn) <= 10 * BOUND[sfx]
    y = F.idwt2_adjoint(x.detach(), w, levels)
    assert [tuple(t.shape) for t in y] == [tuple(b.shape) for b in bands]


def test_no_graph_without_requires_grad(torch):
    F = pdwt_amd.functional
    x = _randn(torch, (2, 9, 11), 6, grad=False)
    bands = F.dwt2(x, "db2", 2)
    assert all(not b.requires_grad and b.grad_fn is None for b in bands)
    assert F.idwt2(bands, (9, 11), "db2").grad_fn is None
    rows = F.dwt1(x, "db2", 1, "periodic")
    assert all(b.grad_fn is None for b in rows) and F.idwt1(rows, 11, "db2").grad_fn is None
    xg = x.clone().requires_grad_(True)
    assert F.dwt1(xg, "db2", 1)[0].grad_fn is not None


def test_refusals_of_the_functional_layer(torch):
    F = pdwt_amd.functional
    x = _randn(torch, (2, 9, 11), 7, grad=False)
    bands = F.dwt2(x, "db2", 2)
    with pytest.raises(ValueError):
        F.dwt2(x, "db2", 0)
    with pytest.raises(ValueError):
        F.dwt2(x, "db2", 33)
    with pytest.raises(ValueError):
        F.dwt2(_randn(torch, (2, 6, 11), 8, grad=False), "db4", 1)  # 6 rows < hlen - 1 = 7
    with pytest.raises(ValueError):
        F.dwt1(_randn(torch, (2, 4), 8, grad=False), "db4", 1)
    with pytest.raises(ValueError):
        F.dwt1(x, "db2", 0)
    with pytest.raises(ValueError):
        F.dwt2(x, "db2", 1, "mirror")
    with pytest.raises(ValueError):
        F.dwt2(x, "nosuch", 1)
    with pytest.raises(ValueError):
        F.idwt2(bands[:-1], (9, 11), "db2")  # wrong length
    with pytest.raises(ValueError):
        F.idwt2(bands, (9, 13), "db2")  # wrong shapes: 13 columns give bands of 8, not 7
    with pytest.raises(ValueError):
        F.dwt2_adjoint(bands, (10, 11), "db2", "mirror")
    with pytest.raises(ValueError):
        F.idwt1([bands[0]], 11, "db2")
    with pytest.raises(ValueError):
        F.idwt2_adjoint(x, "db2", 0)
    with pytest.raises(TypeError):
        F.dwt2(x.cpu(), "db2", 1)
    with pytest.raises(TypeError):
        F.dwt2(x.transpose(1, 2), "db2", 1)  # not contiguous
    with pytest.raises(TypeError):
        F.dwt2(x.half(), "db2", 1)
    with pytest.raises(TypeError):
        F.dwt2(x.cpu().numpy(), "db2", 1)
    with pytest.raises(TypeError):
        F.idwt2([b.cpu() for b in bands], (9, 11), "db2")
    with pytest.raises(TypeError):
        F.dwt1(x.to(torch.int32), "db2", 1)
