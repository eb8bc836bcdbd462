"""The adjoint operators of one level of the 3-D boundary-mode transform on the GPU (include/pdwt_hip.h "Adjoints of the 3-D boundary-mode
DWT") and the differentiable dwt3 / idwt3 of pdwt_amd.functional, against the float64 reference of tests/refadj3d.py.

Bounds: 1e-5 (float32) / 1e-12 (float64) of max|ref| for every case -- the family's; tests/test_refadj3d_cpu.py measures the float32 error
of the kernels' order on each case (at most 3.7e-7: below a quarter of the bound, so no case has a bound of its own) -- and 10x those for
a round trip, as in tests/test_ext3d_gpu.py.  The operator identities are asked to 1e-12 of the product of the norms in float64."""
import ctypes as C
import functools

import numpy as np
import pytest

import pdwt_amd
from pdwt_amd import _native as nat
from tests import refadj as A
from tests import refadj3d as A3
from tests import refext3d as R3
from tests.cabi_arena import Arena, Region

pytestmark = pytest.mark.gpu

DT = {"f32": np.float32, "f64": np.float64}


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


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available()
    return torch


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


def tmp_elems(shape, hlen):
    e = pdwt_amd.hip().pdwt_ext3d_adjoint_level_tmp_elems(shape[0], shape[1], shape[2], hlen)
    assert e > 0
    return e


# ---- references, computed once ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cot3(k):
    shape, w, L, _ = A3.CASES[k]
    return tuple(A.cotangent(R3.band_shapes(shape, R3.bank(w)[0], L), (), 10 + k))


@functools.lru_cache(maxsize=None)
def ref3(k, mode):
    shape, w, L, _ = A3.CASES[k]
    r = A3.wavedec3_adjoint(list(cot3(k)), shape, w, mode)
    r.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def vol3(k):
    return A.cotangent([A3.CASES[k][0]], (), 40 + k)[0]


@functools.lru_cache(maxsize=None)
def refinv3(k):
    shape, w, L, _ = A3.CASES[k]
    return tuple(A3.waverec3_adjoint(vol3(k), w, L))


CASES3 = [(k, m) for k, c in enumerate(A3.CASES) for m in c[3]]
INV3 = [k for k, c in enumerate(A3.CASES) if c[:3] not in [d[:3] for d in A3.CASES[:k]]]  # every (shape, bank, levels) once


def _id3(p):
    s, w, L, _ = A3.CASES[p[0]]
    return "%dx%dx%d-%s-L%d-%s" % (s + (w, L, p[1]))


def chain_adj3(dev, sfx, f, ptrs, shape, levels, mode, out):
    """the level entries one after the other, coarse to fine, on the band table `ptrs`; the last level writes `out`"""
    dt = np.dtype(DT[sfx])
    shapes = R3.level_shapes(shape, f.hlen, levels)
    tmp = dev.empty(tmp_elems(shape, f.hlen), dt)
    a = ptrs[0]
    for lev in range(levels, 0, -1):
        dst = out if lev == 1 else dev.empty(int(np.prod(shapes[lev - 1])), dt)
        k0 = 1 + 7 * (levels - lev)
        nz, nr, nc = shapes[lev - 1]
        rc = fn("ext3d_forward_adjoint_level", sfx)(dst, table([a] + list(ptrs[k0:k0 + 7])), nz, nr, nc, R3.MODES.index(mode), C.byref(f), tmp)
        assert rc == 0, rc
        a = dst
    return out


def test_the_middle_z_chunk_of_the_three_chunk_case_is_interior():
    """(40, 24, 24) db2: chunks [0, 16), [16, 32), [32, 40); the halo cells repeat samples of the first and the last only"""
    L = pdwt_amd.hip()
    for mode in ("symmetric", "zero", "periodic"):
        z0, z1 = C.c_int(), C.c_int()
        assert L.pdwt_ext3d_adjoint_z_run(40, 4, R3.MODES.index(mode), C.byref(z0), C.byref(z1)) == 0
        assert z0.value <= 16 and z1.value >= 32, (mode, z0.value, z1.value)
        if mode != "zero":
            assert z0.value > 0 and z1.value < 40, (mode, z0.value, z1.value)  # the other two chunks do fold
    # (40, 48, 40) db20: halo targets in every chunk
    for mode in ("symmetric", "periodic"):
        z0, z1 = C.c_int(), C.c_int()
        assert L.pdwt_ext3d_adjoint_z_run(40, 40, R3.MODES.index(mode), C.byref(z0), C.byref(z1)) == 0
        assert z1.value - z0.value < 16, (mode, z0.value, z1.value)


# ---- adjoint values --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sfx", ["f32", "f64"])
@pytest.mark.parametrize("case", CASES3, ids=_id3)
def test_forward_adjoint_3d(case, sfx, dev):
    k, mode = case
    shape, w, levels, _ = A3.CASES[k]
    dt = DT[sfx]
    f = bank(sfx, w)
    c = [b.astype(dt) for b in cot3(k)]
    ptrs = [dev.up(b) for b in c]
    out = dev.up(np.full(shape, 777, dt))
    chain_adj3(dev, sfx, f, ptrs, shape, levels, mode, out)
    x = dev.down(out, shape, dt)
    e = A.rel_err(x, ref3(k, mode))
    print("adjoint 3-D %s %s: %.3e" % (_id3(case), sfx, e))
    assert e <= A3.bound(sfx, shape, w, levels, mode), e
    # the cotangents are intact; a second run gives the same bits
    for p, b in zip(ptrs, c):
        assert np.array_equal(dev.down(p, b.shape, dt).view(np.uint8), b.view(np.uint8))
    out2 = dev.up(np.full(shape, 555, dt))
    chain_adj3(dev, sfx, f, ptrs, shape, levels, mode, out2)
    assert np.array_equal(dev.down(out2, shape, dt).view(np.uint8), x.view(np.uint8))


@pytest.mark.parametrize("sfx", ["f32", "f64"])
@pytest.mark.parametrize("k", INV3, ids=lambda k: _id3((k, "inv")))
def test_inverse_adjoint_3d(k, sfx, dev):
    shape, w, levels, _ = A3.CASES[k]
    dt = DT[sfx]
    f = bank(sfx, w)
    shapes = R3.level_shapes(shape, f.hlen, levels)
    y = vol3(k).astype(dt)
    src = dev.up(y)
    tmp = dev.empty(tmp_elems(shape, f.hlen), dt)
    got, a = {}, src
    for lev in range(1, levels + 1):
        ptrs = [dev.up(np.full(shapes[lev], 777, dt)) for _ in range(8)]
        nz, nr, nc = shapes[lev - 1]
        before = dev.down(a, shapes[lev - 1], dt)
        assert fn("ext3d_inverse_adjoint_level", sfx)(a, table(ptrs), nz, nr, nc, C.byref(f), tmp) == 0
        assert np.array_equal(dev.down(a, shapes[lev - 1], dt).view(np.uint8), before.view(np.uint8))  # the source is intact
        for j, p in enumerate(ptrs[1:]):
            got[1 + 7 * (levels - lev) + j] = dev.down(p, shapes[lev], dt)
        a = ptrs[0]
    got[0] = dev.down(a, shapes[levels], dt)
    for n, r in enumerate(refinv3(k)):
        e = A.rel_err(got[n], r)
        print("inverse adjoint 3-D %s %s band %d: %.3e" % (_id3((k, "inv")), sfx, n, e))
        assert e <= A3.bound(sfx, shape, w, levels, "zero"), (n, e)
    assert np.array_equal(dev.down(src, shape, dt).view(np.uint8), y.view(np.uint8))


def _dev_t(torch, arr, dt, grad=False):
    return torch.from_numpy(np.ascontiguousarray(arr, dtype=dt)).cuda().requires_grad_(grad)


@pytest.mark.parametrize("sfx", ["f32", "f64"])
@pytest.mark.parametrize("case", CASES3, ids=_id3)
def test_dwt3_adjoint_of_the_functional_layer(case, sfx, torch):
    k, mode = case
    shape, w, levels, _ = A3.CASES[k]
    dt = DT[sfx]
    c = [_dev_t(torch, b, dt) for b in cot3(k)]
    keep = [b.clone() for b in c]
    x = pdwt_amd.dwt3_adjoint(c, shape, w, mode)
    assert tuple(x.shape) == shape and x.dtype == c[0].dtype and not x.requires_grad
    e = A.rel_err(x.cpu().numpy(), ref3(k, mode))
    print("dwt3_adjoint %s %s: %.3e" % (_id3(case), sfx, e))
    assert e <= A3.bound(sfx, shape, w, levels, mode), e
    assert all(torch.equal(a, b) for a, b in zip(c, keep))
    assert torch.equal(pdwt_amd.dwt3_adjoint(c, shape, w, mode), x)


@pytest.mark.parametrize("sfx", ["f32", "f64"])
@pytest.mark.parametrize("k", INV3, ids=lambda k: _id3((k, "inv")))
def test_idwt3_adjoint_of_the_functional_layer(k, sfx, torch):
    shape, w, levels, _ = A3.CASES[k]
    dt = DT[sfx]
    y = _dev_t(torch, vol3(k), dt)
    keep = y.clone()
    got = pdwt_amd.idwt3_adjoint(y, w, levels)
    assert [tuple(b.shape) for b in got] == R3.band_shapes(shape, R3.bank(w)[0], levels)
    for n, (b, r) in enumerate(zip(got, refinv3(k))):
        e = A.rel_err(b.cpu().numpy(), r)
        assert e <= A3.bound(sfx, shape, w, levels, "zero"), (n, e)
    assert torch.equal(y, keep)
    assert all(torch.equal(a, b) for a, b in zip(pdwt_amd.idwt3_adjoint(y, w, levels), got))


# ---- identities and bit equality --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,w,levels,mode", [((40, 24, 24), "db2", 2, "symmetric"), ((9, 33, 47), "haar", 3, "reflect"), ((24, 28, 32), "bior2.2", 2, "periodic")])
def test_operator_identities_3d(shape, w, levels, mode, torch):
    F = pdwt_amd.functional
    rs = np.random.RandomState(8)
    x = _dev_t(torch, rs.standard_normal(shape), np.float64)
    shapes = R3.band_shapes(shape, R3.bank(w)[0], levels)
    c = [_dev_t(torch, rs.standard_normal(s), np.float64) for s in shapes]
    dot = lambda u, v: sum(float((a * b).sum()) for a, b in zip(u, v))
    Wx, Wtc = F.dwt3(x, w, levels, mode), F.dwt3_adjoint(c, shape, w, mode)
    lhs, rhs = dot(Wx, c), float((x * Wtc).sum())
    scale = np.sqrt(dot(Wx, Wx)) * np.sqrt(dot(c, c))
    print("<Wx, c> - <x, W^T c> = %.3e of %.3e" % (lhs - rhs, scale))
    assert abs(lhs - rhs) <= 1e-12 * scale
    Sc, Stx = F.idwt3(c, shape, w), F.idwt3_adjoint(x, w, levels)
    lhs, rhs = float((Sc * x).sum()), dot(c, Stx)
    scale = np.sqrt(float((Sc * Sc).sum())) * np.sqrt(float((x * x).sum()))
    print("<Sc, x> - <c, S^T x> = %.3e of %.3e" % (lhs - rhs, scale))
    assert abs(lhs - rhs) <= 1e-12 * scale


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_a_stack_of_two_volumes_equals_two_single_calls(dtype, torch):
    F = pdwt_amd.functional
    shape, w, levels, mode = (16, 16, 16), "db2", 2, "symmetric"
    g = torch.Generator().manual_seed(3)
    x = torch.randn((2,) + shape, generator=g, dtype=torch.float64).to(getattr(torch, dtype)).cuda()
    keep = x.clone()
    both = F.dwt3(x, w, levels, mode)
    assert torch.equal(x, keep)
    for v in range(2):
        one = F.dwt3(x[v], w, levels, mode)
        assert all(torch.equal(b[v], o) for b, o in zip(both, one))
        assert torch.equal(F.dwt3_adjoint(both, shape, w, mode)[v], F.dwt3_adjoint(one, shape, w, mode))
        assert torch.equal(F.idwt3(both, shape, w)[v], F.idwt3(one, shape, w))
        assert all(torch.equal(b[v], o) for b, o in zip(F.idwt3_adjoint(x, w, levels), F.idwt3_adjoint(x[v], w, levels)))
    # a (1, 2, ...) lead is the same stack
    again = F.dwt3(x.reshape((1, 2) + shape), w, levels, mode)
    assert all(torch.equal(a[0], b) for a, b in zip(again, both))


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_dwt3_bands_are_the_coefficients_of_the_class_bit_for_bit(dt, torch):
    shape, w, levels, mode = (16, 16, 16), "db2", 2, "symmetric"
    x = R3.make_input(shape, dt)
    W = pdwt_amd.BoundaryWavelets3D(x, w, levels, mode)
    assert W.levels == levels
    W.forward()
    want = W.coeffs
    got = pdwt_amd.dwt3(_dev_t(torch, x, dt), w, levels, mode)
    assert len(got) == len(want) == 7 * levels + 1
    for n, (g, c) in enumerate(zip(got, want)):
        assert tuple(g.shape) == c.shape and np.array_equal(g.cpu().numpy().view(np.uint8), c.view(np.uint8)), n


@pytest.mark.parametrize("sfx", ["f32", "f64"])
@pytest.mark.parametrize("shape,w,levels,mode", [((16, 16, 16), "db2", 2, "symmetric"), ((9, 33, 47), "haar", 3, "reflect"), ((24, 28, 32), "bior2.2", 2, "reflect")])
def test_round_trip(shape, w, levels, mode, sfx, torch):
    dt = DT[sfx]
    xn = R3.make_input(shape, dt)
    x = _dev_t(torch, xn, dt)
    bands = pdwt_amd.dwt3(x, w, levels, mode)
    for n, (b, r) in enumerate(zip(bands, R3.wavedec3(xn.astype(np.float64), w, levels, mode))):
        assert A.rel_err(b.cpu().numpy(), r) <= A3.bound(sfx, shape, w, levels, mode), n
    back = pdwt_amd.idwt3(bands, shape, w)
    e = A.rel_err(back.cpu().numpy(), xn.astype(np.float64))
    print("round trip %s %s %s: %.3e" % (shape, w, sfx, e))
    assert e <= 10 * A3.bound(sfx, shape, w, levels, mode), e


# ---- guard zones and misaligned caller buffers: the level drivers ------------------------------------------------------------------------
@pytest.mark.parametrize("sfx", ["f32", "f64"])
@pytest.mark.parametrize("shape,wname,mode", [((9, 33, 47), "haar", "reflect"), ((16, 16, 16), "db2", "symmetric")])
def test_3d_level_drivers_on_guarded_misaligned_buffers(shape, wname, mode, sfx):
    L = pdwt_amd.hip()
    dt = np.dtype(DT[sfx])
    f = bank(sfx, wname)
    hlen = f.hlen
    nz, nr, nc = shape
    bshape = R3.level_shapes(shape, hlen, 1)[1]
    nb = int(np.prod(bshape))
    taps = R3.bank(wname)[1]
    c = A.cotangent([bshape] * 8, (), 31)
    ref = A3.dwt3_adjoint(dict(zip(R3.LEVEL_KEYS, c)), shape, taps, mode)
    y = A.cotangent([shape], (), 32)[0]
    refinv = A3.idwt3_adjoint(y, taps)
    regions = ([Region("x", nz * nr * nc, dt, "out", 1)] + [Region(k, nb, dt, "in", j + 1) for j, k in enumerate(R3.LEVEL_KEYS)]
               + [Region("tmp", tmp_elems(shape, hlen), dt, "scratch", 3)])
    arena = Arena(L, regions, {k: b.astype(dt) for k, b in zip(R3.LEVEL_KEYS, c)})
    adj, inv = fn("ext3d_forward_adjoint_level", sfx), fn("ext3d_inverse_adjoint_level", sfx)
    m = R3.MODES.index(mode)
    try:
        bands = [arena.ptr(k) for k in R3.LEVEL_KEYS]
        tab, x, tmp, fp = table(bands), arena.ptr("x"), arena.ptr("tmp"), C.byref(f)
        hole = table(bands[:5] + [None] + bands[6:])
        # refusals first: nothing may be touched (x and tmp still hold the fill pattern afterwards)
        refused = [adj(x, tab, nz, nr, nc, 5, fp, tmp), adj(x, tab, nz, nr, nc, -1, fp, tmp), adj(x, tab, 65536, nr, nc, m, fp, tmp), adj(x, tab, 0, nr, nc, m, fp, tmp),
                   adj(None, tab, nz, nr, nc, m, fp, tmp), adj(x, None, nz, nr, nc, m, fp, tmp), adj(x, tab, nz, nr, nc, m, None, tmp), adj(x, tab, nz, nr, nc, m, fp, None),
                   adj(x, hole, nz, nr, nc, m, fp, tmp), inv(x, hole, nz, nr, nc, fp, tmp), inv(None, tab, nz, nr, nc, fp, tmp), inv(x, None, nz, nr, nc, fp, tmp),
                   inv(x, tab, nz, nr, nc, None, tmp), inv(x, tab, nz, nr, nc, fp, None), inv(x, tab, 65536, nr, nc, fp, tmp)]
        if hlen > 2:
            refused += [adj(x, tab, hlen - 2, nr, nc, m, fp, tmp), adj(x, tab, nz, hlen - 2, nc, m, fp, tmp), adj(x, tab, nz, nr, hlen - 2, m, fp, tmp),
                        inv(x, tab, hlen - 2, nr, nc, fp, tmp)]
        assert refused == [-1] * len(refused), refused
        arena.by_name["x"].role = arena.by_name["tmp"].role = "in"
        arena.check("refusals %s %s" % (wname, sfx))
        arena.by_name["x"].role, arena.by_name["tmp"].role = "out", "scratch"
        # W^T: the bands are read-only
        assert adj(x, tab, nz, nr, nc, m, fp, tmp) == 0
        img = arena.check("adjoint level %s %s %s" % (wname, mode, sfx))
        e = A.rel_err(arena.get(img, "x", shape=shape), ref)
        print("guarded 3-D level adjoint %s %s %s: %.3e" % (wname, mode, sfx, e))
        assert e <= A3.bound(sfx, shape, wname, 1, mode), e
        # S^T: x is read-only, the bands are written
        arena.upload("x", y.astype(dt))
        arena.by_name["x"].role = "in"
        for k in R3.LEVEL_KEYS:
            arena.by_name[k].role = "out"
        assert inv(x, tab, nz, nr, nc, fp, tmp) == 0
        img = arena.check("inverse adjoint level %s %s" % (wname, sfx))
        for k in R3.LEVEL_KEYS:
            e = A.rel_err(arena.get(img, k, shape=bshape), refinv[k])
            assert e <= A3.bound(sfx, shape, wname, 1, "zero"), (k, e)
    finally:
        arena.free()


# ---- autograd ------------------------------------------------------------------------------------------------------------------
def _randn(torch, shape, seed, dtype=None, grad=True):
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(shape, generator=g, dtype=torch.float64).to(dtype or torch.float64).cuda()
    return t.requires_grad_(grad)


@pytest.mark.parametrize("lead,shape,w,levels,mode", [((), (4, 5, 6), "db2", 2, "symmetric"), ((2,), (3, 4, 5), "haar", 1, "periodic")])
def test_gradcheck_dwt3_and_idwt3(lead, shape, w, levels, mode, torch):
    F = pdwt_amd.functional
    x = _randn(torch, lead + shape, 1)
    assert torch.autograd.gradcheck(lambda t: tuple(F.dwt3(t, w, levels, mode)), (x,), eps=1e-6, atol=1e-7, rtol=1e-7)
    shapes = R3.band_shapes(shape, R3.bank(w)[0], levels)
    bands = [_randn(torch, lead + s, 2 + k) for k, s in enumerate(shapes)]
    assert torch.autograd.gradcheck(lambda *b: F.idwt3(list(b), shape, w), tuple(bands), eps=1e-6, atol=1e-7, rtol=1e-7)


@pytest.mark.parametrize("dtype,sfx", [("float32", "f32"), ("float64", "f64")])
def test_gradient_of_half_the_squared_norm_is_the_adjoint_of_the_transform(dtype, sfx, torch):
    F = pdwt_amd.functional
    shape, w, levels, mode = (24, 28, 32), "bior2.2", 2, "reflect"
    x = _randn(torch, (2,) + shape, 5, getattr(torch, dtype))
    bands = F.dwt3(x, w, levels, mode)
    assert all(b.requires_grad for b in bands) and tuple(bands[0].shape) == (2,) + R3.band_shapes(shape, 6, levels)[0]
    (0.5 * sum((b * b).sum() for b in bands)).backward()
    g = F.dwt3_adjoint([b.detach() for b in bands], shape, w, mode)
    assert torch.equal(g, x.grad)
    xn = x.detach().cpu().numpy().astype(np.float64)
    for v in range(2):
        fwd = R3.wavedec3(xn[v], w, levels, mode)
        ref = A3.wavedec3_adjoint(fwd, shape, w, mode)
        e = A.rel_err(x.grad[v].cpu().numpy(), ref)
        print("grad of 0.5 |dwt3 x|^2, %s volume %d: %.3e" % (sfx, v, e))
        assert e <= A3.bound(sfx, shape, w, levels, mode), e


def test_no_graph_without_requires_grad(torch):
    F = pdwt_amd.functional
    x = _randn(torch, (2, 8, 9, 10), 6, grad=False)
    bands = F.dwt3(x, "db2", 2)
    assert len(bands) == 15 and all(not b.requires_grad and b.grad_fn is None for b in bands)
    assert F.idwt3(bands, (8, 9, 10), "db2").grad_fn is None
    xg = x.clone().requires_grad_(True)
    assert F.dwt3(xg, "db2", 1)[0].grad_fn is not None
    bg = [b.clone().requires_grad_(True) for b in bands]
    assert F.idwt3(bg, (8, 9, 10), "db2").grad_fn is not None


def test_refusals_of_the_functional_layer(torch):
    F = pdwt_amd.functional
    x = _randn(torch, (2, 8, 9, 10), 7, grad=False)
    bands = F.dwt3(x, "db2", 2)
    bad_values = [
        lambda: F.dwt3(x, "db2", 0), lambda: F.dwt3(x, "db2", 14), lambda: F.dwt3(x, "db2", 1.5),
        lambda: F.dwt3(_randn(torch, (6, 9, 10), 8, grad=False), "db4", 1),   # 6 planes < hlen - 1 = 7
        lambda: F.dwt3(_randn(torch, (9, 6, 10), 8, grad=False), "db4", 1),
        lambda: F.dwt3(_randn(torch, (9, 10, 6), 8, grad=False), "db4", 1),
        lambda: F.dwt3(_randn(torch, (9, 10, 6), 8, grad=False), "db4", 3),   # (an axis of hlen - 1 samples keeps that length at every level)
        lambda: F.dwt3(x, "db2", 1, "mirror"), lambda: F.dwt3(x, "nosuch", 1), lambda: F.dwt3(x[0, 0], "haar", 1),
        lambda: F.dwt3(torch.zeros((65536, 2, 2), device="cuda"), "haar", 1),  # a size the level entries refuse
        lambda: F.idwt3(bands[:-1], (8, 9, 10), "db2"), lambda: F.idwt3(bands[:1], (8, 9, 10), "db2"),
        lambda: F.idwt3(bands, (8, 9, 13), "db2"),                             # wrong shapes: 13 columns give bands of 8, not 6
        lambda: F.idwt3(bands, (9, 10), "db2"), lambda: F.idwt3(bands, (8, 9, 0), "db2"),
        lambda: F.idwt3([bands[0].float()] + bands[1:], (8, 9, 10), "db2"),                 # (the bands are float64)
        lambda: F.dwt3_adjoint(bands, (8, 9, 10), "db2", "mirror"), lambda: F.dwt3_adjoint(bands[:8], (8, 9, 10), "db2"),
        lambda: F.dwt3_adjoint(bands, (8, 9, 10), "nosuch"), lambda: F.idwt3_adjoint(x, "db2", 0), lambda: F.idwt3_adjoint(x, "db2", 14),
    ]
    for k, call in enumerate(bad_values):
        with pytest.raises(ValueError):
            call()
            pytest.fail("call %d was not refused" % k)
    bad_types = [lambda: F.dwt3(x.cpu(), "db2", 1), lambda: F.dwt3(x.transpose(2, 3), "db2", 1), lambda: F.dwt3(x.half(), "db2", 1),
                 lambda: F.dwt3(x.cpu().numpy(), "db2", 1), lambda: F.idwt3([b.cpu() for b in bands], (8, 9, 10), "db2"),
                 lambda: F.dwt3(x.to(torch.int32), "db2", 1), lambda: F.dwt3_adjoint([b.cpu() for b in bands], (8, 9, 10), "db2"),
                 lambda: F.idwt3_adjoint(x.cpu(), "db2", 1)]
    for k, call in enumerate(bad_types):
        with pytest.raises(TypeError):
            call()
            pytest.fail("call %d was not refused" % k)
    # nothing above launched anything that changed the inputs
    assert torch.equal(F.dwt3(x, "db2", 2)[0], bands[0])
