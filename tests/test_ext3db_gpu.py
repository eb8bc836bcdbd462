"""The batched 3-D boundary-mode drivers on the GPU (include/pdwt_hip.h "Batched 3-D DWT with boundary modes"; pdwt_amd/csrc/dwt_ext3db.hip):
a stack of V volumes, every level in one call, and the functional layer on top of them.

Values: against the float64 references of tests/refext3d.py and tests/refadj3d.py, looped over the volumes, with the bounds of
tests/test_adjoint3d_gpu.py -- refadj3d.bound (1e-5 float32 / 1e-12 float64 of max|ref|, per volume) and 10x that for a round trip.
Bits: volume v of every result equals the chain of level entries (pdwt_ext3d_*_level_*) run on volume v alone."""
import ctypes as C
import functools
import re

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
OPS = ("forward", "inverse", "forward_adjoint", "inverse_adjoint")
V3 = 3

# (shape, bank, levels, modes): cases of refadj3d.CASES
SEL = [((7, 7, 7), "db4", 1, R3.MODES), ((16, 16, 16), "db2", 2, R3.MODES), ((9, 33, 47), "haar", 3, R3.MODES),
       ((40, 24, 24), "db2", 2, ("symmetric", "zero", "periodic")),   # three z chunks
       ((40, 48, 40), "db20", 1, ("constant",))]
CASES = [(s, w, L, m) for s, w, L, modes in SEL for m in modes]


def _id(c):
    return "%dx%dx%d-%s-L%d-%s" % (c[0] + c[1:])


POOL_BYTES = 192 << 20  # the grid-chunk test holds about 70 MB at a time


class Dev:
    """device buffers of one test, cut from ONE allocation of the module (an allocation per buffer costs more than the kernels here):
    256-byte aligned pieces handed out in turn; free() hands the whole pool back"""

    def __init__(self, base, nbytes):
        self.L = pdwt_amd.hip()
        self.base, self.nbytes, self.used = base, nbytes, 0

    def empty(self, elems, dt):
        n = (max(int(elems), 1) * np.dtype(dt).itemsize + 255) & ~255
        assert self.used + n <= self.nbytes, "the pool of the module is too small"
        p = self.base + self.used
        self.used += n
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
        assert self.L.pdwt_sync() == 0
        self.used = 0


@pytest.fixture(scope="module")
def pool():
    L = pdwt_amd.hip()
    base = L.pdwt_malloc(POOL_BYTES)
    assert base
    yield base
    L.pdwt_sync()
    L.pdwt_free(base)


@pytest.fixture
def dev(pool):
    d = Dev(pool, POOL_BYTES)
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


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def tmp_elems(op, V, shape, hlen, levels):
    L = pdwt_amd.hip()
    e = (L.pdwt_ext3db_adjoint_tmp_elems if op == "forward_adjoint" else L.pdwt_ext3db_tmp_elems)(V, shape[0], shape[1], shape[2], hlen, levels)
    assert e > 0, e
    return e


def call_batched(op, sfx, f, x, tab, V, shape, levels, mode, tmp):
    m = R3.MODES.index(mode)
    head = (x, tab, V, shape[0], shape[1], shape[2], levels)
    return fn("ext3db_" + op, sfx)(*(head + ((m,) if op in ("forward", "forward_adjoint") else ()) + (C.byref(f), tmp)))


def run_batched(dev, sfx, f, op, V, shape, levels, mode, inp):
    """one driver call on fresh buffers (results pre-filled with NaN); the input must come back intact.  forward / inverse_adjoint: inp is
    the (V,) + shape stack, the result the list of band stacks; inverse / forward_adjoint: the other way round."""
    dt = DT[sfx]
    bshapes = [(V,) + s for s in R3.band_shapes(shape, f.hlen, levels)]
    tmp = dev.empty(tmp_elems(op, V, shape, f.hlen, levels), dt)
    if op in ("forward", "inverse_adjoint"):
        xin = np.ascontiguousarray(inp, dtype=dt)
        x = dev.up(xin)
        bands = [dev.up(np.full(s, np.nan, dt)) for s in bshapes]
        assert call_batched(op, sfx, f, x, table(bands), V, shape, levels, mode, tmp) == 0
        out = [dev.down(p, s, dt) for p, s in zip(bands, bshapes)]
        assert same_bits(dev.down(x, xin.shape, dt), xin), "the source changed"
        return out
    cin = [np.ascontiguousarray(b, dtype=dt) for b in inp]
    assert [b.shape for b in cin] == bshapes
    bands = [dev.up(b) for b in cin]
    x = dev.up(np.full((V,) + shape, np.nan, dt))
    assert call_batched(op, sfx, f, x, table(bands), V, shape, levels, mode, tmp) == 0
    out = dev.down(x, (V,) + shape, dt)
    for p, b in zip(bands, cin):
        assert same_bits(dev.down(p, b.shape, dt), b), "a band changed"
    return out


def run_chain(dev, sfx, f, op, shape, levels, mode, inp):
    """the chain of level entries on ONE volume: the yardstick of the bits.  Same layout as run_batched without the leading axis."""
    dt = DT[sfx]
    shapes = R3.level_shapes(shape, f.hlen, levels)
    e = pdwt_amd.hip().pdwt_ext3d_adjoint_level_tmp_elems(shape[0], shape[1], shape[2], f.hlen)
    assert e > 0
    tmp = dev.empty(e, dt)
    m = R3.MODES.index(mode)
    if op in ("forward", "inverse_adjoint"):
        a = dev.up(np.ascontiguousarray(inp, dtype=dt))
        got = [None] * (7 * levels + 1)
        for lev in range(1, levels + 1):
            ptrs = [dev.up(np.full(shapes[lev], np.nan, dt)) for _ in range(8)]
            nz, nr, nc = shapes[lev - 1]
            if op == "forward":
                rc = fn("ext3d_forward_level", sfx)(a, table(ptrs), nz, nr, nc, m, C.byref(f), tmp)
            else:
                rc = fn("ext3d_inverse_adjoint_level", sfx)(a, table(ptrs), nz, nr, nc, C.byref(f), tmp)
            assert rc == 0, rc
            for j, p in enumerate(ptrs[1:]):
                got[1 + 7 * (levels - lev) + j] = dev.down(p, shapes[lev], dt)
            a = ptrs[0]
        got[0] = dev.down(a, shapes[levels], dt)
        return got
    ptrs = [dev.up(np.ascontiguousarray(b, dtype=dt)) for b in inp]
    a = ptrs[0]
    for lev in range(levels, 0, -1):
        dst = dev.up(np.full(shapes[lev - 1], np.nan, dt))
        k0 = 1 + 7 * (levels - lev)
        nz, nr, nc = shapes[lev - 1]
        if op == "inverse":
            rc = fn("ext3d_inverse_level", sfx)(dst, table([a] + ptrs[k0:k0 + 7]), nz, nr, nc, C.byref(f), tmp)
        else:
            rc = fn("ext3d_forward_adjoint_level", sfx)(dst, table([a] + ptrs[k0:k0 + 7]), nz, nr, nc, m, C.byref(f), tmp)
        assert rc == 0, rc
        a = dst
    return dev.down(a, shape, dt)


# ---- inputs and float64 references, computed once and left unchanged -------------------------------------------------------------
def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def vols(shape):
    """V3 distinct volumes whose values are float32 numbers"""
    return _frozen(A.cotangent([shape], (V3,), 71)[0])


@functools.lru_cache(maxsize=None)
def cots(shape, w, levels):
    return tuple(_frozen(b) for b in A.cotangent(R3.band_shapes(shape, R3.bank(w)[0], levels), (V3,), 72))


def _stack_tables(per_volume):
    return tuple(_frozen(np.stack([t[k] for t in per_volume])) for k in range(len(per_volume[0])))


@functools.lru_cache(maxsize=None)
def ref_forward(shape, w, levels, mode):
    return _stack_tables([R3.wavedec3(vols(shape)[v], w, levels, mode) for v in range(V3)])


@functools.lru_cache(maxsize=None)
def ref_forward_adjoint(shape, w, levels, mode):
    c = cots(shape, w, levels)
    return _frozen(np.stack([A3.wavedec3_adjoint([b[v] for b in c], shape, w, mode) for v in range(V3)]))


@functools.lru_cache(maxsize=None)
def ref_inverse(shape, w, levels):
    c = cots(shape, w, levels)
    return _frozen(np.stack([R3.waverec3([b[v] for b in c], shape, w) for v in range(V3)]))


@functools.lru_cache(maxsize=None)
def ref_inverse_adjoint(shape, w, levels):
    return _stack_tables([A3.waverec3_adjoint(vols(shape)[v], w, levels) for v in range(V3)])


def worst(got, ref):
    """the largest error of a volume relative to that volume's max|ref|"""
    return max(A.rel_err(got[v], ref[v]) for v in range(ref.shape[0]))


def check_values(results, shape, w, levels, mode, sfx, what):
    """results: {op: result of run_batched on vols / cots}; every band and volume against the float64 references"""
    bound = A3.bound(sfx, shape, w, levels, mode)
    zero = A3.bound(sfx, shape, w, levels, "zero")
    errs = {"forward": max(worst(g, r) for g, r in zip(results["forward"], ref_forward(shape, w, levels, mode))),
            "inverse": worst(results["inverse"], ref_inverse(shape, w, levels)),
            "forward_adjoint": worst(results["forward_adjoint"], ref_forward_adjoint(shape, w, levels, mode)),
            "inverse_adjoint": max(worst(g, r) for g, r in zip(results["inverse_adjoint"], ref_inverse_adjoint(shape, w, levels)))}
    print("%s %s: %s" % (what, sfx, ", ".join("%s %.3e" % (k, errs[k]) for k in OPS)))
    assert errs["forward"] <= bound and errs["forward_adjoint"] <= bound, errs
    assert errs["inverse"] <= bound and errs["inverse_adjoint"] <= zero, errs


def inputs_of(op, shape, w, levels):
    return vols(shape) if op in ("forward", "inverse_adjoint") else list(cots(shape, w, levels))


# ---- 1. against the float64 references, and 2. bit equality ---------------------------------------------------------------------------
def equal_results(a, b):
    return all(same_bits(p, q) for p, q in zip(a, b)) and len(a) == len(b) if isinstance(a, list) else same_bits(a, b)


def volume_of(res, v):
    return [b[v] for b in res] if isinstance(res, list) else res[v]


@pytest.mark.parametrize("shape,w,levels,modes", SEL, ids=["%dx%dx%d-%s-L%d" % (c[0] + c[1:3]) for c in SEL])
def test_four_operators_against_the_float64_references_and_the_bits_of_the_level_entries(shape, w, levels, modes, dev):
    """every mode of the case, both precisions, V = 3 distinct volumes (one test per shape: the suite counts its tests).  Values: every
    operator against the float64 reference per volume, and the round trip.  Bits: a second run; every volume against the chain of level
    entries on it alone; V = 3 against three V = 1 calls."""
    for mode in modes:
        values_and_bits(dev, (shape, w, levels, mode))


def values_and_bits(dev, case):
    shape, w, levels, mode = case
    for sfx in ("f32", "f64"):
        f = bank(sfx, w)
        res = {}
        for op in OPS:
            inp = inputs_of(op, shape, w, levels)
            res[op] = run_batched(dev, sfx, f, op, V3, shape, levels, mode, inp)
            assert equal_results(run_batched(dev, sfx, f, op, V3, shape, levels, mode, inp), res[op]), (_id(case), sfx, op, "second run")
            for v in range(V3):
                one = volume_of(inp, v)
                assert equal_results(volume_of(res[op], v), run_chain(dev, sfx, f, op, shape, levels, mode, one)), (_id(case), sfx, op, v, "level entries")
                single = run_batched(dev, sfx, f, op, 1, shape, levels, mode, [b[None] for b in one] if isinstance(one, list) else one[None])
                assert equal_results(volume_of(single, 0), volume_of(res[op], v)), (_id(case), sfx, op, v, "V = 1")
            dev.free()
        check_values(res, shape, w, levels, mode, sfx, "batched " + _id(case))
        back = run_batched(dev, sfx, f, "inverse", V3, shape, levels, mode, res["forward"])
        e = worst(back, vols(shape))
        print("round trip %s %s: %.3e" % (_id(case), sfx, e))
        assert e <= 10 * A3.bound(sfx, shape, w, levels, mode), (_id(case), sfx, e)
        dev.free()


# ---- 3. grid chunks ---------------------------------------------------------------------------------------------------------------
def test_plane_and_pair_chunks_that_begin_inside_the_batch_and_inside_a_volume(dev):
    for mode in ("symmetric", "zero"):
        chunked_batch(dev, mode)


def chunked_batch(dev, mode):
    """(7, 3, 3) haar L2, V = 32769: level 1 has 7 V = 229383 planes (x-y chunks of 65535 begin at plane 65535 = volume 9362, plane 1)
    and 4 V = 131076 pairs (z chunks begin at pair 65535 = volume 16383, quadrant 3); level 2 has 4 V planes."""
    sfx, dt, shape, w, levels, V = "f32", np.float32, (7, 3, 3), "haar", 2, 32769
    assert 7 * V > 3 * 65535 and 4 * V > 2 * 65535 and 65535 % 7 and 65535 % 4
    f = bank(sfx, w)
    rs = np.random.RandomState(5)
    base_x = rs.standard_normal((5,) + shape).astype(dt)
    base_c = [rs.standard_normal((5,) + s).astype(dt) for s in R3.band_shapes(shape, f.hlen, levels)]
    pick = np.arange(V) % 5
    for op in OPS:
        base = base_x if op in ("forward", "inverse_adjoint") else base_c
        ref = [run_chain(dev, sfx, f, op, shape, levels, mode, volume_of(base, j)) for j in range(5)]
        inp = base[pick] if not isinstance(base, list) else [b[pick] for b in base]
        got = run_batched(dev, sfx, f, op, V, shape, levels, mode, inp)
        if isinstance(got, list):
            for k, g in enumerate(got):
                want = np.stack([r[k] for r in ref])[pick]
                assert same_bits(g, want), (mode, op, k, np.flatnonzero((g.view(np.uint32) != want.view(np.uint32)).reshape(V, -1).any(axis=1))[:8])
        else:
            want = np.stack(ref)[pick]
            assert same_bits(got, want), (mode, op, np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)).reshape(V, -1).any(axis=1))[:8])
        dev.free()


# ---- 4. guard zones and misaligned caller buffers -----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,w,levels,mode", [((9, 33, 47), "haar", 3, "reflect"), ((7, 7, 7), "db4", 1, "symmetric")])
def test_drivers_on_guarded_misaligned_buffers(shape, w, levels, mode):
    for sfx in ("f32", "f64"):
        guarded(shape, w, levels, mode, sfx)


def guarded(shape, w, levels, mode, sfx):
    L = pdwt_amd.hip()
    dt = np.dtype(DT[sfx])
    f = bank(sfx, w)
    V, m = V3, R3.MODES.index(mode)
    bshapes = R3.band_shapes(shape, f.hlen, levels)
    names = ["b%d" % k for k in range(len(bshapes))]
    regions = ([Region("x", V * int(np.prod(shape)), dt, "in", 1)] + [Region(n, V * int(np.prod(s)), dt, "out", 1 + k % 3) for k, (n, s) in enumerate(zip(names, bshapes))]
               + [Region("tmp", tmp_elems("forward", V, shape, f.hlen, levels), dt, "scratch", 3), Region("tmpa", tmp_elems("forward_adjoint", V, shape, f.hlen, levels), dt, "scratch", 1)])
    arena = Arena(L, regions, {"x": vols(shape).astype(dt)})

    def roles(x, bands):
        arena.by_name["x"].role = x
        for n in names:
            arena.by_name[n].role = bands

    try:
        x, tmp, tmpa, fp = arena.ptr("x"), arena.ptr("tmp"), arena.ptr("tmpa"), C.byref(f)
        ptrs = [arena.ptr(n) for n in names]
        tab, hole = table(ptrs), table(ptrs[:3] + [None] + ptrs[4:])
        nz, nr, nc = shape
        fwd, inv, adj, iadj = (fn("ext3db_" + op, sfx) for op in OPS)
        # refusals first: nothing may be touched, the scratch included
        refused = [fwd(x, tab, V, nz, nr, nc, levels, 5, fp, tmp), fwd(x, tab, V, nz, nr, nc, levels, -1, fp, tmp), fwd(x, tab, 0, nz, nr, nc, levels, m, fp, tmp),
                   fwd(x, tab, V, nz, nr, nc, 0, m, fp, tmp), fwd(x, tab, V, nz, nr, nc, 14, m, fp, tmp), fwd(x, hole, V, nz, nr, nc, levels, m, fp, tmp),
                   fwd(None, tab, V, nz, nr, nc, levels, m, fp, tmp), fwd(x, None, V, nz, nr, nc, levels, m, fp, tmp), fwd(x, tab, V, nz, nr, nc, levels, m, None, tmp),
                   fwd(x, tab, V, nz, nr, nc, levels, m, fp, None), fwd(x, tab, V, 65536, nr, nc, levels, m, fp, tmp), fwd(x, tab, V, f.hlen - 2, nr, nc, levels, m, fp, tmp),
                   inv(x, tab, V, nz, nr, nc, 14, fp, tmp), inv(x, hole, V, nz, nr, nc, levels, fp, tmp), inv(x, tab, -1, nz, nr, nc, levels, fp, tmp),
                   inv(x, tab, V, nz, f.hlen - 2, nc, levels, fp, tmp), inv(x, tab, V, nz, nr, nc, levels, fp, None),
                   adj(x, tab, V, nz, nr, nc, levels, 5, fp, tmpa), adj(x, hole, V, nz, nr, nc, levels, m, fp, tmpa), adj(x, tab, V, 65536, nr, nc, levels, m, fp, tmpa),
                   adj(x, tab, V, nz, nr, nc, 0, m, fp, tmpa), adj(None, tab, V, nz, nr, nc, levels, m, fp, tmpa),
                   iadj(x, hole, V, nz, nr, nc, levels, fp, tmp), iadj(x, tab, 0, nz, nr, nc, levels, fp, tmp), iadj(x, tab, V, nz, nr, f.hlen - 2, levels, fp, tmp),
                   iadj(x, tab, V, nz, nr, nc, levels, None, tmp)]
        assert refused == [-1] * len(refused), refused
        roles("in", "in")
        arena.by_name["tmp"].role = arena.by_name["tmpa"].role = "in"
        arena.check("refusals %s %s" % (w, sfx))
        arena.by_name["tmp"].role = arena.by_name["tmpa"].role = "scratch"
        res = {}
        # W: x is read-only
        roles("in", "out")
        assert fwd(x, tab, V, nz, nr, nc, levels, m, fp, tmp) == 0
        img = arena.check("forward %s %s %s" % (w, mode, sfx))
        res["forward"] = [arena.get(img, n, shape=(V,) + s) for n, s in zip(names, bshapes)]
        # S on those bands: a round trip; the bands are read-only
        roles("out", "in")
        assert inv(x, tab, V, nz, nr, nc, levels, fp, tmp) == 0
        img = arena.check("inverse %s %s" % (w, sfx))
        e = worst(arena.get(img, "x", shape=(V,) + shape), vols(shape))
        assert e <= 10 * A3.bound(sfx, shape, w, levels, mode), e
        # S and W^T on the cotangents
        for n, c in zip(names, cots(shape, w, levels)):
            arena.upload(n, c.astype(dt))
        assert inv(x, tab, V, nz, nr, nc, levels, fp, tmp) == 0
        img = arena.check("inverse %s %s" % (w, sfx))
        res["inverse"] = arena.get(img, "x", shape=(V,) + shape)
        assert adj(x, tab, V, nz, nr, nc, levels, m, fp, tmpa) == 0
        img = arena.check("forward adjoint %s %s %s" % (w, mode, sfx))
        res["forward_adjoint"] = arena.get(img, "x", shape=(V,) + shape)
        # S^T: x is read-only
        arena.upload("x", vols(shape).astype(dt))
        roles("in", "out")
        assert iadj(x, tab, V, nz, nr, nc, levels, fp, tmp) == 0
        img = arena.check("inverse adjoint %s %s" % (w, sfx))
        res["inverse_adjoint"] = [arena.get(img, n, shape=(V,) + s) for n, s in zip(names, bshapes)]
        check_values(res, shape, w, levels, mode, sfx, "guarded %s %s" % (w, mode))
    finally:
        arena.free()


# ---- 5. operator identities -------------------------------------------------------------------------------------------------------
def test_operator_identities_on_a_batch(dev):
    for shape, w, levels, mode in [((40, 24, 24), "db2", 2, "symmetric"), ((9, 33, 47), "haar", 3, "reflect"), ((7, 7, 7), "db4", 1, "constant")]:
        identities(dev, shape, w, levels, mode)
        dev.free()


def identities(dev, shape, w, levels, mode):
    sfx = "f64"
    f = bank(sfx, w)
    x, c = vols(shape), list(cots(shape, w, levels))
    dot = lambda u, v: sum(float((a * b).sum()) for a, b in zip(u, v))
    Wx = run_batched(dev, sfx, f, "forward", V3, shape, levels, mode, x)
    Wtc = run_batched(dev, sfx, f, "forward_adjoint", V3, shape, levels, mode, c)
    lhs, rhs = dot(Wx, c), float((x * Wtc).sum())
    scale = np.sqrt(dot(Wx, Wx)) * np.sqrt(dot(c, c))
    print("<Wx, c> - <x, W^T c> = %.3e of %.3e" % (lhs - rhs, scale))
    assert abs(lhs - rhs) <= 1e-12 * scale, (shape, w, mode)
    Sc = run_batched(dev, sfx, f, "inverse", V3, shape, levels, mode, c)
    Stx = run_batched(dev, sfx, f, "inverse_adjoint", V3, shape, levels, mode, x)
    lhs, rhs = float((Sc * x).sum()), dot(c, Stx)
    scale = np.sqrt(float((Sc * Sc).sum())) * np.sqrt(float((x * x).sum()))
    print("<Sc, x> - <c, S^T x> = %.3e of %.3e" % (lhs - rhs, scale))
    assert abs(lhs - rhs) <= 1e-12 * scale, (shape, w, mode)


# ---- 6. the functional layer ------------------------------------------------------------------------------------------------------
class Recorder:
    """the library, with the names that are fetched from it written down"""

    def __init__(self, lib):
        self._lib, self.names = lib, []

    def __getattr__(self, name):
        self.names.append(name)
        return getattr(self._lib, name)


def test_the_functional_layer_makes_one_batched_call_per_operator(torch, dev, monkeypatch):
    F = pdwt_amd.functional
    lead, shape, w, levels, mode, sfx = (2, 3), (9, 10, 11), "db2", 2, "symmetric", "f64"
    f = bank(sfx, w)
    rs = np.random.RandomState(9)
    xn = rs.standard_normal(lead + shape)
    cn = [rs.standard_normal(lead + s) for s in R3.band_shapes(shape, f.hlen, levels)]
    x = torch.from_numpy(xn).cuda()
    c = [torch.from_numpy(b).cuda() for b in cn]
    rec = Recorder(pdwt_amd.hip())
    monkeypatch.setattr(nat, "hip", lambda: rec)
    calls = {"forward": lambda: F.dwt3(x, w, levels, mode), "inverse": lambda: F.idwt3(c, shape, w),
             "forward_adjoint": lambda: F.dwt3_adjoint(c, shape, w, mode), "inverse_adjoint": lambda: F.idwt3_adjoint(x, w, levels)}
    got = {}
    for op in OPS:
        del rec.names[:]
        got[op] = calls[op]()
        batched = [n for n in rec.names if re.match(r"pdwt_ext3db_(forward|inverse)(_adjoint)?_f(32|64)$", n)]
        assert batched == ["pdwt_ext3db_%s_%s" % (op, sfx)], (op, rec.names)
        assert not [n for n in rec.names if re.match(r"pdwt_ext3d_\w+_level_f(32|64)$", n)], (op, rec.names)
    monkeypatch.undo()
    for op in OPS:
        res = got[op]
        if isinstance(res, list):
            assert [tuple(b.shape) for b in res] == [lead + s for s in R3.band_shapes(shape, f.hlen, levels)]
            res = [b.cpu().numpy().reshape((-1,) + tuple(b.shape[len(lead):])) for b in res]
        else:
            assert tuple(res.shape) == lead + shape
            res = res.cpu().numpy().reshape((-1,) + shape)
        inp = xn.reshape((-1,) + shape) if op in ("forward", "inverse_adjoint") else [b.reshape((-1,) + b.shape[len(lead):]) for b in cn]
        for v in range(6):
            assert equal_results(volume_of(res, v), run_chain(dev, sfx, f, op, shape, levels, mode, volume_of(inp, v))), (op, v)
