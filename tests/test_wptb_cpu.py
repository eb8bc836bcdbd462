"""CPU-only: the batched 2-D wavelet packet layer loads and its device-free logic is right -- the exported symbols of the three libraries,
the geometry against WaveletPackets::geometry, the plan of the fused form (pdwt_wptb_fused / pdwt_wptb_lds_bytes / pdwt_wptb_tmp_elems: the
shapes DESIGN 3.17 tabulates, monotone in the image size, the largest fused square found by search through the plan function), the
node-state table of the inverse and the chunk lists of its per-depth form, and every refusal of the whole-transform drivers (refused before
anything touches a device).  The transcript of failed constructions of WaveletPacketsImages is in test_packets_host_cpu.py, with those of
the other two packet classes."""
import ctypes as C

import numpy as np
import pytest

import pdwt_amd
from pdwt_amd import _native as nat
from pdwt_amd import wpt
from tests import refwpt as R

HANDLE = ["new", "delete", "forward", "inverse", "fused", "get_image", "set_image", "state", "info", "node_shape", "path_index", "geometry", "get_node",
          "get_level", "set_node", "node_int_ptr", "node_costs", "best_basis", "set_basis", "basis_size", "get_basis", "soft_threshold", "hard_threshold",
          "norm1", "images_norm1", "node_stats", "estimate_sigma", "images_estimate_sigma"]
PLAIN = ["pdwt_wptb_geometry", "pdwt_wptb_fused", "pdwt_wptb_lds_bytes", "pdwt_wptb_tmp_elems", "pdwt_wptb_state_table", "pdwt_wptb_chunk_lists"]
TYPED = ["wptb_forward", "wptb_inverse"]
LDS_MAX = 160 * 1024


def off(l):
    return (4 ** l - 1) // 3


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_handle_symbols_load(dt):
    L = nat.host(dt)
    missing = [n for n in HANDLE if not hasattr(L, "pdwt_wpbh_" + n)]
    assert not missing, missing
    assert pdwt_amd.WaveletPacketBatch is wpt.WaveletPacketBatch and "WaveletPacketBatch" in pdwt_amd.__all__
    assert issubclass(wpt.WaveletPacketBatch, wpt.WaveletPackets2D)


def test_c_abi_symbols_are_listed_and_exported():
    L = pdwt_amd.hip()
    for n in PLAIN:
        assert n in nat.PLAIN_SYMBOLS and hasattr(L, n), n
    for n in TYPED:
        assert n in nat.TYPED_SYMBOLS
        for s in ("f32", "f64"):
            assert hasattr(L, "pdwt_%s_%s" % (n, s))


def _geom(fn, Nr, Nc, hlen, asked):
    nr, nc = (C.c_int * 8)(), (C.c_int * 8)()
    L = fn(Nr, Nc, hlen, asked, nr, nc)
    return L, [(nr[k], nc[k]) for k in range(L + 1)] if L > 0 else []


def test_geometry_is_that_of_the_single_image_class():
    hipfn = pdwt_amd.hip().pdwt_wptb_geometry
    for dt in (np.float32, np.float64):
        H = nat.host(dt)
        for Nr, Nc in ((37, 51), (9, 7), (8, 8), (64, 64), (128, 128), (61, 67), (78, 80), (160, 200), (6, 64), (1, 1), (0, 5), (46341, 46341)):
            for hlen in (2, 4, 6, 8, 16, 40, 3, 0, 42):
                for asked in (-1, 0, 1, 2, 3, 7, 9):
                    if hlen in (3, 0, 42):  # the class never sees a bad bank length; the C entry gives 0
                        assert hipfn(Nr, Nc, hlen, asked, None, None) == 0
                        continue
                    want = _geom(H.pdwt_wpt_geometry, Nr, Nc, hlen, asked)
                    assert _geom(hipfn, Nr, Nc, hlen, asked) == want == _geom(H.pdwt_wpbh_geometry, Nr, Nc, hlen, asked), (Nr, Nc, hlen, asked)
    assert _geom(hipfn, 37, 51, 6, 2) == (2, [(37, 51), (19, 26), (10, 13)])
    assert _geom(hipfn, 128, 128, 2, 9)[0] == 7 and _geom(hipfn, 6, 64, 8, 2) == (0, [])
    assert hipfn(78, 80, 40, 3, None, None) == 1 == R.clamp_levels((78, 80), "db20", 3)


def _plan_bytes(Nr, Nc, hlen, L, elem):
    """DESIGN 3.17, restated: (forward, inverse) bytes of the dynamic LDS of one workgroup"""
    nr, nc = [Nr], [Nc]
    for _ in range(L):
        nr.append((nr[-1] + 1) // 2), nc.append((nc[-1] + 1) // 2)
    ru4 = lambda v: (v + 3) & ~3
    cur = ru4(max(4 ** l * nr[l] * nc[l] for l in range(L + 1)))
    tmp = ru4(max(cur, max(2 * 4 ** l * nr[l] * nc[l + 1] for l in range(L))))
    tab = ru4(2 * max(nr[1], nc[1]) + hlen - 2)
    fwd = (cur + tmp) * elem + 8 * tab
    return fwd, fwd + ((off(L + 1) + 15) & ~15)


def test_plan_of_the_tabulated_shapes():
    L = pdwt_amd.hip()
    fu, lds, tmp = L.pdwt_wptb_fused, L.pdwt_wptb_lds_bytes, L.pdwt_wptb_tmp_elems
    table = [((64, 64), 8, 3, 4, 1), ((128, 128), 8, 3, 4, 1), ((128, 128), 8, 3, 8, 0), ((78, 80), 40, 1, 8, 1), ((256, 256), 8, 3, 4, 0),
             ((96, 96), 8, 3, 8, 1), ((37, 51), 6, 2, 4, 1), ((160, 200), 8, 3, 4, 0), ((128, 128), 2, 7, 4, 1)]
    for (Nr, Nc), hlen, lev, elem, want in table:
        assert fu(Nr, Nc, hlen, lev, elem) == want, (Nr, Nc, hlen, elem)
        f, i = _plan_bytes(Nr, Nc, hlen, lev, elem)
        assert (lds(Nr, Nc, hlen, lev, elem, 0), lds(Nr, Nc, hlen, lev, elem, 1)) == (f, i)
        assert (max(f, i) <= LDS_MAX) == bool(want)
        assert (tmp(5, Nr, Nc, hlen, lev, elem, 1) == 0) == bool(want)  # scratch exactly when the per-depth form runs
        assert tmp(5, Nr, Nc, hlen, lev, elem, 0) == sum(min(5 * 4 ** l, 16384) for l in range(lev)) > 0
    assert _plan_bytes(64, 64, 8, 3, 4) == (33344, 33440) and _plan_bytes(128, 128, 8, 3, 4) == (132160, 132256)  # below / above the 64 KiB opt-in
    assert _plan_bytes(78, 80, 40, 1, 8) == (100800, 100816) and _plan_bytes(128, 128, 8, 3, 8)[1] == 263328
    assert fu(6, 64, 8, 2, 4) == -1 and fu(64, 64, 8, 3, 2) == -1 and fu(64, 64, 7, 3, 4) == -1 and lds(64, 64, 8, 3, 4, 2) == -1
    assert tmp(0, 64, 64, 8, 3, 4, 1) == -1 and tmp(65536, 64, 64, 8, 3, 4, 1) == -1 and tmp(65535, 128, 128, 2, 4, 4, 1) == -1  # B 4^4 > 2^22
    assert tmp(65535, 64, 64, 8, 3, 4, 1) == 0 and tmp(16384, 128, 128, 2, 4, 4, 1) == 0 and tmp(16385, 128, 128, 2, 4, 4, 1) == -1


def largest_fused_square(hlen, elem, levels=3):
    """the largest n with pdwt_wptb_fused(n, n) == 1, by bisection through the plan function (monotone: asserted below)"""
    fu = pdwt_amd.hip().pdwt_wptb_fused
    lo, hi = max(2 * (hlen - 1), 2), 4096
    assert fu(lo, lo, hlen, levels, elem) == 1 and fu(hi, hi, hlen, levels, elem) == 0
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if fu(mid, mid, hlen, levels, elem) == 1 else (lo, mid)
    return lo


@pytest.mark.parametrize("elem", [4, 8])
@pytest.mark.parametrize("hlen", [2, 8, 40])
def test_plan_is_monotone_and_the_largest_fused_square(hlen, elem):
    fu = pdwt_amd.hip().pdwt_wptb_fused
    last = 1
    for n in range(max(2 * (hlen - 1), 2), 400):  # once an image stops fitting no larger one fits (the asked depth clamps as the size allows)
        f = fu(n, n, hlen, 7, elem)
        assert f in (0, 1) and f <= last, (hlen, n)
        last = f
    assert last == 0
    for n in (78, 100, 131):  # and in Nr Nc for other aspects
        assert fu(n, 2 * n, hlen, 1, elem) >= fu(2 * n, 2 * n, hlen, 1, elem) and fu(n, n, hlen, 1, elem) >= fu(n, 2 * n, hlen, 1, elem) >= 0
    n = largest_fused_square(hlen, elem)
    wname = {2: "haar", 8: "db4", 40: "db20"}[hlen]
    fits = [max(_plan_bytes(m, m, hlen, R.clamp_levels((m, m), wname, 3), elem)) <= LDS_MAX for m in (n, n + 1)]
    assert fits == [True, False]
    # "float32 up to about 128 x 128, float64 up to about 96 x 96": two image-sized buffers in 160 KiB
    assert (135 <= n <= 143) if elem == 4 else (95 <= n <= 101), n


def _table(levels, nodes, fill=9):
    L = pdwt_amd.hip()
    d, i = (C.c_int * max(len(nodes), 1))(*[v[0] for v in nodes]), (C.c_int * max(len(nodes), 1))(*[v[1] for v in nodes])
    out = (C.c_ubyte * off(levels + 1))(*([fill] * off(levels + 1)))
    return L.pdwt_wptb_state_table(levels, d, i, len(nodes), out), list(out)


def test_state_table():
    # 1 = a node of the basis, 2 = above it, 0 = below it; node i of depth l at (4^l - 1) / 3 + i
    assert _table(1, [(1, q) for q in range(4)]) == (0, [2, 1, 1, 1, 1])
    assert _table(2, [(2, k) for k in range(16)]) == (0, [2] + [2] * 4 + [1] * 16)
    assert _table(2, [(0, 0)]) == (0, [1] + [0] * 20)
    mixed = [(1, 0), (1, 2), (1, 3)] + [(2, 4 + q) for q in range(4)]
    assert _table(2, mixed) == (0, [2, 1, 2, 1, 1] + [0] * 4 + [1] * 4 + [0] * 8)
    deep = sorted(set(mixed) - {(2, 5)} | {(3, 20 + q) for q in range(4)})
    rc, t = _table(3, deep)
    assert rc == 0 and t[:5] == [2, 1, 2, 1, 1] and t[5:21] == [0] * 4 + [1, 2, 1, 1] + [0] * 8 and t[21:] == [0] * 20 + [1] * 4 + [0] * 40
    for bad in ([(1, 0), (1, 1), (1, 2)], [(1, 0), (1, 1), (1, 2), (1, 3), (2, 0)], [(1, 0)] * 2 + [(1, 1), (1, 2), (1, 3)], [(3, 0)], [(1, 4)], [(1, -1)],
                [(0, 0), (1, 0)], []):
        assert _table(2, bad)[0] == -1, bad  # gap, overlap, duplicate, too deep, bad index, nothing
        if bad:
            with pytest.raises(ValueError):
                R.check_basis(bad, 2)
    assert _table(0, [(0, 0)])[0] == -1 and pdwt_amd.hip().pdwt_wptb_state_table(8, None, None, 1, None) == -1
    assert pdwt_amd.hip().pdwt_wptb_state_table(2, None, None, 1, (C.c_ubyte * 21)()) == -1


def test_chunk_lists_of_the_per_depth_inverse():
    L = pdwt_amd.hip()
    mixed = [(1, 0), (1, 2), (1, 3)] + [(2, 4 + q) for q in range(4)]
    st = (C.c_ubyte * 21)(*_table(2, mixed)[1])
    n = L.pdwt_wptb_chunk_lists(3, 2, st, None)
    assert n == 3 + 12 == L.pdwt_wptb_tmp_elems(3, 64, 64, 8, 2, 4, 0)
    out = (C.c_int * n)(*([-7] * n))
    assert L.pdwt_wptb_chunk_lists(3, 2, st, out) == n
    assert list(out[:3]) == [0, 1, 2] and list(out[3:6]) == [1, 5, 9] and list(out[6:]) == [-7] * 9  # depth 0: every image; depth 1: node 1 of each
    # a chunk of 16384 parents holds 16384 / 4^l whole images: the list of one chunk serves them all
    big = 5000
    n = L.pdwt_wptb_chunk_lists(big, 2, st, None)
    assert n == 5000 + 16384
    out = (C.c_int * n)()
    assert L.pdwt_wptb_chunk_lists(big, 2, st, out) == n and list(out[5000:5004]) == [1, 5, 9, 13] and out[5000 + 4095] == 4 * 4095 + 1 and out[5000 + 4096] == 0
    bad = (C.c_ubyte * 21)(*([1] * 21))
    assert L.pdwt_wptb_chunk_lists(3, 2, bad, None) == -1 and L.pdwt_wptb_chunk_lists(0, 2, st, None) == -1 and L.pdwt_wptb_chunk_lists(3, 2, None, None) == -1
    assert L.pdwt_wptb_chunk_lists(65536, 2, st, None) == -1 and L.pdwt_wptb_chunk_lists(3, 8, st, None) == -1
    root = (C.c_ubyte * 21)(*_table(2, [(0, 0)])[1])
    assert L.pdwt_wptb_chunk_lists(3, 2, root, None) == -1  # nothing to synthesise: the inverse has no work


@pytest.mark.parametrize("sfx,FT", [("f32", nat.Filters32), ("f64", nat.Filters64)])
def test_drivers_refuse_bad_arguments(sfx, FT):
    """PDWT_EINVAL before anything is launched: the pointers are never dereferenced (they are not device memory)."""
    L = pdwt_amd.hip()
    f = FT()
    assert getattr(L, "pdwt_compute_filters_separable_" + sfx)(b"db4", 0, C.byref(f)) == 8
    f.hlen = 8
    g = FT()
    fake = C.c_void_p(4096)
    tab = (C.c_void_p * 3)(4096, 4096, 4096)
    hole = (C.c_void_p * 3)(4096, None, 4096)
    st = (C.c_ubyte * off(4))(*_table(3, [(3, k) for k in range(64)])[1])
    mixed = (C.c_ubyte * off(4))(*_table(3, [(1, 0), (1, 2), (1, 3)] + [(2, 4 + q) for q in range(4)])[1])
    garbage = (C.c_ubyte * off(4))(*([2] * off(4)))
    fwd, inv = getattr(L, "pdwt_wptb_forward_" + sfx), getattr(L, "pdwt_wptb_inverse_" + sfx)
    for allow in (0, 1):
        for fn, extra in ((fwd, ()), (inv, (st, fake, fake))):
            def call(src, t, B, Nr, Nc, lev, bank):
                return fn(src, t, B, Nr, Nc, lev, *extra, bank, allow)
            assert call(None, tab, 4, 64, 64, 3, C.byref(f)) == -1
            assert call(fake, None, 4, 64, 64, 3, C.byref(f)) == -1
            assert call(fake, hole, 4, 64, 64, 3, C.byref(f)) == -1
            assert call(fake, tab, 4, 64, 64, 3, None) == -1
            assert call(fake, tab, 0, 64, 64, 3, C.byref(f)) == -1
            assert call(fake, tab, -1, 64, 64, 3, C.byref(f)) == -1
            assert call(fake, tab, 65536, 64, 64, 3, C.byref(f)) == -1
            assert call(fake, tab, 65535, 512, 512, 4, C.byref(f)) == -1  # B 4^L > 2^22
            assert call(fake, tab, 4, 64, 64, 4, C.byref(f)) == -1        # deeper than the clamp: ilog2(64 / 7) = 3
            assert call(fake, tab, 4, 64, 64, 0, C.byref(f)) == -1
            assert call(fake, tab, 4, 6, 64, 1, C.byref(f)) == -1         # too small for one level
            assert call(fake, tab, 4, 0, 64, 1, C.byref(f)) == -1
            assert call(fake, tab, 4, 65536, 32768, 3, C.byref(f)) == -1  # Nr Nc = 2^31
            for bad in (0, 3, 42):
                g.hlen = bad
                assert call(fake, tab, 4, 64, 64, 3, C.byref(g)) == -1
        assert inv(fake, tab, 4, 64, 64, 3, None, fake, fake, C.byref(f), allow) == -1     # no state table
        assert inv(fake, tab, 4, 64, 64, 3, garbage, fake, fake, C.byref(f), allow) == -1  # not a table state_table writes
    assert inv(fake, tab, 4, 64, 64, 3, st, None, fake, C.byref(f), 1) == -1       # the fused form reads the device copy
    assert inv(fake, tab, 4, 64, 64, 3, mixed, fake, None, C.byref(f), 0) == -1    # the per-depth form reads the lists of a mixed depth
    assert inv(fake, tab, 4, 256, 256, 3, mixed, fake, None, C.byref(f), 1) == -1  # (beyond the budget: per depth whatever is allowed)


# ---- the host class without a device (its transcript of failed constructions: test_packets_host_cpu.py) -----------------------------
def test_class_refuses_to_construct_without_a_gpu():
    if pdwt_amd.hip().pdwt_device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(RuntimeError, match="no HIP device"):
        pdwt_amd.WaveletPacketBatch(np.zeros((2, 64, 64), np.float32), "db2", 2)
