"""CPU-only: the host side of BoundaryWavelets3D in the built libraries, no GPU needed.

  * pdwt_bw3_geometry and pdwt_bw3_mode_index against tests/refext3d.py on all the cases of the GPU tests, the clamps and the refusals;
  * every construction that fails before a device allocation, through the handle API (zero size, NULL / unknown bank, bad mode,
    6 x 6 x 6 db4 = 0 levels, Nz = 70000): W_CREATION_ERROR, and then every method answers what the 2-D class answers on a failed
    instance (both are asked here);
  * the PDWT_EINVAL answers of the three geometry entries and of the level drivers (a refused call dereferences nothing).
"""
import ctypes as C

import numpy as np
import pytest

from tests import refext3d as R3

_ids = ["%dx%dx%d-%s" % (c[0] + (c[1],)) for c in R3.CASES]


def _host():
    from pdwt_amd import _native as N
    return N, N.hip(), N.host(np.float32), N.host(np.float64)


@pytest.mark.parametrize("case", R3.CASES, ids=_ids)
def test_library_geometry_equals_the_reference(case):
    shape, wname, levels, _ = case
    N, hip, h32, h64 = _host()
    F, _ = R3.bank(wname)
    want = R3.band_shapes(shape, F, levels)
    assert hip.pdwt_num_bands_ext3d(*shape, F, levels) == len(want) == 7 * levels + 1
    for k, s in enumerate(want):
        bz, br, bc = C.c_int(), C.c_int(), C.c_int()
        assert hip.pdwt_ext3d_band_shape(*shape, F, levels, k, C.byref(bz), C.byref(br), C.byref(bc)) == s[0] * s[1] * s[2]
        assert (bz.value, br.value, bc.value) == s, k
    assert hip.pdwt_ext3d_band_shape(*shape, F, levels, len(want), None, None, None) == -1
    assert hip.pdwt_ext3d_band_shape(*shape, F, levels, -1, None, None, None) == -1
    s1 = R3.level_shapes(shape, F, 1)[1]
    pad = lambda n: (n + 63) // 64 * 64  # noqa: E731
    assert hip.pdwt_ext3d_tmp_elems(*shape, F) == pad(4 * shape[0] * s1[1] * s1[2]) + pad(s1[0] * s1[1] * s1[2])
    assert hip.pdwt_ext3d_tmp_approx_offset(*shape, F) == pad(4 * shape[0] * s1[1] * s1[2])
    clamped = R3.clamp_levels(shape, F, levels)
    for L in (h32, h64):
        nz, nr, nc = (C.c_int * 14)(), (C.c_int * 14)(), (C.c_int * 14)()
        assert L.pdwt_bw3_geometry(*shape, F, levels, nz, nr, nc) == clamped
        assert [(nz[l], nr[l], nc[l]) for l in range(clamped + 1)] == R3.level_shapes(shape, F, clamped)
    # db4 on 7^3 and db20 on 40 x 48 x 40: ilog2(7 / 7) = ilog2(40 / 39) = 0 levels, the level drivers take them
    assert clamped == (0 if shape in R3.DRIVER_CASES else levels)


def test_geometry_clamps_and_refusals():
    N, hip, h32, h64 = _host()
    g = h32.pdwt_bw3_geometry
    assert g(96, 80, 120, 8, 9, None, None, None) == 3       # ilog2(80 / 7)
    assert g(28, 200, 200, 8, 9, None, None, None) == 2      # the shortest axis decides: ilog2(28 / 7)
    assert g(64, 64, 64, 4, 0, None, None, None) == 1        # levels < 1 asks for 1
    assert g(6, 64, 64, 8, 2, None, None, None) == 0 and g(64, 64, 6, 8, 2, None, None, None) == 0  # too small for one level
    assert g(64, 64, 64, 7, 2, None, None, None) == 0 and g(64, 64, 64, 42, 1, None, None, None) == 0
    assert g(70000, 64, 64, 4, 1, None, None, None) == 0     # Nz is a grid dimension
    assert g(4, 1 << 16, 1 << 15, 2, 1, None, None, None) == 0  # Nr * Nc >= 2^31
    assert h64.pdwt_bw3_geometry(65535, 1 << 15, 1 << 15, 2, 40, None, None, None) == 13  # ilog2(2^15) = 15, clamped to 13 (92 bands)
    assert g(0, 64, 64, 4, 1, None, None, None) == 0
    assert [h32.pdwt_bw3_mode_index(m.encode()) for m in R3.MODES] == [0, 1, 2, 3, 4]
    assert h32.pdwt_bw3_mode_index(b"smooth") == -1 and h32.pdwt_bw3_mode_index(b"periodization") == -1 and h32.pdwt_bw3_mode_index(None) == -1


def test_the_geometry_entries_answer_einval():
    N, hip, h32, h64 = _host()
    nb, bs, tm, ao = hip.pdwt_num_bands_ext3d, hip.pdwt_ext3d_band_shape, hip.pdwt_ext3d_tmp_elems, hip.pdwt_ext3d_tmp_approx_offset
    assert nb(7, 7, 7, 8, 1) == 8 and nb(64, 64, 64, 4, 13) == 92 and tm(7, 7, 7, 8) > 0
    bad = [(6, 64, 64, 8), (64, 6, 64, 8), (64, 64, 6, 8),   # an axis below hlen - 1
           (0, 64, 64, 2), (64, 0, 64, 2), (64, 64, 0, 2),
           (64, 64, 64, 7), (64, 64, 64, 0), (64, 64, 64, 42),  # bank lengths
           (70000, 64, 64, 4), (65536, 64, 64, 2),               # nz <= 65535
           (4, 1 << 16, 1 << 15, 2)]                            # a plane of 2^31 elements
    for z, r, c, h in bad:
        assert nb(z, r, c, h, 1) == -1, (z, r, c, h)
        assert bs(z, r, c, h, 1, 0, None, None, None) == -1, (z, r, c, h)
        assert tm(z, r, c, h) == -1 and ao(z, r, c, h) == -1, (z, r, c, h)
    assert nb(65535, 64, 64, 2, 1) == 8
    assert nb(64, 64, 64, 4, 14) == -1 and nb(64, 64, 64, 4, 0) == -1
    assert bs(64, 64, 64, 4, 2, 15, None, None, None) == -1 and bs(64, 64, 64, 4, 2, 14, None, None, None) == 33 ** 3


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_constructions_that_fail_before_any_device_allocation(dt):
    """W_CREATION_ERROR from the constructor, and every method of the failed instance gives what BoundaryWavelets gives on one."""
    from pdwt_amd.wavelets import W_CREATION_ERROR
    N, hip, h32, h64 = _host()
    L = h32 if dt == np.float32 else h64
    ct = C.c_float if dt == np.float32 else C.c_double
    buf = np.zeros(64, dt)
    p = buf.ctypes.data_as(C.c_void_p)
    stats = (N.BandStats * 4)()

    def answers(pfx, h, nshape):
        f = lambda n: getattr(L, pfx + n)  # noqa: E731
        f("forward")(h)
        f("inverse")(h)
        out = [f("state")(h), f("num_bands")(h), f("coeff_shape")(h, 0, *([None] * nshape)), f("get_image")(h, p), f("get_coeff")(h, p, 0),
               f("image_int_ptr")(h), f("coeff_int_ptr")(h, 0), f("norm1")(h), f("band_stats")(h, 0, stats, 1), f("all_band_stats")(h, stats, 0),
               f("estimate_sigma")(h), f("denoise")(h, 0, -1.0, 0, p), f("denoise")(h, 1, 1.0, 1, None)]
        f("set_image")(h, p, 0)
        f("set_coeff")(h, p, 0, 0)
        f("soft_threshold")(h, ct(1.0), 1)
        f("hard_threshold")(h, ct(1.0), 0)
        f("threshold_bands")(h, p, 0)
        out.append(f("state")(h))
        return out

    cases3 = [((0, 64, 64), b"db2", 1, 2), ((64, 0, 64), b"db2", 1, 2), ((64, 64, 0), b"db2", 1, 2), ((64, 64, 64), None, 1, 2),
              ((64, 64, 64), b"nosuchwavelet", 1, 2), ((64, 64, 64), b"db2", 1, 5), ((64, 64, 64), b"db2", 1, -1), ((6, 6, 6), b"db4", 2, 2),
              ((70000, 8, 8), b"db2", 1, 2)]
    try:
        h2 = L.pdwt_bw_new(None, 6, 64, b"db4", 2, 2, 1)  # the 2-D class on a failed instance: the yardstick
        assert h2 and L.pdwt_bw_state(h2) == W_CREATION_ERROR
        want = answers("pdwt_bw_", h2, 2)
        L.pdwt_bw_delete(h2)
        assert want[0] == want[-1] == W_CREATION_ERROR and want[1:7] == [0] * 6 and want[7] == -1.0
        for shape, wname, levels, mode in cases3:
            h = L.pdwt_bw3_new(None, shape[0], shape[1], shape[2], wname, levels, mode, 1)
            assert h and L.pdwt_bw3_state(h) == W_CREATION_ERROR, (shape, wname, mode)
            info = N.InfoBW3()
            L.pdwt_bw3_info(h, C.byref(info))
            assert (info.Nz, info.Nr, info.Nc, info.mode) == shape + (mode,)
            assert answers("pdwt_bw3_", h, 3) == want, (shape, wname, mode)
            L.pdwt_bw3_delete(h)
    finally:
        C.CDLL(None).fflush(None)  # the class reports on the C stdout: leave nothing in its buffer for a later test's capture


@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_the_level_drivers_refuse_bad_arguments_without_a_device(dt):
    N, hip, h32, h64 = _host()
    sfx = "f32" if dt == np.float32 else "f64"
    f = (N.Filters32 if dt == np.float32 else N.Filters64)()
    assert getattr(hip, "pdwt_compute_filters_separable_" + sfx)(b"db4", 0, C.byref(f)) == 8
    f.hlen = 8
    buf = np.zeros(64, dt)  # host memory: a refused call dereferences nothing
    p = buf.ctypes.data
    tab = (C.c_void_p * 8)(*([p] * 8))
    hole = (C.c_void_p * 8)(*([p] * 5 + [None] + [p] * 2))
    fwd, inv = getattr(hip, "pdwt_ext3d_forward_level_" + sfx), getattr(hip, "pdwt_ext3d_inverse_level_" + sfx)
    assert fwd(p, tab, 16, 16, 16, 5, C.byref(f), p) == -1 and fwd(p, tab, 16, 16, 16, -1, C.byref(f), p) == -1
    for shape in ((6, 16, 16), (16, 6, 16), (16, 16, 6), (70000, 16, 16), (0, 16, 16)):
        assert fwd(p, tab, *shape, 2, C.byref(f), p) == -1 and inv(p, tab, *shape, C.byref(f), p) == -1, shape
    assert fwd(None, tab, 16, 16, 16, 2, C.byref(f), p) == -1 and fwd(p, None, 16, 16, 16, 2, C.byref(f), p) == -1
    assert fwd(p, hole, 16, 16, 16, 2, C.byref(f), p) == -1 and inv(p, hole, 16, 16, 16, C.byref(f), p) == -1
    assert fwd(p, tab, 16, 16, 16, 2, None, p) == -1 and fwd(p, tab, 16, 16, 16, 2, C.byref(f), None) == -1
    assert inv(None, tab, 16, 16, 16, C.byref(f), p) == -1 and inv(p, tab, 16, 16, 16, C.byref(f), None) == -1
    f.hlen = 7
    assert fwd(p, tab, 16, 16, 16, 2, C.byref(f), p) == -1 and inv(p, tab, 16, 16, 16, C.byref(f), p) == -1
