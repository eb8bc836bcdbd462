"""No-GPU tests of the batched 2-D transform with boundary modes (dwt_ext2db.hip; BoundaryWaveletsImages, include/wt_ext.h): the exported
symbols, the plan of the fused path (pdwt_ext2db_fused: which side of the LDS rule each documented shape lies on), the scratch size, the
band shapes, every refusal of the drivers (refused before anything touches a device, so no device is needed), and the transcript of the
host class through its handle API after a failed construction, in the style of tests/test_boundary_host_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import pdwt_amd
from pdwt_amd import _native as N

PLAIN = ["pdwt_ext2db_fused", "pdwt_ext2db_tmp_elems"]
TYPED = ["ext2db_forward_level", "ext2db_inverse_level", "ext2db_forward", "ext2db_inverse"]
HANDLE = ["new", "delete", "forward", "inverse", "get_image", "set_image", "state", "mode_index", "num_bands", "get_coeff", "set_coeff", "image_int_ptr",
          "coeff_int_ptr", "soft_threshold", "hard_threshold", "norm1", "band_stats", "all_band_stats", "estimate_sigma", "threshold_bands", "denoise",
          "info", "geometry", "coeff_shape", "fused", "images_all_band_stats", "images_estimate_sigma", "images_threshold_bands", "images_denoise",
          "images_norm1"]
EINVAL = -1


def _hlen(wname):
    return pdwt_amd.hip().pdwt_compute_filters_separable_f32(wname.encode(), 0, None)


def test_symbols_are_exported_and_listed():
    L = pdwt_amd.hip()
    for s in PLAIN:
        assert hasattr(L, s) and s in N.PLAIN_SYMBOLS, s
    for t in TYPED:
        assert t in N.TYPED_SYMBOLS, t
        for sfx in ("f32", "f64"):
            assert hasattr(L, "pdwt_%s_%s" % (t, sfx)), (t, sfx)
    for dt in (np.float32, np.float64):
        H = N.host(dt)
        for n in HANDLE:
            assert hasattr(H, "pdwt_bwb_" + n), n
    assert "BoundaryImageBatch" in pdwt_amd.__all__


# (Nr, Nc, bank, levels, elem_size) -> fused
PLAN = [
    (64, 64, "db4", 3, 4, 1),     # 34 KB: below the 64 KiB opt-in
    (128, 128, "db4", 3, 4, 1),   # 132 KiB: above the opt-in
    (256, 256, "db4", 3, 4, 0),   # the image alone is 256 KiB
    (78, 80, "db20", 1, 8, 1),    # forward 49 920 + 73 632 B + tables; inverse with two child bands resident at a time
    (156, 160, "db20", 2, 8, 0),
    (128, 128, "db4", 3, 8, 0),   # the float64 image and its row-pass buffer: 262 KiB
    (160, 200, "db4", 3, 4, 0),
    (61, 67, "sym8", 2, 8, 1),
    (37, 51, "db3", 2, 8, 1),
    (9, 7, "haar", 2, 8, 1),
    (79, 81, "db20", 1, 8, 1),    # the largest all-banks shape: about 127 KB
]


@pytest.mark.parametrize("Nr,Nc,wname,levels,elem,fused", PLAN)
def test_plan_sides_and_scratch(Nr, Nc, wname, levels, elem, fused):
    L = pdwt_amd.hip()
    h = _hlen(wname)
    assert L.pdwt_ext2db_fused(Nr, Nc, h, levels, elem) == fused
    for B in (1, 5, 65535):
        want = 0 if fused else 2 * B * ((Nr + h - 1) // 2) * ((Nc + h - 1) // 2)
        assert L.pdwt_ext2db_tmp_elems(B, Nr, Nc, h, levels, elem) == want
    assert (L.pdwt_ext2db_tmp_elems(3, Nr, Nc, h, levels, elem) == 0) == bool(fused)


def test_plan_refuses_bad_arguments():
    L = pdwt_amd.hip()
    assert L.pdwt_ext2db_fused(64, 64, 8, 3, 2) == EINVAL and L.pdwt_ext2db_fused(64, 64, 7, 3, 4) == EINVAL
    assert L.pdwt_ext2db_fused(64, 64, 8, 0, 4) == EINVAL and L.pdwt_ext2db_fused(64, 64, 8, 33, 4) == EINVAL
    assert L.pdwt_ext2db_fused(6, 64, 8, 1, 4) == EINVAL  # an axis shorter than hlen - 1
    assert L.pdwt_ext2db_fused(65536, 32768, 2, 1, 4) == EINVAL
    assert L.pdwt_ext2db_tmp_elems(0, 256, 256, 8, 3, 4) == EINVAL and L.pdwt_ext2db_tmp_elems(65536, 256, 256, 8, 3, 4) == EINVAL


def test_band_shapes_are_those_of_the_2d_transform():
    L = pdwt_amd.hip()
    H = N.host(np.float32)
    nr, nc = (C.c_int * 8)(), (C.c_int * 8)()
    assert H.pdwt_bwb_geometry(37, 51, 6, 2, nr, nc) == 2 and list(nr[:3]) == [37, 21, 13] and list(nc[:3]) == [51, 28, 16]
    assert H.pdwt_bwb_geometry(64, 64, 8, 9, None, None) == 3 and H.pdwt_bwb_geometry(6, 6, 8, 1, None, None) == 0
    br, bc = C.c_int(), C.c_int()
    want = [(13, 16), (21, 28), (21, 28), (21, 28), (13, 16), (13, 16), (13, 16)]
    assert L.pdwt_num_bands_ext(37, 51, 6, 2) == 7
    for k, (r, c) in enumerate(want):
        assert L.pdwt_ext_band_shape(37, 51, 6, 2, k, C.byref(br), C.byref(bc)) == r * c and (br.value, bc.value) == (r, c)


@pytest.mark.parametrize("sfx,FT", [("f32", N.Filters32), ("f64", N.Filters64)])
def test_drivers_refuse_before_touching_a_device(sfx, FT):
    """Fake, never dereferenced addresses: every call below must return PDWT_EINVAL without a launch (a launch would fail: the test runs without a device)."""
    L = pdwt_amd.hip()
    f = FT()
    h = getattr(L, "pdwt_compute_filters_separable_" + sfx)(b"db4", 0, C.byref(f))
    f.hlen = h
    fr = C.byref(f)
    fwdl, invl = getattr(L, "pdwt_ext2db_forward_level_" + sfx), getattr(L, "pdwt_ext2db_inverse_level_" + sfx)
    fwd, inv = getattr(L, "pdwt_ext2db_forward_" + sfx), getattr(L, "pdwt_ext2db_inverse_" + sfx)
    p = 0x1000
    tab = (C.c_void_p * 4)(p, p, p, p)
    hole = (C.c_void_p * 4)(p, p, None, p)
    # the level drivers
    assert fwdl(p, p, p, p, p, 2, 16, 16, 5, fr) == EINVAL and fwdl(p, p, p, p, p, 2, 16, 16, -1, fr) == EINVAL   # mode
    assert fwdl(p, p, p, p, p, 0, 16, 16, 2, fr) == EINVAL and fwdl(p, p, p, p, p, 65536, 16, 16, 2, fr) == EINVAL  # B
    assert fwdl(p, p, p, p, p, 2, 6, 16, 2, fr) == EINVAL and fwdl(p, p, p, p, p, 2, 16, 6, 2, fr) == EINVAL        # n < hlen - 1
    assert fwdl(p, p, p, p, p, 2, 65536, 32768, 2, fr) == EINVAL
    for k in range(5):
        a = [p] * 5
        a[k] = None
        assert fwdl(*a, 2, 16, 16, 2, fr) == EINVAL and invl(*a, 2, 16, 16, fr) == EINVAL
    assert fwdl(p, p, p, p, p, 2, 16, 16, 2, None) == EINVAL and invl(p, p, p, p, p, 2, 16, 16, None) == EINVAL
    assert invl(p, p, p, p, p, 0, 16, 16, fr) == EINVAL and invl(p, p, p, p, p, 65536, 16, 16, fr) == EINVAL
    assert invl(p, p, p, p, p, 2, 6, 16, fr) == EINVAL
    # the whole-transform drivers
    assert fwd(p, tab, 2, 16, 16, 1, 5, fr, None) == EINVAL                                                  # mode 5
    assert fwd(p, tab, 2, 16, 16, 0, 2, fr, None) == EINVAL and inv(p, tab, 2, 16, 16, 0, fr, None) == EINVAL  # 0 levels
    assert fwd(p, tab, 0, 16, 16, 1, 2, fr, None) == EINVAL and inv(p, tab, 0, 16, 16, 1, fr, None) == EINVAL  # B < 1
    assert fwd(p, tab, 65536, 16, 16, 1, 2, fr, None) == EINVAL and inv(p, tab, 65536, 16, 16, 1, fr, None) == EINVAL
    assert fwd(None, tab, 2, 16, 16, 1, 2, fr, None) == EINVAL and inv(None, tab, 2, 16, 16, 1, fr, None) == EINVAL
    assert fwd(p, None, 2, 16, 16, 1, 2, fr, None) == EINVAL and inv(p, None, 2, 16, 16, 1, fr, None) == EINVAL
    assert fwd(p, hole, 2, 16, 16, 1, 2, fr, None) == EINVAL and inv(p, hole, 2, 16, 16, 1, fr, None) == EINVAL
    assert fwd(p, tab, 2, 16, 16, 1, 2, None, None) == EINVAL and inv(p, tab, 2, 16, 16, 1, None, None) == EINVAL
    assert fwd(p, tab, 2, 6, 16, 1, 2, fr, None) == EINVAL
    # a shape that runs per level needs its scratch
    assert L.pdwt_ext2db_fused(256, 256, h, 1, 4 if sfx == "f32" else 8) == 0
    assert fwd(p, tab, 2, 256, 256, 1, 2, fr, None) == EINVAL and inv(p, tab, 2, 256, 256, 1, fr, None) == EINVAL


# ---- the host class after a failed construction (tests/test_boundary_host_cpu.py for the new prefix) -----------------------------------
MODES = "(0 zero, 1 constant, 2 symmetric, 3 reflect, 4 periodic)"
CLS = "BoundaryWaveletsImages"
CASES = {
    "zero size": ((2, 0, 8, b"haar", 1, 2, 1), "ERROR: %s(): invalid image batch size or wavelet name\n" % CLS, "2 0 8 1 0 2"),
    "B 0": ((0, 8, 8, b"haar", 1, 2, 1), "ERROR: %s(): invalid image batch size or wavelet name\n" % CLS, "0 8 8 1 0 2"),
    "B 65536": ((65536, 8, 8, b"haar", 1, 2, 1), "ERROR: %s(): invalid image batch size or wavelet name\n" % CLS, "65536 8 8 1 0 2"),
    "too large": ((1, 65536, 32768, b"haar", 1, 2, 1), "ERROR: %s(): invalid image batch size or wavelet name\n" % CLS, "1 65536 32768 1 0 2"),
    "NULL name": ((2, 8, 8, None, 1, 2, 1), "ERROR: %s(): invalid image batch size or wavelet name\n" % CLS, "2 8 8 1 0 2"),
    "unknown bank": ((2, 8, 8, b"nosuch", 1, 2, 1), "ERROR: unknown wavelet name nosuch\n", "2 8 8 1 0 2"),
    "mode 5": ((2, 8, 8, b"haar", 1, 5, 1), "ERROR: %s(): unknown boundary mode 5 %s\n" % (CLS, MODES), "2 8 8 1 0 5"),
    "mode -1": ((2, 8, 8, b"haar", 1, -1, 1), "ERROR: %s(): unknown boundary mode -1 %s\n" % (CLS, MODES), "2 8 8 1 0 -1"),
    "too small": ((2, 6, 6, b"db4", 1, 2, 1),
                  "Warning: required level (1) is greater than the maximum possible level for db4 (0) on 6x6 images.\nForcing nlevels = 0\n"
                  "ERROR: 6x6 images are too small for one level of db4\n", "2 6 6 0 8 2"),
    "levels 0": ((2, 6, 6, b"db4", 0, 0, 1),
                 "Warning: cannot initialize wavelet coefficients with nlevels < 1. Forcing nlevels = 1\n"
                 "Warning: required level (1) is greater than the maximum possible level for db4 (0) on 6x6 images.\nForcing nlevels = 0\n"
                 "ERROR: 6x6 images are too small for one level of db4\n", "2 6 6 0 8 0"),
}
EXPECTED_METHODS = """\
state -> 4
num_bands -> 0
coeff_shape -> 0 (-7, -7, -7)
fused -> 0
forward
Warning: forward transform not computed, as there was an error when creating the wavelets
inverse
Warning: inverse transform not computed, as there was an error in a previous stage
soft_threshold
hard_threshold
norm1 -> -1.0
band_stats -> -1
all_band_stats -> -1
estimate_sigma -> -1.0
threshold_bands
denoise -> -1.0
images_all_band_stats -> -1
images_estimate_sigma -> -1
images_threshold_bands -> -1
images_denoise -> -1
images_norm1 -> -1
get_image -> 0
get_coeff -> 0
set_image
set_coeff
image_int_ptr -> 0
coeff_int_ptr -> 0
state -> 4
delete
"""
VOID = ("delete", "forward", "inverse", "soft_threshold", "hard_threshold", "set_image", "set_coeff", "threshold_bands")


def transcript(dtype, args, capfd):
    L = N.host(dtype)
    libc = C.CDLL(None)
    ct = C.c_float if np.dtype(dtype) == np.float32 else C.c_double
    lines = []

    def call(name, *a, show=None):
        capfd.readouterr()
        ret = getattr(L, "pdwt_bwb_" + name)(*a)
        libc.fflush(None)
        lines.append(name if name in VOID else "%s -> %s" % (name, show(ret) if show else ret))
        lines.extend(capfd.readouterr().out.splitlines())
        return ret

    h = call("new", None, *args, show=lambda r: "handle" if r else "NULL")
    assert h
    info = N.InfoBWB()
    call("info", h, C.byref(info), show=lambda r: " ".join(str(getattr(info, f)) for f in ("B", "Nr", "Nc", "nlevels", "hlen", "mode")))
    sz = [C.c_int(-7) for _ in range(3)]
    buf = np.zeros(64, dtype=dtype)
    p = buf.ctypes.data_as(C.c_void_p)
    dbl = (C.c_double * 8)()
    stats = (N.BandStats * 97)()
    call("state", h)
    call("num_bands", h)
    call("coeff_shape", h, 0, *[C.byref(s) for s in sz], show=lambda n: "%d (%s)" % (n, ", ".join(str(s.value) for s in sz)))
    call("fused", h)
    call("forward", h)
    call("inverse", h)
    call("soft_threshold", h, ct(1.0), 1)
    call("hard_threshold", h, ct(1.0), 0)
    call("norm1", h)
    call("band_stats", h, 0, stats, 1)
    call("all_band_stats", h, stats, 0)
    call("estimate_sigma", h)
    call("threshold_bands", h, p, 0)
    call("denoise", h, 1, C.c_double(-1.0), 0, p)
    call("images_all_band_stats", h, stats, 0)
    call("images_estimate_sigma", h, dbl)
    call("images_threshold_bands", h, p, 0)
    call("images_denoise", h, 1, None, 0, dbl, p)
    call("images_norm1", h, dbl)
    call("get_image", h, p)
    call("get_coeff", h, p, 0)
    call("set_image", h, p, 0)
    call("set_coeff", h, p, 0, 0)
    call("image_int_ptr", h)
    call("coeff_int_ptr", h, 0)
    call("state", h)
    call("delete", h)
    return "\n".join(lines) + "\n"


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("case", list(CASES))
def test_failed_construction_transcript(case, dtype, capfd):
    args, head, info = CASES[case]
    got = transcript(dtype, args, capfd)
    assert got == "new -> handle\n" + head + "info -> " + info + "\n" + EXPECTED_METHODS


def test_mode_names_are_those_of_the_other_classes():
    fn = N.host(np.float32).pdwt_bwb_mode_index
    assert [fn(m) for m in (b"zero", b"constant", b"symmetric", b"reflect", b"periodic", b"periodization", b"", None)] == [0, 1, 2, 3, 4, -1, -1, -1]
