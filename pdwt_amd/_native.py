"""ctypes bindings of the in-tree native libraries (pdwt_amd/lib/*.so).

There is NO CPU fallback: if a library is missing or no HIP device is visible, the product path
raises.  (The CPU oracle under oracle/ is test infrastructure and is never imported from here.)
"""
import ctypes as C
import os

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
# PDWT_LIBDIR: an alternative set of the in-tree libraries (diagnostic builds: tools/build_trace.sh, tools/ab_libs.sh)
LIBDIR = os.environ.get("PDWT_LIBDIR") or os.path.join(_PKG, "lib")


class Info3D(C.Structure):
    """== pdwt_info3d (include/pdwt_hip.h) == w_info3d (include/wt3d.h)."""
    _fields_ = [("Nz", C.c_int), ("Nr", C.c_int), ("Nc", C.c_int), ("nlevels", C.c_int), ("hlen", C.c_int)]


class InfoWPT(C.Structure):
    """== w_info_wpt (include/wpt.h)."""
    _fields_ = [("Nr", C.c_int), ("Nc", C.c_int), ("nlevels", C.c_int), ("hlen", C.c_int)]


class InfoWPT1(C.Structure):
    """== w_info_wpt1 (include/wpt1d.h)."""
    _fields_ = [("Nr", C.c_int), ("Nc", C.c_int), ("nlevels", C.c_int), ("hlen", C.c_int)]


class InfoWPTB(C.Structure):
    """== w_info_wptb (include/wpt_batch.h)."""
    _fields_ = [("B", C.c_int), ("Nr", C.c_int), ("Nc", C.c_int), ("nlevels", C.c_int), ("hlen", C.c_int)]


class InfoBW(C.Structure):
    """== w_info_bw (include/wt_ext.h)."""
    _fields_ = [("Nr", C.c_int), ("Nc", C.c_int), ("nlevels", C.c_int), ("hlen", C.c_int), ("mode", C.c_int)]


class InfoBWB(C.Structure):
    """== w_info_bwb (include/wt_ext.h)."""
    _fields_ = [("B", C.c_int), ("Nr", C.c_int), ("Nc", C.c_int), ("nlevels", C.c_int), ("hlen", C.c_int), ("mode", C.c_int)]


class InfoBW3(C.Structure):
    """== w_info_bw3 (include/wt_ext.h)."""
    _fields_ = [("Nz", C.c_int), ("Nr", C.c_int), ("Nc", C.c_int), ("nlevels", C.c_int), ("hlen", C.c_int), ("mode", C.c_int)]


class BandStats(C.Structure):
    """== pdwt_band_stats (include/pdwt_hip.h) == w_band_stats (include/wt.h)."""
    _fields_ = [("n", C.c_double), ("sum_abs", C.c_double), ("sum_sq", C.c_double), ("max_abs", C.c_double), ("median_abs", C.c_double)]

    def as_dict(self):
        return {k: float(getattr(self, k)) for k, _ in self._fields_}


class Info(C.Structure):
    """== pdwt_info (include/pdwt_hip.h) == reference w_info (src/utils.h:9-19)."""
    _fields_ = [("ndims", C.c_int), ("Nr", C.c_int), ("Nc", C.c_int), ("nlevels", C.c_int), ("do_swt", C.c_int), ("hlen", C.c_int)]

    def __repr__(self):
        return "Info(ndims=%d, Nr=%d, Nc=%d, nlevels=%d, do_swt=%d, hlen=%d)" % (self.ndims, self.Nr, self.Nc, self.nlevels, self.do_swt, self.hlen)


def _filters_struct(ct):
    class F(C.Structure):
        _fields_ = [("hlen", C.c_int), ("L", ct * 40), ("H", ct * 40), ("IL", ct * 40), ("IH", ct * 40)]
    return F


Filters32 = _filters_struct(C.c_float)
Filters64 = _filters_struct(C.c_double)

DRIVERS = ["forward_separable", "forward_separable_1d", "inverse_separable", "inverse_separable_1d",
           "forward_swt_separable", "forward_swt_separable_1d", "inverse_swt_separable", "inverse_swt_separable_1d"]
HAAR_DRIVERS = ["haar_forward2d", "haar_inverse2d", "haar_forward1d", "haar_inverse1d"]

# every symbol include/pdwt_hip.h declares (checked by tests/test_cabi_symbols.py)
PLAIN_SYMBOLS = ["pdwt_device_count", "pdwt_set_device", "pdwt_get_device", "pdwt_device_name", "pdwt_malloc", "pdwt_free",
                 "pdwt_memset", "pdwt_memcpy_h2d", "pdwt_memcpy_d2h", "pdwt_memcpy_d2d", "pdwt_memcpy_d2d_foreign", "pdwt_set_stream", "pdwt_sync", "pdwt_get_stream",
                 "pdwt_last_error_string", "pdwt_event_create", "pdwt_event_record", "pdwt_event_sync", "pdwt_event_elapsed_ms",
                 "pdwt_event_destroy", "pdwt_ktime_enable", "pdwt_ktime_reset", "pdwt_ktime_read", "pdwt_kernel_name",
                 "pdwt_kernel_count", "pdwt_graph_allowed", "pdwt_graph_capture_begin", "pdwt_graph_capture_end", "pdwt_graph_launch",
                 "pdwt_graph_destroy", "pdwt_num_wavelets", "pdwt_wavelet_name", "pdwt_num_bands", "pdwt_band_size", "pdwt_tmp_elems", "pdwt_debug_set", "pdwt_debug_get", "pdwt_clock_probe_enable", "pdwt_clock_probe_read", "pdwt_clock_probe_dump", "pdwt_probe_bandwidth", "pdwt_selfcheck_vmcnt_order", "pdwt_rccl_available", "pdwt_rccl_allreduce_sum_f64", "pdwt_sum_result_index", "pdwt_sum_spare_index",
                 "pdwt_batch2d_create_f32", "pdwt_batch2d_forward_f32", "pdwt_batch2d_inverse_f32", "pdwt_batch2d_destroy",
                 "pdwt_batch2d_create_f64", "pdwt_batch2d_forward_f64", "pdwt_batch2d_inverse_f64", "pdwt_batch2d_destroy_f64",
                 "pdwt_sum_scratch_doubles", "pdwt_sum_scratch_read", "pdwt_num_bands3d", "pdwt_band_size3d", "pdwt_tmp_elems3d",
                 "pdwt_num_bands_swt3d", "pdwt_band_size_swt3d", "pdwt_tmp_elems_swt3d", "pdwt_num_bands_ext", "pdwt_ext_band_shape",
                 "pdwt_num_bands_ext1d", "pdwt_ext1d_band_len", "pdwt_ext1d_fused", "pdwt_ext1d_tmp_elems",
                 "pdwt_ext2db_fused", "pdwt_ext2db_tmp_elems", "pdwt_ext2db_adjoint_tmp_elems", "pdwt_ext1d_adjoint_tmp_elems",
                 "pdwt_num_bands_ext3d", "pdwt_ext3d_band_shape", "pdwt_ext3d_tmp_elems", "pdwt_ext3d_tmp_approx_offset",
                 "pdwt_ext3d_adjoint_level_tmp_elems", "pdwt_ext3d_adjoint_z_run", "pdwt_ext3db_tmp_elems", "pdwt_ext3db_adjoint_tmp_elems",
                 "pdwt_wp1_geometry", "pdwt_wp1_fused", "pdwt_wp1_tmp_elems", "pdwt_wp1_frequency_order", "pdwt_wp1_state_table", "pdwt_memcpy2d",
                 "pdwt_wptb_geometry", "pdwt_wptb_fused", "pdwt_wptb_lds_bytes", "pdwt_wptb_tmp_elems", "pdwt_wptb_state_table", "pdwt_wptb_chunk_lists"]
TYPED_SYMBOLS = (["compute_filters_separable", "create_coeffs_buffer", "free_coeffs_buffer", "copy_coeffs_buffer",
                  "soft_thresh", "soft_thresh_sum", "norm1", "norm1_as_double", "norm1_enqueue", "hard_thresh", "proj_linf", "shrink", "group_soft_thresh",
                  "norm2sq", "norm2sq_as_double", "add_coeffs", "circshift", "forward_nonseparable", "inverse_nonseparable",
                  "forward_swt_nonseparable", "inverse_swt_nonseparable",
                  "create_coeffs_buffer3d", "free_coeffs_buffer3d", "forward3d_separable", "inverse3d_separable", "soft_thresh3d", "hard_thresh3d",
                  "norm1_3d", "create_coeffs_buffer_swt3d", "free_coeffs_buffer_swt3d", "forward3d_swt", "inverse3d_swt",
                  "soft_thresh_swt3d", "hard_thresh_swt3d", "norm1_swt3d", "bandlist_stats", "bandlist_thresh", "bandbatch_stats", "bandbatch_thresh",
                  "wpt2d_forward_level", "wpt2d_inverse_level", "wpt2d_node_cost", "ext2d_forward_level", "ext2d_inverse_level",
                  "ext1d_forward_level", "ext1d_inverse_level", "ext1d_forward", "ext1d_inverse",
                  "ext3d_forward_level", "ext3d_inverse_level", "ext3d_forward_adjoint_level", "ext3d_inverse_adjoint_level",
                  "ext3db_forward", "ext3db_inverse", "ext3db_forward_adjoint", "ext3db_inverse_adjoint",
                  "ext2db_forward_level", "ext2db_inverse_level", "ext2db_forward", "ext2db_inverse",
                  "ext2db_forward_adjoint_level", "ext2db_forward_adjoint", "ext2db_inverse_adjoint",
                  "ext1d_forward_adjoint_level", "ext1d_forward_adjoint", "ext1d_inverse_adjoint",
                  "wp1_forward_level", "wp1_inverse_level", "wp1_forward", "wp1_inverse", "wp1_moments", "wp1_thresh",
                  "wptb_forward", "wptb_inverse"] + DRIVERS + HAAR_DRIVERS)

_hip = None
_host = {}


def _require(path):
    if not os.path.exists(path):
        raise RuntimeError("%s is missing: build the native libraries first (python -m pdwt_amd.build); "
                           "pdwt_amd has no CPU fallback" % path)
    return path


def hip():
    """libpdwt_hip.so with argument/return types set."""
    global _hip
    if _hip is not None:
        return _hip
    L = C.CDLL(_require(os.path.join(LIBDIR, "libpdwt_hip.so")), mode=C.RTLD_GLOBAL)
    vp, ci, sz = C.c_void_p, C.c_int, C.c_size_t
    L.pdwt_malloc.restype = vp
    L.pdwt_malloc.argtypes = [sz]
    L.pdwt_free.argtypes = [vp]
    L.pdwt_memset.argtypes = [vp, ci, sz]
    L.pdwt_set_stream.argtypes = [vp, ci]
    for n in ("pdwt_memcpy_h2d", "pdwt_memcpy_d2h", "pdwt_memcpy_d2d", "pdwt_memcpy_d2d_foreign"):
        getattr(L, n).argtypes = [vp, vp, sz]
    L.pdwt_get_stream.restype = vp
    L.pdwt_last_error_string.restype = C.c_char_p
    L.pdwt_device_name.argtypes = [C.c_char_p, ci]
    L.pdwt_event_create.restype = vp
    for n in ("pdwt_event_record", "pdwt_event_sync", "pdwt_event_destroy"):
        getattr(L, n).argtypes = [vp]
    L.pdwt_probe_bandwidth.argtypes = [vp, vp, C.c_size_t, ci]
    L.pdwt_selfcheck_vmcnt_order.restype = C.c_longlong
    L.pdwt_event_elapsed_ms.restype = C.c_float
    L.pdwt_event_elapsed_ms.argtypes = [vp, vp]
    L.pdwt_ktime_read.argtypes = [ci, C.POINTER(ci), C.POINTER(C.c_double)]
    L.pdwt_kernel_name.restype = C.c_char_p
    L.pdwt_kernel_name.argtypes = [ci]
    L.pdwt_wavelet_name.restype = C.c_char_p
    L.pdwt_wavelet_name.argtypes = [ci]
    L.pdwt_num_bands.argtypes = [Info]
    L.pdwt_band_size.restype = C.c_longlong
    L.pdwt_band_size.argtypes = [Info, ci, C.POINTER(ci), C.POINTER(ci)]
    L.pdwt_clock_probe_enable.argtypes = [ci]
    L.pdwt_batch2d_create_f32.restype = vp
    L.pdwt_batch2d_create_f32.argtypes = [ci, vp, vp, vp, Info]
    L.pdwt_batch2d_forward_f32.argtypes = [vp, vp]
    L.pdwt_batch2d_inverse_f32.argtypes = [vp, vp]
    L.pdwt_batch2d_destroy.argtypes = [vp]
    L.pdwt_batch2d_create_f64.restype = vp
    L.pdwt_batch2d_create_f64.argtypes = [ci, vp, vp, vp, Info]
    L.pdwt_batch2d_forward_f64.argtypes = [vp, vp]
    L.pdwt_batch2d_inverse_f64.argtypes = [vp, vp]
    L.pdwt_batch2d_destroy_f64.argtypes = [vp]
    L.pdwt_clock_probe_dump.argtypes = [vp, ci]
    L.pdwt_sum_scratch_doubles.restype = sz
    L.pdwt_sum_result_index.restype = sz
    L.pdwt_sum_spare_index.restype = sz
    L.pdwt_sum_scratch_read.argtypes = [vp, C.POINTER(C.c_double)]
    L.pdwt_clock_probe_read.argtypes = [ci, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.pdwt_debug_set.argtypes = [C.c_char_p, ci]
    L.pdwt_debug_get.argtypes = [C.c_char_p, C.POINTER(ci)]
    L.pdwt_tmp_elems.restype = sz
    L.pdwt_tmp_elems.argtypes = [Info]
    L.pdwt_num_bands3d.argtypes = [Info3D]
    L.pdwt_band_size3d.restype = C.c_longlong
    L.pdwt_band_size3d.argtypes = [Info3D, ci, C.POINTER(ci), C.POINTER(ci), C.POINTER(ci)]
    L.pdwt_tmp_elems3d.restype = sz
    L.pdwt_tmp_elems3d.argtypes = [Info3D]
    L.pdwt_num_bands_swt3d.argtypes = [Info3D]
    L.pdwt_band_size_swt3d.restype = C.c_longlong
    L.pdwt_band_size_swt3d.argtypes = [Info3D, ci, C.POINTER(ci), C.POINTER(ci), C.POINTER(ci)]
    L.pdwt_tmp_elems_swt3d.restype = sz
    L.pdwt_tmp_elems_swt3d.argtypes = [Info3D]
    L.pdwt_num_bands_ext.argtypes = [ci, ci, ci, ci]
    L.pdwt_ext_band_shape.restype = C.c_longlong
    L.pdwt_ext_band_shape.argtypes = [ci, ci, ci, ci, ci, C.POINTER(ci), C.POINTER(ci)]
    for sfx, ct, FT in (("f32", C.c_float, Filters32), ("f64", C.c_double, Filters64)):
        P = C.POINTER(ct)
        PP = C.POINTER(P)
        f = getattr(L, "pdwt_compute_filters_separable_" + sfx)
        f.argtypes = [C.c_char_p, ci, C.POINTER(FT)]
        f = getattr(L, "pdwt_create_coeffs_buffer_" + sfx)
        f.restype = PP
        f.argtypes = [Info]
        getattr(L, "pdwt_free_coeffs_buffer_" + sfx).argtypes = [PP, Info]
        getattr(L, "pdwt_copy_coeffs_buffer_" + sfx).argtypes = [PP, PP, Info]
        getattr(L, "pdwt_soft_thresh_" + sfx).argtypes = [PP, ct, Info, ci, ci]
        getattr(L, "pdwt_norm1_" + sfx).argtypes = [PP, Info, P]
        getattr(L, "pdwt_norm1_as_double_" + sfx).argtypes = [PP, Info, C.POINTER(C.c_double)]
        getattr(L, "pdwt_norm1_enqueue_" + sfx).argtypes = [PP, Info, vp]
        getattr(L, "pdwt_soft_thresh_sum_" + sfx).argtypes = [PP, ct, Info, ci, ci, vp]
        for n in ("hard_thresh", "group_soft_thresh"):
            getattr(L, "pdwt_%s_%s" % (n, sfx)).argtypes = [PP, ct, Info, ci, ci]
        for n in ("proj_linf", "shrink"):
            getattr(L, "pdwt_%s_%s" % (n, sfx)).argtypes = [PP, ct, Info, ci]
        getattr(L, "pdwt_norm2sq_" + sfx).argtypes = [PP, Info, P]
        getattr(L, "pdwt_norm2sq_as_double_" + sfx).argtypes = [PP, Info, C.POINTER(C.c_double)]
        getattr(L, "pdwt_add_coeffs_" + sfx).argtypes = [PP, PP, Info, ct]
        getattr(L, "pdwt_circshift_" + sfx).argtypes = [vp, vp, Info, ci, ci, ci]
        for d in DRIVERS:
            getattr(L, "pdwt_%s_%s" % (d, sfx)).argtypes = [vp, PP, vp, Info, C.POINTER(FT)]
        for d in HAAR_DRIVERS:
            getattr(L, "pdwt_%s_%s" % (d, sfx)).argtypes = [vp, PP, vp, Info]
        f = getattr(L, "pdwt_create_coeffs_buffer3d_" + sfx)
        f.restype = PP
        f.argtypes = [Info3D]
        getattr(L, "pdwt_free_coeffs_buffer3d_" + sfx).argtypes = [PP, Info3D]
        for d in ("forward3d_separable", "inverse3d_separable"):
            getattr(L, "pdwt_%s_%s" % (d, sfx)).argtypes = [vp, PP, vp, Info3D, C.POINTER(FT)]
        for d in ("soft_thresh3d", "hard_thresh3d"):
            getattr(L, "pdwt_%s_%s" % (d, sfx)).argtypes = [PP, ct, Info3D, ci, ci]
        getattr(L, "pdwt_norm1_3d_" + sfx).argtypes = [PP, Info3D, C.POINTER(C.c_double)]
        f = getattr(L, "pdwt_create_coeffs_buffer_swt3d_" + sfx)
        f.restype = PP
        f.argtypes = [Info3D]
        getattr(L, "pdwt_free_coeffs_buffer_swt3d_" + sfx).argtypes = [PP, Info3D]
        for d in ("forward3d_swt", "inverse3d_swt"):
            getattr(L, "pdwt_%s_%s" % (d, sfx)).argtypes = [vp, PP, vp, Info3D, C.POINTER(FT)]
        for d in ("soft_thresh_swt3d", "hard_thresh_swt3d"):
            getattr(L, "pdwt_%s_%s" % (d, sfx)).argtypes = [PP, ct, Info3D, ci, ci]
        getattr(L, "pdwt_norm1_swt3d_" + sfx).argtypes = [PP, Info3D, C.POINTER(C.c_double)]
        getattr(L, "pdwt_bandlist_stats_" + sfx).argtypes = [PP, C.POINTER(sz), ci, C.POINTER(C.c_ubyte), C.POINTER(BandStats)]
        getattr(L, "pdwt_bandlist_thresh_" + sfx).argtypes = [ci, PP, C.POINTER(sz), P, ci]
        # the same over a regular batch: the table of B * nb band pointers is a DEVICE address
        getattr(L, "pdwt_bandbatch_stats_" + sfx).argtypes = [vp, C.POINTER(sz), ci, ci, C.POINTER(C.c_ubyte), C.POINTER(BandStats)]
        getattr(L, "pdwt_bandbatch_thresh_" + sfx).argtypes = [ci, vp, C.POINTER(sz), P, ci, ci]
        # 2-D wavelet packets, one depth step: (parents, children, nr, nc, device node list or NULL, count, bank)
        for d in ("wpt2d_forward_level", "wpt2d_inverse_level"):
            getattr(L, "pdwt_%s_%s" % (d, sfx)).argtypes = [vp, vp, ci, ci, vp, ci, C.POINTER(FT)]
        getattr(L, "pdwt_wpt2d_node_cost_" + sfx).argtypes = [vp, sz, ci, ci, C.POINTER(C.c_double)]
        # 2-D DWT with boundary modes, one level: (image, A, H, V, D, nr, nc, [mode,] bank)
        getattr(L, "pdwt_ext2d_forward_level_" + sfx).argtypes = [vp, vp, vp, vp, vp, ci, ci, ci, C.POINTER(FT)]
        getattr(L, "pdwt_ext2d_inverse_level_" + sfx).argtypes = [vp, vp, vp, vp, vp, ci, ci, C.POINTER(FT)]
        # batched 1-D with boundary modes: one level (src, a, d, nr, nc, mode, bank) / (dst, a, d, nr, nc, bank); all levels (src or dst,
        # HOST table of levels + 1 device pointers, nr, nc, levels, [mode,] bank, scratch or NULL) -> 1 fused / 0 per level / < 0
        getattr(L, "pdwt_ext1d_forward_level_" + sfx).argtypes = [vp, vp, vp, ci, ci, ci, C.POINTER(FT)]
        getattr(L, "pdwt_ext1d_inverse_level_" + sfx).argtypes = [vp, vp, vp, ci, ci, C.POINTER(FT)]
        getattr(L, "pdwt_ext1d_forward_" + sfx).argtypes = [vp, C.POINTER(vp), ci, ci, ci, ci, C.POINTER(FT), vp]
        getattr(L, "pdwt_ext1d_inverse_" + sfx).argtypes = [vp, C.POINTER(vp), ci, ci, ci, C.POINTER(FT), vp]
        # volumes with boundary modes, one level: (volume, HOST table of the 8 band pointers aaa .. ddd, nz, nr, nc, [mode,] bank, scratch)
        getattr(L, "pdwt_ext3d_forward_level_" + sfx).argtypes = [vp, C.POINTER(vp), ci, ci, ci, ci, C.POINTER(FT), vp]
        getattr(L, "pdwt_ext3d_inverse_level_" + sfx).argtypes = [vp, C.POINTER(vp), ci, ci, ci, C.POINTER(FT), vp]
        # their adjoints: (dst, HOST table of the 8 cotangent bands, nz, nr, nc, mode, bank, scratch) / (src, table, nz, nr, nc, bank, scratch)
        getattr(L, "pdwt_ext3d_forward_adjoint_level_" + sfx).argtypes = [vp, C.POINTER(vp), ci, ci, ci, ci, C.POINTER(FT), vp]
        getattr(L, "pdwt_ext3d_inverse_adjoint_level_" + sfx).argtypes = [vp, C.POINTER(vp), ci, ci, ci, C.POINTER(FT), vp]
        for name in ("forward", "forward_adjoint"):
            getattr(L, "pdwt_ext3db_%s_%s" % (name, sfx)).argtypes = [vp, C.POINTER(vp), ci, ci, ci, ci, ci, ci, C.POINTER(FT), vp]
        for name in ("inverse", "inverse_adjoint"):
            getattr(L, "pdwt_ext3db_%s_%s" % (name, sfx)).argtypes = [vp, C.POINTER(vp), ci, ci, ci, ci, ci, C.POINTER(FT), vp]
        # batched 2-D with boundary modes: one level of B images (src, A, H, V, D stacks, B, nr, nc, [mode,] bank); all levels (src or dst,
        # HOST table of 3 * levels + 1 device pointers, B, Nr, Nc, levels, [mode,] bank, scratch or NULL) -> 1 fused / 0 per level / < 0
        getattr(L, "pdwt_ext2db_forward_level_" + sfx).argtypes = [vp, vp, vp, vp, vp, ci, ci, ci, ci, C.POINTER(FT)]
        getattr(L, "pdwt_ext2db_inverse_level_" + sfx).argtypes = [vp, vp, vp, vp, vp, ci, ci, ci, C.POINTER(FT)]
        getattr(L, "pdwt_ext2db_forward_" + sfx).argtypes = [vp, C.POINTER(vp), ci, ci, ci, ci, ci, C.POINTER(FT), vp]
        getattr(L, "pdwt_ext2db_inverse_" + sfx).argtypes = [vp, C.POINTER(vp), ci, ci, ci, ci, C.POINTER(FT), vp]
        # adjoints of the boundary-mode transforms: the forward adjoints take the output first, the cotangent bands like the inverse, and
        # a scratch last; the inverse adjoints have the arguments of the forward entries without the mode
        getattr(L, "pdwt_ext2db_forward_adjoint_level_" + sfx).argtypes = [vp, vp, vp, vp, vp, ci, ci, ci, ci, C.POINTER(FT), vp]
        getattr(L, "pdwt_ext2db_forward_adjoint_" + sfx).argtypes = [vp, C.POINTER(vp), ci, ci, ci, ci, ci, C.POINTER(FT), vp]
        getattr(L, "pdwt_ext2db_inverse_adjoint_" + sfx).argtypes = [vp, C.POINTER(vp), ci, ci, ci, ci, C.POINTER(FT), vp]
        getattr(L, "pdwt_ext1d_forward_adjoint_level_" + sfx).argtypes = [vp, vp, vp, ci, ci, ci, C.POINTER(FT), vp]
        getattr(L, "pdwt_ext1d_forward_adjoint_" + sfx).argtypes = [vp, C.POINTER(vp), ci, ci, ci, ci, C.POINTER(FT), vp]
        getattr(L, "pdwt_ext1d_inverse_adjoint_" + sfx).argtypes = [vp, C.POINTER(vp), ci, ci, ci, C.POINTER(FT), vp]
        # batched 1-D wavelet packets: one depth step (parents, children, nr, nnodes, n, [device list or NULL, count,] bank); the whole
        # tree (src or dst, HOST table of `levels` device pointers, nr, nc, levels, [device state table,] bank) -> 1 fused / 0 per level / < 0
        getattr(L, "pdwt_wp1_forward_level_" + sfx).argtypes = [vp, vp, ci, ci, ci, C.POINTER(FT)]
        getattr(L, "pdwt_wp1_inverse_level_" + sfx).argtypes = [vp, vp, ci, ci, ci, vp, ci, C.POINTER(FT)]
        getattr(L, "pdwt_wp1_forward_" + sfx).argtypes = [vp, C.POINTER(vp), ci, ci, ci, C.POINTER(FT)]
        getattr(L, "pdwt_wp1_inverse_" + sfx).argtypes = [vp, C.POINTER(vp), ci, ci, ci, vp, C.POINTER(FT)]
        getattr(L, "pdwt_wp1_moments_" + sfx).argtypes = [vp, C.c_longlong, ci, C.POINTER(C.c_double)]
        getattr(L, "pdwt_wp1_thresh_" + sfx).argtypes = [ci, vp, ci, ci, ci, vp, ct]
        getattr(L, "pdwt_wptb_forward_" + sfx).argtypes = [vp, C.POINTER(vp), ci, ci, ci, ci, C.POINTER(FT), ci]
        getattr(L, "pdwt_wptb_inverse_" + sfx).argtypes = [vp, C.POINTER(vp), ci, ci, ci, ci, C.POINTER(C.c_ubyte), vp, vp, C.POINTER(FT), ci]
    L.pdwt_wp1_geometry.argtypes = [ci, ci, ci, C.POINTER(ci)]
    L.pdwt_wptb_geometry.argtypes = [ci, ci, ci, ci, C.POINTER(ci), C.POINTER(ci)]
    L.pdwt_wptb_fused.argtypes = [ci, ci, ci, ci, ci]
    L.pdwt_wptb_lds_bytes.restype = C.c_longlong
    L.pdwt_wptb_lds_bytes.argtypes = [ci, ci, ci, ci, ci, ci]
    L.pdwt_wptb_tmp_elems.restype = C.c_longlong
    L.pdwt_wptb_tmp_elems.argtypes = [ci, ci, ci, ci, ci, ci, ci]
    L.pdwt_wptb_state_table.argtypes = [ci, C.POINTER(ci), C.POINTER(ci), ci, C.POINTER(C.c_ubyte)]
    L.pdwt_wptb_chunk_lists.restype = C.c_longlong
    L.pdwt_wptb_chunk_lists.argtypes = [ci, ci, C.POINTER(C.c_ubyte), C.POINTER(ci)]
    L.pdwt_wp1_fused.argtypes = [ci, ci, ci, ci]
    L.pdwt_wp1_tmp_elems.restype = C.c_longlong
    L.pdwt_wp1_tmp_elems.argtypes = [ci, ci, ci, ci, ci]
    L.pdwt_wp1_frequency_order.argtypes = [ci, C.POINTER(ci)]
    L.pdwt_wp1_state_table.argtypes = [ci, C.POINTER(ci), C.POINTER(ci), ci, C.POINTER(C.c_ubyte)]
    L.pdwt_memcpy2d.argtypes = [vp, sz, vp, sz, sz, sz, ci]
    L.pdwt_num_bands_ext3d.argtypes = [ci, ci, ci, ci, ci]
    L.pdwt_ext3d_band_shape.restype = C.c_longlong
    L.pdwt_ext3d_band_shape.argtypes = [ci, ci, ci, ci, ci, ci, C.POINTER(ci), C.POINTER(ci), C.POINTER(ci)]
    L.pdwt_ext3d_tmp_elems.restype = C.c_longlong
    L.pdwt_ext3d_tmp_elems.argtypes = [ci, ci, ci, ci]
    L.pdwt_ext3d_tmp_approx_offset.restype = C.c_longlong
    L.pdwt_ext3d_tmp_approx_offset.argtypes = [ci, ci, ci, ci]
    L.pdwt_ext3d_adjoint_level_tmp_elems.restype = C.c_longlong
    L.pdwt_ext3d_adjoint_level_tmp_elems.argtypes = [ci, ci, ci, ci]
    L.pdwt_ext3d_adjoint_z_run.argtypes = [ci, ci, ci, C.POINTER(ci), C.POINTER(ci)]
    L.pdwt_ext3db_tmp_elems.restype = C.c_longlong
    L.pdwt_ext3db_tmp_elems.argtypes = [ci, ci, ci, ci, ci, ci]
    L.pdwt_ext3db_adjoint_tmp_elems.restype = C.c_longlong
    L.pdwt_ext3db_adjoint_tmp_elems.argtypes = [ci, ci, ci, ci, ci, ci]
    L.pdwt_num_bands_ext1d.argtypes = [ci, ci, ci]
    L.pdwt_ext1d_band_len.restype = C.c_longlong
    L.pdwt_ext1d_band_len.argtypes = [ci, ci, ci, ci]
    L.pdwt_ext1d_fused.argtypes = [ci, ci, ci, ci]
    L.pdwt_ext1d_tmp_elems.restype = C.c_longlong
    L.pdwt_ext1d_tmp_elems.argtypes = [ci, ci, ci, ci, ci]
    L.pdwt_ext2db_fused.argtypes = [ci, ci, ci, ci, ci]
    L.pdwt_ext2db_tmp_elems.restype = C.c_longlong
    L.pdwt_ext2db_tmp_elems.argtypes = [ci, ci, ci, ci, ci, ci]
    L.pdwt_ext2db_adjoint_tmp_elems.restype = C.c_longlong
    L.pdwt_ext2db_adjoint_tmp_elems.argtypes = [ci, ci, ci, ci, ci, ci]
    L.pdwt_ext1d_adjoint_tmp_elems.restype = C.c_longlong
    L.pdwt_ext1d_adjoint_tmp_elems.argtypes = [ci, ci, ci, ci, ci]
    _hip = L
    return L


def host(dtype):
    """libpdwt.so (float32) / libpdwtd.so (float64): the C++ Wavelets class behind a C handle API."""
    dt = np.dtype(dtype)
    if dt not in _host:
        hip()  # resolve libpdwt_hip.so first (same directory, RTLD_GLOBAL)
        name = {np.dtype(np.float32): "libpdwt.so", np.dtype(np.float64): "libpdwtd.so"}[dt]
        L = C.CDLL(_require(os.path.join(LIBDIR, name)))
        ct = C.c_float if dt == np.float32 else C.c_double
        vp, ci = C.c_void_p, C.c_int
        assert L.pdwt_wavelets_sizeof_dtype() == dt.itemsize
        L.pdwt_wavelets_new.restype = vp
        L.pdwt_wavelets_new.argtypes = [vp, ci, ci, C.c_char_p, ci, ci, ci, ci, ci, ci]
        L.pdwt_wavelets_copy.restype = vp
        L.pdwt_wavelets_copy.argtypes = [vp]
        L.pdwt_wavelets_delete.argtypes = [vp]
        for n in ("forward", "inverse", "print_informations"):
            getattr(L, "pdwt_wavelets_" + n).argtypes = [vp]
        L.pdwt_wavelets_soft_threshold.argtypes = [vp, ct, ci, ci]
        L.pdwt_wavelets_norm1.restype = ct
        L.pdwt_wavelets_norm1.argtypes = [vp]
        L.pdwt_wavelets_norm1_f64.restype = C.c_double
        L.pdwt_wavelets_norm1_f64.argtypes = [vp]
        L.pdwt_wavelets_set_norm_cache.argtypes = [vp, ci]
        L.pdwt_wavelets_norm1_begin.argtypes = [vp]
        L.pdwt_wavelets_norm1_end.restype = C.c_double
        L.pdwt_wavelets_norm1_end.argtypes = [vp]
        L.pdwt_wavelets_norm2sq.restype = ct
        L.pdwt_wavelets_norm2sq.argtypes = [vp]
        for n in ("hard_threshold", "group_soft_threshold"):
            getattr(L, "pdwt_wavelets_" + n).argtypes = [vp, ct, ci, ci]
        for n in ("shrink", "proj_linf"):
            getattr(L, "pdwt_wavelets_" + n).argtypes = [vp, ct, ci]
        L.pdwt_wavelets_circshift.argtypes = [vp, ci, ci, ci]
        L.pdwt_wavelets_set_filters_forward.argtypes = [vp, C.c_char_p, C.c_uint, vp, vp]
        L.pdwt_wavelets_set_filters_inverse.argtypes = [vp, vp, vp]
        L.pdwt_wavelets_set_filters_forward4.argtypes = [vp, C.c_char_p, C.c_uint, vp, vp, vp, vp]
        L.pdwt_wavelets_set_filters_inverse4.argtypes = [vp, vp, vp, vp, vp]
        L.pdwt_wavelets_add_wavelet.argtypes = [vp, vp, ct]
        L.pdwt_wavelets_shifts.argtypes = [vp, C.POINTER(ci), C.POINTER(ci)]
        L.pdwt_wavelets_get_image.argtypes = [vp, vp]
        L.pdwt_wavelets_set_image.argtypes = [vp, vp, ci]
        L.pdwt_wavelets_get_coeff.argtypes = [vp, vp, ci]
        L.pdwt_wavelets_set_coeff.argtypes = [vp, vp, ci, ci]
        L.pdwt_wavelets_state.argtypes = [vp]
        L.pdwt_wavelets_set_state.argtypes = [vp, ci]
        L.pdwt_wavelets_info.argtypes = [vp, C.POINTER(Info)]
        for n in ("image_int_ptr", "coeffs_table_ptr", "tmp_int_ptr"):
            getattr(L, "pdwt_wavelets_" + n).restype = C.c_ssize_t
            getattr(L, "pdwt_wavelets_" + n).argtypes = [vp]
        L.pdwt_images_new.restype = vp
        L.pdwt_images_new.argtypes = [vp, ci, ci, ci, C.c_char_p, ci, ci]
        L.pdwt_images_new_swt.restype = vp
        L.pdwt_images_new_swt.argtypes = [vp, ci, ci, ci, C.c_char_p, ci, ci, ci]
        L.pdwt_images_at.restype = vp
        L.pdwt_images_at.argtypes = [vp, ci]
        for n in ("delete", "ok", "batched", "forward", "inverse"):
            getattr(L, "pdwt_images_" + n).argtypes = [vp]
        L.pdwt_images_num_bands.argtypes = [vp]
        L.pdwt_images_all_band_stats.argtypes = [vp, C.POINTER(BandStats), ci]
        L.pdwt_images_estimate_sigma.argtypes = [vp, C.POINTER(C.c_double)]
        L.pdwt_images_threshold_bands.argtypes = [vp, vp, ci]
        L.pdwt_images_denoise.argtypes = [vp, ci, C.POINTER(C.c_double), ci, C.POINTER(C.c_double), vp]
        L.pdwt_images_norm1.argtypes = [vp, C.POINTER(C.c_double)]
        L.pdwt_wavelets_coeff_int_ptr.restype = C.c_ssize_t
        L.pdwt_wavelets_coeff_int_ptr.argtypes = [vp, ci]
        # Wavelets3D (include/wt3d.h) and StationaryWavelets3D (include/swt3d.h), both in wt3d.cpp: the same handle API
        for pfx in ("pdwt_wavelets3d_", "pdwt_swt3d_"):
            getattr(L, pfx + "new").restype = vp
            getattr(L, pfx + "new").argtypes = [vp, ci, ci, ci, C.c_char_p, ci, ci]
            for n in ("delete", "forward", "inverse", "num_bands", "state"):
                getattr(L, pfx + n).argtypes = [vp]
            for n in ("soft_threshold", "hard_threshold"):
                getattr(L, pfx + n).argtypes = [vp, ct, ci, ci]
            getattr(L, pfx + "norm1").restype = ct
            getattr(L, pfx + "norm1").argtypes = [vp]
            getattr(L, pfx + "norm1_f64").restype = C.c_double
            getattr(L, pfx + "norm1_f64").argtypes = [vp]
            getattr(L, pfx + "get_image").argtypes = [vp, vp]
            getattr(L, pfx + "set_image").argtypes = [vp, vp, ci]
            getattr(L, pfx + "band_shape").restype = C.c_longlong
            getattr(L, pfx + "band_shape").argtypes = [vp, ci, C.POINTER(ci), C.POINTER(ci), C.POINTER(ci)]
            getattr(L, pfx + "get_coeff").argtypes = [vp, vp, ci]
            getattr(L, pfx + "set_coeff").argtypes = [vp, vp, ci, ci]
            getattr(L, pfx + "info").argtypes = [vp, C.POINTER(Info3D)]
            getattr(L, pfx + "image_int_ptr").restype = C.c_ssize_t
            getattr(L, pfx + "image_int_ptr").argtypes = [vp]
            getattr(L, pfx + "coeff_int_ptr").restype = C.c_ssize_t
            getattr(L, pfx + "coeff_int_ptr").argtypes = [vp, ci]
        # band statistics and noise-adaptive thresholds: the same five handle functions on the four classes
        for pfx in ("pdwt_wavelets_", "pdwt_wavelets3d_", "pdwt_swt3d_", "pdwt_bw_", "pdwt_bw1_", "pdwt_bw3_", "pdwt_bwb_"):
            getattr(L, pfx + "band_stats").argtypes = [vp, ci, C.POINTER(BandStats), ci]
            getattr(L, pfx + "all_band_stats").argtypes = [vp, C.POINTER(BandStats), ci]
            getattr(L, pfx + "estimate_sigma").restype = C.c_double
            getattr(L, pfx + "estimate_sigma").argtypes = [vp]
            getattr(L, pfx + "threshold_bands").argtypes = [vp, vp, ci]
            getattr(L, pfx + "denoise").restype = C.c_double
            getattr(L, pfx + "denoise").argtypes = [vp, ci, C.c_double, ci, vp]
        # WaveletPackets, WaveletPackets1D, WaveletPacketsImages (include/wpt.h, wpt1d.h, wpt_batch.h; wpt.cpp): the handle functions the three
        # share, then those whose arguments or return types are their class's
        pi = C.POINTER(ci)
        pd, pll = C.POINTER(C.c_double), C.POINTER(C.c_longlong)
        for pfx in ("pdwt_wpt_", "pdwt_wp1h_", "pdwt_wpbh_"):
            for n in ("delete", "forward", "inverse", "state", "basis_size"):
                getattr(L, pfx + n).argtypes = [vp]
            getattr(L, pfx + "set_image").argtypes = [vp, vp, ci]
            getattr(L, pfx + "node_shape").restype = C.c_longlong
            getattr(L, pfx + "node_shape").argtypes = [vp, ci, pi, pi]
            getattr(L, pfx + "path_index").argtypes = [C.c_char_p, pi]
            getattr(L, pfx + "get_image").argtypes = [vp, vp]
            getattr(L, pfx + "get_node").argtypes = [vp, vp, ci, ci]
            getattr(L, pfx + "get_level").restype = C.c_longlong
            getattr(L, pfx + "get_level").argtypes = [vp, vp, ci]
            getattr(L, pfx + "set_node").argtypes = [vp, vp, ci, ci, ci]
            getattr(L, pfx + "node_int_ptr").restype = C.c_ssize_t
            getattr(L, pfx + "best_basis").argtypes = [vp, ci]
            getattr(L, pfx + "set_basis").argtypes = [vp, pi, pi, ci]
            getattr(L, pfx + "get_basis").argtypes = [vp, pi, pi]
            for n in ("soft_threshold", "hard_threshold"):
                getattr(L, pfx + n).argtypes = [vp, ct, ci]
            getattr(L, pfx + "norm1").restype = C.c_double
            getattr(L, pfx + "norm1").argtypes = [vp]
            getattr(L, pfx + "node_stats").argtypes = [vp, ci, C.POINTER(BandStats)]
            getattr(L, pfx + "estimate_sigma").restype = C.c_double
            getattr(L, pfx + "estimate_sigma").argtypes = [vp]
        L.pdwt_wpt_new.restype = L.pdwt_wp1h_new.restype = L.pdwt_wpbh_new.restype = vp
        L.pdwt_wpt_new.argtypes = L.pdwt_wp1h_new.argtypes = [vp, ci, ci, C.c_char_p, ci, ci]
        L.pdwt_wpbh_new.argtypes = [vp, ci, ci, ci, C.c_char_p, ci, ci, ci]
        L.pdwt_wpt_info.argtypes = [vp, C.POINTER(InfoWPT)]
        L.pdwt_wp1h_info.argtypes = [vp, C.POINTER(InfoWPT1)]
        L.pdwt_wpbh_info.argtypes = [vp, C.POINTER(InfoWPTB)]
        L.pdwt_wpt_geometry.argtypes = L.pdwt_wpbh_geometry.argtypes = [ci, ci, ci, ci, pi, pi]
        L.pdwt_wp1h_geometry.argtypes = [ci, ci, ci, pi]
        L.pdwt_wp1h_frequency_order.argtypes = [ci, pi]
        L.pdwt_wp1h_fused.argtypes = L.pdwt_wpbh_fused.argtypes = [vp]
        L.pdwt_wpt_node_int_ptr.argtypes = [vp, ci, ci]
        L.pdwt_wp1h_node_int_ptr.argtypes = L.pdwt_wpbh_node_int_ptr.argtypes = [vp, ci, ci, pll]
        L.pdwt_wpt_node_costs.argtypes = [vp, ci, ci, pd]
        L.pdwt_wp1h_node_costs.argtypes = L.pdwt_wpbh_node_costs.argtypes = [vp, ci, ci, pd, pd]
        for n in ("get_image", "get_node", "set_node"):  # the element counts of a stack
            getattr(L, "pdwt_wpbh_" + n).restype = C.c_longlong
        L.pdwt_wpbh_images_norm1.argtypes = L.pdwt_wpbh_images_estimate_sigma.argtypes = [vp, pd]
        # BoundaryWavelets (include/wt_ext.h, wt_ext.cpp)
        L.pdwt_bw_new.restype = vp
        L.pdwt_bw_new.argtypes = [vp, ci, ci, C.c_char_p, ci, ci, ci]
        for n in ("delete", "forward", "inverse", "state", "num_bands"):
            getattr(L, "pdwt_bw_" + n).argtypes = [vp]
        L.pdwt_bw_get_image.argtypes = [vp, vp]
        L.pdwt_bw_set_image.argtypes = [vp, vp, ci]
        L.pdwt_bw_info.argtypes = [vp, C.POINTER(InfoBW)]
        L.pdwt_bw_geometry.argtypes = [ci, ci, ci, ci, pi, pi]
        L.pdwt_bw_mode_index.argtypes = [C.c_char_p]
        L.pdwt_bw_coeff_shape.restype = C.c_longlong
        L.pdwt_bw_coeff_shape.argtypes = [vp, ci, pi, pi]
        L.pdwt_bw_get_coeff.argtypes = [vp, vp, ci]
        L.pdwt_bw_set_coeff.argtypes = [vp, vp, ci, ci]
        L.pdwt_bw_image_int_ptr.restype = C.c_ssize_t
        L.pdwt_bw_image_int_ptr.argtypes = [vp]
        L.pdwt_bw_coeff_int_ptr.restype = C.c_ssize_t
        L.pdwt_bw_coeff_int_ptr.argtypes = [vp, ci]
        for n in ("soft_threshold", "hard_threshold"):
            getattr(L, "pdwt_bw_" + n).argtypes = [vp, ct, ci]
        L.pdwt_bw_norm1.restype = C.c_double
        L.pdwt_bw_norm1.argtypes = [vp]
        L.pdwt_bw1_new.restype = vp
        L.pdwt_bw1_new.argtypes = [vp, ci, ci, C.c_char_p, ci, ci, ci]
        for n in ("delete", "forward", "inverse", "state", "num_bands", "fused"):
            getattr(L, "pdwt_bw1_" + n).argtypes = [vp]
        L.pdwt_bw1_get_image.argtypes = [vp, vp]
        L.pdwt_bw1_set_image.argtypes = [vp, vp, ci]
        L.pdwt_bw1_info.argtypes = [vp, C.POINTER(InfoBW)]
        L.pdwt_bw1_geometry.argtypes = [ci, ci, ci, pi]
        L.pdwt_bw1_mode_index.argtypes = [C.c_char_p]
        L.pdwt_bw1_coeff_shape.restype = C.c_longlong
        L.pdwt_bw1_coeff_shape.argtypes = [vp, ci, pi, pi]
        L.pdwt_bw1_get_coeff.argtypes = [vp, vp, ci]
        L.pdwt_bw1_set_coeff.argtypes = [vp, vp, ci, ci]
        L.pdwt_bw1_image_int_ptr.restype = C.c_ssize_t
        L.pdwt_bw1_image_int_ptr.argtypes = [vp]
        L.pdwt_bw1_coeff_int_ptr.restype = C.c_ssize_t
        L.pdwt_bw1_coeff_int_ptr.argtypes = [vp, ci]
        for n in ("soft_threshold", "hard_threshold"):
            getattr(L, "pdwt_bw1_" + n).argtypes = [vp, ct, ci]
        L.pdwt_bw1_norm1.restype = C.c_double
        L.pdwt_bw1_norm1.argtypes = [vp]
        L.pdwt_bw3_new.restype = vp
        L.pdwt_bw3_new.argtypes = [vp, ci, ci, ci, C.c_char_p, ci, ci, ci]
        for n in ("delete", "forward", "inverse", "state", "num_bands"):
            getattr(L, "pdwt_bw3_" + n).argtypes = [vp]
        L.pdwt_bw3_get_image.argtypes = [vp, vp]
        L.pdwt_bw3_set_image.argtypes = [vp, vp, ci]
        L.pdwt_bw3_info.argtypes = [vp, C.POINTER(InfoBW3)]
        L.pdwt_bw3_geometry.argtypes = [ci, ci, ci, ci, ci, pi, pi, pi]
        L.pdwt_bw3_mode_index.argtypes = [C.c_char_p]
        L.pdwt_bw3_coeff_shape.restype = C.c_longlong
        L.pdwt_bw3_coeff_shape.argtypes = [vp, ci, pi, pi, pi]
        L.pdwt_bw3_get_coeff.argtypes = [vp, vp, ci]
        L.pdwt_bw3_set_coeff.argtypes = [vp, vp, ci, ci]
        L.pdwt_bw3_image_int_ptr.restype = C.c_ssize_t
        L.pdwt_bw3_image_int_ptr.argtypes = [vp]
        L.pdwt_bw3_coeff_int_ptr.restype = C.c_ssize_t
        L.pdwt_bw3_coeff_int_ptr.argtypes = [vp, ci]
        for n in ("soft_threshold", "hard_threshold"):
            getattr(L, "pdwt_bw3_" + n).argtypes = [vp, ct, ci]
        L.pdwt_bw3_norm1.restype = C.c_double
        L.pdwt_bw3_norm1.argtypes = [vp]
        # BoundaryWaveletsImages: the handle API of the three above, and the per-image statistics (the signatures of pdwt_images_*)
        L.pdwt_bwb_new.restype = vp
        L.pdwt_bwb_new.argtypes = [vp, ci, ci, ci, C.c_char_p, ci, ci, ci]
        for n in ("delete", "forward", "inverse", "state", "num_bands", "fused"):
            getattr(L, "pdwt_bwb_" + n).argtypes = [vp]
        L.pdwt_bwb_get_image.argtypes = [vp, vp]
        L.pdwt_bwb_set_image.argtypes = [vp, vp, ci]
        L.pdwt_bwb_info.argtypes = [vp, C.POINTER(InfoBWB)]
        L.pdwt_bwb_geometry.argtypes = [ci, ci, ci, ci, pi, pi]
        L.pdwt_bwb_mode_index.argtypes = [C.c_char_p]
        L.pdwt_bwb_coeff_shape.restype = C.c_longlong
        L.pdwt_bwb_coeff_shape.argtypes = [vp, ci, pi, pi, pi]
        L.pdwt_bwb_get_coeff.argtypes = [vp, vp, ci]
        L.pdwt_bwb_set_coeff.argtypes = [vp, vp, ci, ci]
        L.pdwt_bwb_image_int_ptr.restype = C.c_ssize_t
        L.pdwt_bwb_image_int_ptr.argtypes = [vp]
        L.pdwt_bwb_coeff_int_ptr.restype = C.c_ssize_t
        L.pdwt_bwb_coeff_int_ptr.argtypes = [vp, ci]
        for n in ("soft_threshold", "hard_threshold"):
            getattr(L, "pdwt_bwb_" + n).argtypes = [vp, ct, ci]
        L.pdwt_bwb_norm1.restype = C.c_double
        L.pdwt_bwb_norm1.argtypes = [vp]
        L.pdwt_bwb_images_all_band_stats.argtypes = [vp, C.POINTER(BandStats), ci]
        L.pdwt_bwb_images_estimate_sigma.argtypes = [vp, C.POINTER(C.c_double)]
        L.pdwt_bwb_images_threshold_bands.argtypes = [vp, vp, ci]
        L.pdwt_bwb_images_denoise.argtypes = [vp, ci, C.POINTER(C.c_double), ci, C.POINTER(C.c_double), vp]
        L.pdwt_bwb_images_norm1.argtypes = [vp, C.POINTER(C.c_double)]
        _host[dt] = L
    return _host[dt]


def require_gpu():
    n = hip().pdwt_device_count()
    if n <= 0:
        raise RuntimeError("pdwt_amd: no HIP device visible (MI355X required; there is no CPU fallback)")
    return n
