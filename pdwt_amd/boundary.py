"""Python view of the C++ ``BoundaryWavelets`` class (include/wt_ext.h): the multi-level 2-D DWT with signal-extension boundary modes
-- ``zero``, ``constant``, ``symmetric`` (the default, as in PyWavelets), ``reflect``, ``periodic`` -- instead of the periodisation of
``Wavelets``.  The bands are those of ``pywt.wavedec2(img, wname, mode, levels)``, in the order of ``Wavelets``:
``[A_L, H1, V1, D1, ..., H_L, V_L, D_L]`` (level 1 the finest), each level ``(n + hlen - 1) // 2`` per axis.

``BoundaryWavelets1D`` (C++ ``BoundaryWavelets1D``) is the same along the last axis of a batch of rows: ``pywt.wavedec(x, wname, mode,
levels, axis=-1)``, bands ``[A_L, D_1, ..., D_L]``, all levels in one kernel launch when a row fits the LDS of a workgroup.

``BoundaryWavelets3D`` (C++ ``BoundaryWavelets3D``) is the same along the three axes of a volume: ``pywt.wavedecn(vol, wname, mode,
levels)``, bands in the order of ``Wavelets3D``.

``BoundaryImageBatch`` (C++ ``BoundaryWaveletsImages``) is the 2-D transform of every image of a ``(B, Nr, Nc)`` batch:
``pywt.wavedec2(x, wname, mode, levels, axes=(-2, -1))``, the whole pyramid of an image in one workgroup when it fits LDS, and the
per-image statistics and denoising of ``ImageBatch``.
"""
import ctypes as C

import numpy as np

from . import _native as N
from .wavelets import DeviceArray, W_CREATION_ERROR, W_INVERSE, _BandStatsAPI, _device_source, _sync_producer
from .wavelets3d import BAND_KEYS

MODES = {"zero": 0, "constant": 1, "symmetric": 2, "reflect": 3, "periodic": 4}


class BoundaryWavelets2D(_BandStatsAPI):
    """BoundaryWavelets2D(img, wname, levels, mode="symmetric", dtype=None): ``img`` is a 2-D numpy array or a contiguous float32 /
    float64 device tensor (copied device to device, as ``Wavelets`` does).  Same state machine as ``Wavelets``; ``forward()`` leaves
    the image intact and ``inverse()`` leaves the bands intact.  Levels are clamped to ilog2(min(Nr, Nc) / (hlen - 1)); an image too
    small for one level, an unknown wavelet or an unknown mode number gives state W_CREATION_ERROR (an unknown mode NAME is a
    ``ValueError`` here)."""

    _hpfx = "pdwt_bw_"

    def __init__(self, img, wname, levels, mode="symmetric", dtype=None):
        N.require_gpu()
        if isinstance(mode, str):
            if mode not in MODES:
                raise ValueError("mode must be one of %s" % ", ".join(MODES))
            mode = MODES[mode]
        dev = _device_source(img)
        if dev is not None:
            ptr, shape, dt = dev
            if dtype is not None and np.dtype(dtype) != dt:
                raise TypeError("dtype does not match the device tensor")
            _sync_producer()
            src, on_host, keep = C.c_void_p(ptr), 0, None
        else:
            img = np.asarray(img)
            dt = np.dtype(dtype or (img.dtype if img.dtype in (np.float32, np.float64) else np.float32))
            keep = np.ascontiguousarray(img, dtype=dt)
            shape, src, on_host = keep.shape, keep.ctypes.data_as(C.c_void_p), 1
        shape = self._shape2(tuple(int(v) for v in shape))
        self.dtype, self.shape, self.wname = np.dtype(dt), tuple(int(v) for v in shape), wname
        self._L = N.host(self.dtype)
        self._ct = C.c_float if self.dtype == np.float32 else C.c_double
        self._h = self._bs("new")(src, *self.shape, wname.encode(), int(levels), int(mode), on_host)
        del keep
        if not self._h:
            raise MemoryError("%s allocation failed" % type(self).__name__)

    @staticmethod
    def _shape2(shape):
        if len(shape) != 2:
            raise ValueError("BoundaryWavelets2D needs a 2-D image (Nr, Nc)")
        return shape

    def close(self):
        if getattr(self, "_h", None):
            self._bs("delete")(self._h)
        self._h = None

    __del__ = close

    # -- introspection ---------------------------------------------------------------------
    _info_t = N.InfoBW

    @property
    def info(self):
        i = self._info_t()
        self._bs("info")(self._h, C.byref(i))
        return i

    @property
    def levels(self):
        return self.info.nlevels

    @property
    def mode(self):
        """The name of the boundary mode (the number as given if it is not one of the five)."""
        m = self.info.mode
        return {v: k for k, v in MODES.items()}.get(m, m)

    @property
    def state(self):
        return self._bs("state")(self._h)

    @property
    def nbands(self):
        return self._bs("num_bands")(self._h)

    def coeff_shape(self, num):
        r, c = C.c_int(), C.c_int()
        if self._bs("coeff_shape")(self._h, int(num), C.byref(r), C.byref(c)) <= 0:
            raise IndexError(num)
        return r.value, c.value

    band_shape = coeff_shape

    def _need_coeffs(self, what):
        if self.state in (W_INVERSE, W_CREATION_ERROR):
            raise RuntimeError("%s refused (state=%d): the coefficients are not valid" % (what, self.state))

    # -- transforms ------------------------------------------------------------------------
    def forward(self):
        self._bs("forward")(self._h)

    def inverse(self):
        self._bs("inverse")(self._h)

    # -- data in and out -------------------------------------------------------------------
    def get_image(self):
        out = np.empty(self.shape, dtype=self.dtype)
        if self._bs("get_image")(self._h, out.ctypes.data_as(C.c_void_p)) != out.size:
            raise RuntimeError("get_image failed (state=%d)" % self.state)
        return out

    def _upload(self, fn, arr, n, *args):
        dev = _device_source(arr)
        if dev is not None:
            if dev[2] != self.dtype or int(np.prod(dev[1])) != n:
                raise ValueError("device array of the wrong dtype or size")
            _sync_producer()
            return fn(self._h, C.c_void_p(dev[0]), *args, 1)
        a = np.ascontiguousarray(arr, dtype=self.dtype)
        if a.size != n:
            raise ValueError("array of the wrong size")
        return fn(self._h, a.ctypes.data_as(C.c_void_p), *args, 0)

    def set_image(self, img):
        if self.state == W_CREATION_ERROR:
            raise RuntimeError("set_image refused (state=%d)" % self.state)
        self._upload(self._bs("set_image"), img, int(np.prod(self.shape)))

    def get_coeff(self, num):
        self._need_coeffs("get_coeff")
        out = np.empty(self.coeff_shape(num), dtype=self.dtype)
        if self._bs("get_coeff")(self._h, out.ctypes.data_as(C.c_void_p), int(num)) != out.size:
            raise RuntimeError("get_coeff(%d) failed (state=%d)" % (num, self.state))
        return out

    def set_coeff(self, arr, num):
        """Overwrite one band (numpy array or device tensor).  Allowed in every state but W_CREATION_ERROR; the state stays."""
        self._upload(self._bs("set_coeff"), arr, int(np.prod(self.coeff_shape(num))), int(num))

    @property
    def coeffs(self):
        return [self.get_coeff(k) for k in range(self.nbands)]

    def image_int_ptr(self):
        return self._bs("image_int_ptr")(self._h)

    def coeff_int_ptr(self, num):
        self.coeff_shape(num)
        return self._bs("coeff_int_ptr")(self._h, int(num))

    def image_view(self):
        """The image as a zero-copy DeviceArray (call ``sync()`` before a consumer on another stream reads it)."""
        return DeviceArray(self, self.image_int_ptr(), self.shape, self.dtype)

    def coeff_view(self, num):
        """Band ``num`` as a zero-copy DeviceArray."""
        return DeviceArray(self, self.coeff_int_ptr(num), self.coeff_shape(num), self.dtype)

    def sync(self):
        return N.hip().pdwt_sync()

    # -- thresholds and norms ----------------------------------------------------------------
    def soft_threshold(self, beta, do_thresh_appcoeffs=0):
        """In place on every detail band; the approximation only when ``do_thresh_appcoeffs``."""
        self._need_coeffs("soft_threshold")
        self._bs("soft_threshold")(self._h, self._ct(beta), int(do_thresh_appcoeffs))

    def hard_threshold(self, beta, do_thresh_appcoeffs=0):
        self._need_coeffs("hard_threshold")
        self._bs("hard_threshold")(self._h, self._ct(beta), int(do_thresh_appcoeffs))

    def norm1(self):
        """Sum of |c| over all bands, in double."""
        v = float(self._bs("norm1")(self._h))
        if v < 0:
            raise RuntimeError("norm1 refused (state=%d): the coefficients are not valid" % self.state)
        return v


class BoundaryWavelets1D(BoundaryWavelets2D):
    """BoundaryWavelets1D(x, wname, levels, mode="symmetric", dtype=None): the batched 1-D DWT with the same boundary modes.  ``x`` is a
    2-D ``(Nr, Nc)`` numpy array or contiguous device tensor of ``Nr`` independent rows (a 1-D array is one row); the transform runs
    along the last axis only.  Bands ``[A_L, D_1, ..., D_L]`` (level 1 the finest), band ``l`` of shape ``(Nr, N_l)`` with
    ``N_l = (N_{l-1} + hlen - 1) // 2``: the bands of ``pywt.wavedec(x, wname, mode, levels, axis=-1)`` in the order of
    ``Wavelets(ndim=1)``.  Levels are clamped to ilog2(Nc / (hlen - 1)).  Same surface and state machine as ``BoundaryWavelets2D``;
    the finest detail band of the statistics is band 1 (all rows together) and N of the universal threshold is Nc."""

    _hpfx = "pdwt_bw1_"

    @staticmethod
    def _shape2(shape):
        if len(shape) == 1:
            return (1, shape[0])
        if len(shape) != 2:
            raise ValueError("BoundaryWavelets1D needs a batch of rows (Nr, Nc) or one row (Nc,)")
        return shape

    @property
    def fused(self):
        """True when ``forward()`` and ``inverse()`` of this instance are one kernel launch each (the rows fit the LDS of a workgroup);
        False: one launch per level."""
        return bool(self._bs("fused")(self._h))


class BoundaryWavelets3D(BoundaryWavelets2D):
    """BoundaryWavelets3D(vol, wname, levels, mode="symmetric", dtype=None): the 3-D DWT of a volume with the same boundary modes.
    ``vol`` is a 3-D ``(Nz, Nr, Nc)`` numpy array or a contiguous float32 / float64 device tensor.  One level runs along x (the last
    axis), then y, then z and gives eight bands of ``(n + hlen - 1) // 2`` per axis: the bands of ``pywt.wavedecn(vol, wname, mode,
    levels)`` in the order of ``Wavelets3D``, ``[A_L, the 7 details of level L, ..., those of level 1]``, the details of a level in
    ``BAND_KEYS`` order (first letter = z axis).  Levels are clamped to ilog2(min(Nz, Nr, Nc) / (hlen - 1)) and to 13; Nz <= 65535 and
    Nr * Nc < 2^31.  Same surface and state machine as ``BoundaryWavelets2D``; the finest diagonal band of the statistics is ``ddd`` of
    level 1 and N of the universal threshold is Nz * Nr * Nc."""

    _hpfx = "pdwt_bw3_"
    _info_t = N.InfoBW3

    @staticmethod
    def _shape2(shape):
        if len(shape) != 3:
            raise ValueError("BoundaryWavelets3D needs a 3-D volume (Nz, Nr, Nc)")
        return shape

    def coeff_shape(self, num):
        z, r, c = C.c_int(), C.c_int(), C.c_int()
        if self._bs("coeff_shape")(self._h, int(num), C.byref(z), C.byref(r), C.byref(c)) <= 0:
            raise IndexError(num)
        return z.value, r.value, c.value

    band_shape = coeff_shape

    def band_index(self, level, key):
        """Index of detail band ``key`` (e.g. "dad") of ``level`` (1 = finest)."""
        L = self.levels
        if not 1 <= level <= L:
            raise IndexError(level)
        return 1 + 7 * (L - level) + BAND_KEYS.index(key)

    def get_image(self):
        out = np.empty(self.shape, dtype=self.dtype)
        if self._bs("get_image")(self._h, out.ctypes.data_as(C.c_void_p)) != min(out.size, 2**31 - 1):
            raise RuntimeError("get_image failed (state=%d)" % self.state)
        return out

    def get_coeff(self, num):
        self._need_coeffs("get_coeff")
        out = np.empty(self.coeff_shape(num), dtype=self.dtype)
        if self._bs("get_coeff")(self._h, out.ctypes.data_as(C.c_void_p), int(num)) != min(out.size, 2**31 - 1):
            raise RuntimeError("get_coeff(%d) failed (state=%d)" % (num, self.state))
        return out


class BoundaryImageBatch(BoundaryWavelets2D):
    """BoundaryImageBatch(imgs, wname, levels, mode="symmetric", dtype=None): the 2-D DWT with boundary modes of ``B`` equally sized
    images.  ``imgs`` is a 3-D ``(B, Nr, Nc)`` numpy array or a contiguous float32 / float64 device tensor; every image is transformed as
    ``BoundaryWavelets2D`` transforms it (the same bits), bands ``[A_L, H1, V1, D1, ..., H_L, V_L, D_L]``; band ``num`` of the batch is
    one ``(B, nr_l, nc_l)`` stack, which is what ``get_coeff`` / ``set_coeff`` / ``coeff_view`` move.  1 <= B <= 65535.  When the pyramid
    of one image fits the LDS of a workgroup (``fused``) ``forward()`` and ``inverse()`` are one kernel launch each, whatever ``levels``
    and ``B``.  Same state machine as ``BoundaryWavelets2D``.

    Statistics.  ``all_band_stats``, ``estimate_sigma``, ``threshold_bands``, ``denoise`` and ``norm1`` carry the names, signatures and
    PER-IMAGE meaning of ``ImageBatch`` (arrays ``(B, nbands)`` / ``(B,)``, every image its own sigma).  The pooled ones of the base
    class, in which a band is the whole stack (the finest diagonal band = the D1 stack of all images, N of the universal threshold =
    Nr * Nc), are ``band_stats`` and ``pooled_all_band_stats`` / ``pooled_estimate_sigma`` / ``pooled_threshold_bands`` /
    ``pooled_denoise`` / ``pooled_norm1``; ``soft_threshold`` / ``hard_threshold`` apply one beta to every image."""

    _hpfx = "pdwt_bwb_"
    _info_t = N.InfoBWB

    @staticmethod
    def _shape2(shape):
        if len(shape) != 3:
            raise ValueError("BoundaryImageBatch needs a batch of images (B, Nr, Nc)")
        return shape

    def __len__(self):
        return self.shape[0]

    def coeff_shape(self, num):
        b, r, c = C.c_int(), C.c_int(), C.c_int()
        if self._bs("coeff_shape")(self._h, int(num), C.byref(b), C.byref(r), C.byref(c)) <= 0:
            raise IndexError(num)
        return b.value, r.value, c.value

    band_shape = coeff_shape

    @property
    def fused(self):
        """True when ``forward()`` and ``inverse()`` of this instance are one kernel launch each (one workgroup per image, all levels
        in LDS); False: one launch per level over the stacks."""
        return bool(self._bs("fused")(self._h))

    get_images = BoundaryWavelets2D.get_image

    # -- the pooled statistics of the base class under their own names -------------------------
    pooled_all_band_stats = BoundaryWavelets2D.all_band_stats
    pooled_estimate_sigma = BoundaryWavelets2D.estimate_sigma
    pooled_threshold_bands = BoundaryWavelets2D.threshold_bands
    pooled_denoise = BoundaryWavelets2D.denoise
    pooled_norm1 = BoundaryWavelets2D.norm1

    # -- per image: the methods of ImageBatch ----------------------------------------------------
    def _refused(self, what, rc=-1):
        if rc != -1:  # (PDWT_EINVAL is the refusal; anything else is a device error: allocation, copy or launch)
            return RuntimeError("%s failed on the device (code %d): %s" % (what, rc, (N.hip().pdwt_last_error_string() or b"").decode()))
        return RuntimeError("%s refused (state=%d): the coefficients are not valid" % (what, self.state))

    def all_band_stats(self, with_median=False):
        """{n, sum_abs, sum_sq, max_abs, median_abs}: float64 arrays of shape (B, nbands), entry [b, k] = the statistics of band k of
        image b (``median_abs`` NaN unless ``with_median``)."""
        B, nb = self.shape[0], self.nbands
        out = (N.BandStats * (B * max(nb, 1)))()
        rc = self._bs("images_all_band_stats")(self._h, out, int(bool(with_median)))
        if rc != 0:
            raise self._refused("all_band_stats", rc)
        a = np.frombuffer(out, dtype=np.float64).reshape(B, max(nb, 1), len(N.BandStats._fields_))[:, :nb]
        return {k: a[:, :, i].copy() for i, (k, _) in enumerate(N.BandStats._fields_)}

    def estimate_sigma(self):
        """(B,) float64: every image's OWN noise level, median |its D1| / 0.6744897501960817."""
        s = np.zeros(self.shape[0], dtype=np.float64)
        rc = self._bs("images_estimate_sigma")(self._h, s.ctypes.data_as(C.POINTER(C.c_double)))
        if rc != 0:
            raise self._refused("estimate_sigma", rc)
        return s

    def threshold_bands(self, betas, kind="soft"):
        """``betas``: (B, nbands), or (nbands,) for every image; a negative beta leaves that band of that image alone."""
        if kind not in self.KINDS:
            raise ValueError("kind must be 'soft' or 'hard'")
        B, nb = self.shape[0], self.nbands
        b = np.asarray(betas, dtype=self.dtype)
        if b.shape == (nb,):
            b = np.broadcast_to(b, (B, nb))
        if b.shape != (B, nb):
            raise ValueError("betas of shape %s for %d images of %d bands" % (b.shape, B, nb))
        b = np.ascontiguousarray(b)
        rc = self._bs("images_threshold_bands")(self._h, b.ctypes.data_as(C.c_void_p), self.KINDS[kind])
        if rc != 0:
            raise self._refused("threshold_bands", rc)

    def denoise(self, method="bayes", sigma=None, kind="soft"):
        """``BoundaryWavelets2D.denoise`` of every image, each with its own sigma: ``sigma`` None (estimated per image), a scalar or a
        (B,) array.  Returns {"sigma": (B,) float64, "betas": (B, nbands) in the batch's dtype, betas[:, 0] == -1}."""
        if method not in self.METHODS:
            raise ValueError("method must be 'visu' or 'bayes'")
        if kind not in self.KINDS:
            raise ValueError("kind must be 'soft' or 'hard'")
        B, nb = self.shape[0], self.nbands
        sin = None
        if sigma is not None:
            sin = np.asarray(sigma, dtype=np.float64)
            if sin.shape not in ((), (B,)):
                raise ValueError("sigma must be None, a scalar or %d values" % B)
            sin = np.ascontiguousarray(np.broadcast_to(sin, (B,)))
            if not np.all(sin >= 0):
                raise ValueError("sigma must be >= 0 (None: estimated)")
        sout = np.zeros(B, dtype=np.float64)
        betas = np.zeros((B, max(nb, 1)), dtype=self.dtype)
        dp = C.POINTER(C.c_double)
        rc = self._bs("images_denoise")(self._h, self.METHODS[method], sin.ctypes.data_as(dp) if sin is not None else None, self.KINDS[kind],
                                        sout.ctypes.data_as(dp), betas.ctypes.data_as(C.c_void_p))
        if rc != 0:
            raise self._refused("denoise", rc)
        return {"sigma": sout, "betas": betas[:, :nb]}

    def norm1(self):
        """(B,) float64: sum |c| over the bands of each image, accumulated in double (``pooled_norm1``: the sum over the batch)."""
        out = np.zeros(self.shape[0], dtype=np.float64)
        rc = self._bs("images_norm1")(self._h, out.ctypes.data_as(C.POINTER(C.c_double)))
        if rc != 0:
            raise self._refused("norm1", rc)
        return out
