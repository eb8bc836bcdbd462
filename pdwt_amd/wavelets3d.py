"""Python view of the C++ ``Wavelets3D`` class (include/wt3d.h): the separable, decimated, periodised 3-D DWT of a volume.

One level is the 1-D level of ``Wavelets(..., ndim=1)`` along x, then y, then z.  Bands: ``coeffs[0]`` = A_L, then for
levels L .. 1 the 7 detail bands of the level in PyWavelets' ``dwtn`` key order (``BAND_KEYS``; first letter = z axis).
"""
import ctypes as C

import numpy as np

from . import _native as N
from .wavelets import DeviceArray, _BandStatsAPI, _device_source, _sync_producer

# detail bands of one level, in storage order (band 1 + 7*(L - lev) + k is BAND_KEYS[k] of level lev, 1 = finest)
BAND_KEYS = ("aad", "ada", "add", "daa", "dad", "dda", "ddd")


class Wavelets3D(_BandStatsAPI):
    """Wavelets3D(vol, wname, levels): ``vol`` is a 3-D numpy array (Nz, Nr, Nc) or a contiguous float32 / float64 torch
    tensor on the GPU (copied device to device into the instance, as Wavelets does: no host round trip).  Same state machine as ``Wavelets``.
    Not in 3-D: SWT, non-separable and custom banks, cycle spinning, group_soft_threshold, shrink, proj_linf (ValueError)."""

    _hpfx = "pdwt_wavelets3d_"  # the handle API (wt3d.cpp) and the name in messages: StationaryWavelets3D sets its own
    _cname = "Wavelets3D"

    def __init__(self, vol, wname, levels, dtype=None, do_swt=0, do_separable=1, do_cycle_spinning=0):
        if do_swt or not do_separable or do_cycle_spinning:
            raise ValueError("Wavelets3D: only the decimated separable transform is available in 3-D "
                             "(no SWT, non-separable transform or cycle spinning)")
        self._open(vol, wname, levels, dtype)

    def _open(self, vol, wname, levels, dtype):
        """Create the C++ instance from a numpy volume or a device tensor (what both volume classes do after checking their arguments)."""
        N.require_gpu()
        dev = _device_source(vol)
        if dev is not None:
            ptr, shape, dt = dev
            if dtype is not None and np.dtype(dtype) != dt:
                raise TypeError("dtype does not match the device tensor")
            _sync_producer()
            src, on_host, self._keep = C.c_void_p(ptr), 0, None
        else:
            vol = np.asarray(vol)
            dt = np.dtype(dtype or (vol.dtype if vol.dtype in (np.float32, np.float64) else np.float32))
            self._keep = np.ascontiguousarray(vol, dtype=dt)
            shape, src, on_host = self._keep.shape, self._keep.ctypes.data_as(C.c_void_p), 1
        if len(shape) != 3:
            raise ValueError("%s needs a 3-D volume (Nz, Nr, Nc)" % self._cname)
        self.dtype, self.shape, self.wname = np.dtype(dt), tuple(int(v) for v in shape), wname
        self._L = N.host(self.dtype)
        self._ct = C.c_float if self.dtype == np.float32 else C.c_double
        self._h = self._fn("new")(src, self.shape[0], self.shape[1], self.shape[2], wname.encode(), int(levels), on_host)
        self._keep = None
        if not self._h:
            raise MemoryError("%s allocation failed" % self._cname)

    _fn = _BandStatsAPI._bs  # handle function ``name`` of this class: getattr(self._L, self._hpfx + name)

    def close(self):
        if getattr(self, "_h", None):
            self._fn("delete")(self._h)
        self._h = None

    __del__ = close

    # -- introspection ---------------------------------------------------------------------
    @property
    def info(self):
        i = N.Info3D()
        self._fn("info")(self._h, C.byref(i))
        return i

    @property
    def levels(self):
        return self.info.nlevels

    @property
    def state(self):
        return self._fn("state")(self._h)

    @property
    def nbands(self):
        return self._fn("num_bands")(self._h)

    def band_shape(self, num):
        z, r, c = C.c_int(), C.c_int(), C.c_int()
        if self._fn("band_shape")(self._h, int(num), C.byref(z), C.byref(r), C.byref(c)) <= 0:
            raise IndexError(num)
        return z.value, r.value, c.value

    def band_index(self, level, key):
        """Index of detail band ``key`` (e.g. "dad") of ``level`` (1 = finest)."""
        L = self.levels
        if not 1 <= level <= L:
            raise IndexError(level)
        return 1 + 7 * (L - level) + BAND_KEYS.index(key)

    # -- transforms and coefficient utilities -----------------------------------------------
    def forward(self):
        self._fn("forward")(self._h)

    def inverse(self):
        self._fn("inverse")(self._h)

    def soft_threshold(self, beta, do_thresh_appcoeffs=0, normalize=0):
        self._fn("soft_threshold")(self._h, self._ct(beta), int(do_thresh_appcoeffs), int(normalize))

    def hard_threshold(self, beta, do_thresh_appcoeffs=0, normalize=0):
        self._fn("hard_threshold")(self._h, self._ct(beta), int(do_thresh_appcoeffs), int(normalize))

    def norm1(self):
        return self.dtype.type(self._fn("norm1")(self._h))

    def norm1_f64(self):
        """Sum of |c| over all bands, in double."""
        return float(self._fn("norm1_f64")(self._h))

    def _refuse(self, name):
        raise ValueError("Wavelets3D: %s is not available in 3-D" % name)

    def group_soft_threshold(self, *a, **k):
        self._refuse("group_soft_threshold")

    def shrink(self, *a, **k):
        self._refuse("shrink")

    def proj_linf(self, *a, **k):
        self._refuse("proj_linf")

    def set_filters_forward(self, *a, **k):
        self._refuse("a custom filter bank")

    set_filters_inverse = set_filters_forward

    # -- data in and out ---------------------------------------------------------------------
    def get_image(self):
        out = np.empty(self.shape, dtype=self.dtype)
        n = self._fn("get_image")(self._h, out.ctypes.data_as(C.c_void_p))
        if n != min(out.size, 2**31 - 1):
            raise RuntimeError("get_image failed")
        return out

    def set_image(self, vol, mem_is_on_device=0):
        n = self.shape[0] * self.shape[1] * self.shape[2]
        dev = _device_source(vol)
        if dev is not None:
            if dev[2] != self.dtype or int(np.prod(dev[1])) != n:
                raise ValueError("device volume of the wrong dtype or size")
            vol, mem_is_on_device = dev[0], 1
        if mem_is_on_device:
            _sync_producer()
            self._fn("set_image")(self._h, C.c_void_p(int(vol)), 1)
        else:
            a = np.ascontiguousarray(vol, dtype=self.dtype)
            if a.size != n:
                raise ValueError("volume of the wrong size")
            self._fn("set_image")(self._h, a.ctypes.data_as(C.c_void_p), 0)

    def get_coeff(self, num):
        out = np.empty(self.band_shape(num), dtype=self.dtype)
        n = self._fn("get_coeff")(self._h, out.ctypes.data_as(C.c_void_p), int(num))
        if n != min(out.size, 2**31 - 1):
            raise RuntimeError("get_coeff(%d) failed (state=%d)" % (num, self.state))
        return out

    def set_coeff(self, arr, num):
        shape = self.band_shape(num)
        n = shape[0] * shape[1] * shape[2]
        dev = _device_source(arr)
        if dev is not None:
            if dev[2] != self.dtype or int(np.prod(dev[1])) != n:
                raise ValueError("device band of the wrong dtype or size")
            _sync_producer()
            self._fn("set_coeff")(self._h, C.c_void_p(dev[0]), int(num), 1)
            return
        a = np.ascontiguousarray(arr, dtype=self.dtype)
        if a.size != n:
            raise ValueError("band of the wrong size")
        self._fn("set_coeff")(self._h, a.ctypes.data_as(C.c_void_p), int(num), 0)

    @property
    def coeffs(self):
        return [self.get_coeff(i) for i in range(self.nbands)]

    def sync(self):
        return N.hip().pdwt_sync()

    def image_int_ptr(self):
        return self._fn("image_int_ptr")(self._h)

    def coeff_int_ptr(self, num):
        return self._fn("coeff_int_ptr")(self._h, int(num))

    def image_view(self):
        """The volume as a zero-copy DeviceArray (call ``sync()`` before a consumer on another stream reads it)."""
        return DeviceArray(self, self.image_int_ptr(), self.shape, self.dtype)

    def coeff_view(self, num):
        """Band ``num`` as a zero-copy DeviceArray."""
        return DeviceArray(self, self.coeff_int_ptr(num), self.band_shape(num), self.dtype)
