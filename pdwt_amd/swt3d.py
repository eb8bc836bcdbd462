"""Python view of the C++ ``StationaryWavelets3D`` class (include/swt3d.h): the separable, stationary (undecimated, a-trous) 3-D
transform of a volume.

Level j is the 1-D a-trous level of ``Wavelets(..., do_swt=1, ndim=1)`` at tap spacing 2^(j-1) along x, then y, then z.  The
bands are indexed as in ``Wavelets3D`` (``coeffs[0]`` = A_L, then for levels L .. 1 the 7 details in ``BAND_KEYS`` order), but
every band is full size (Nz, Nr, Nc), and ``inverse()`` leaves them intact.
"""
import ctypes as C

import numpy as np

from . import _native as N
from .wavelets import _device_source, _sync_producer
from .wavelets3d import BAND_KEYS, Wavelets3D  # noqa: F401  (BAND_KEYS: the same band order)


class _SwtHandleAPI:
    """The pdwt_swt3d_* handle API (swt3d.cpp) under the pdwt_wavelets3d_* names the methods of Wavelets3D call: both C++
    classes export the same handle functions, so every method of the Python class is shared."""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        if name.startswith("pdwt_wavelets3d_"):
            name = "pdwt_swt3d_" + name[len("pdwt_wavelets3d_"):]
        return getattr(self._lib, name)


class StationaryWavelets3D(Wavelets3D):
    """StationaryWavelets3D(vol, wname, levels): ``vol`` is a 3-D numpy array (Nz, Nr, Nc) or a contiguous float32 / float64
    torch tensor on the GPU (copied device to device into the instance).  Same methods and state machine as ``Wavelets3D``.
    Not available: non-separable and custom banks, cycle spinning, group_soft_threshold, shrink, proj_linf (ValueError)."""

    def __init__(self, vol, wname, levels, dtype=None, do_separable=1, do_cycle_spinning=0):
        if not do_separable or do_cycle_spinning:
            raise ValueError("StationaryWavelets3D: only the separable transform is available "
                             "(no non-separable transform or cycle spinning)")
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
            raise ValueError("StationaryWavelets3D needs a 3-D volume (Nz, Nr, Nc)")
        self.dtype, self.shape, self.wname = np.dtype(dt), tuple(int(v) for v in shape), wname
        self._L = _SwtHandleAPI(N.host(self.dtype))
        self._ct = C.c_float if self.dtype == np.float32 else C.c_double
        self._h = self._L.pdwt_swt3d_new(src, self.shape[0], self.shape[1], self.shape[2], wname.encode(), int(levels), on_host)
        self._keep = None
        if not self._h:
            raise MemoryError("StationaryWavelets3D allocation failed")

    def _refuse(self, name):
        raise ValueError("StationaryWavelets3D: %s is not available" % name)
