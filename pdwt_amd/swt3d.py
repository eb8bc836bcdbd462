"""Python view of the C++ ``StationaryWavelets3D`` class (include/swt3d.h): the separable, stationary (undecimated, a-trous) 3-D
transform of a volume.

Level j is the 1-D a-trous level of ``Wavelets(..., do_swt=1, ndim=1)`` at tap spacing 2^(j-1) along x, then y, then z.  The
bands are indexed as in ``Wavelets3D`` (``coeffs[0]`` = A_L, then for levels L .. 1 the 7 details in ``BAND_KEYS`` order), but
every band is full size (Nz, Nr, Nc), and ``inverse()`` leaves them intact.
"""
from .wavelets3d import BAND_KEYS, Wavelets3D  # noqa: F401  (BAND_KEYS: the same band order)


class StationaryWavelets3D(Wavelets3D):
    """StationaryWavelets3D(vol, wname, levels): ``vol`` is a 3-D numpy array (Nz, Nr, Nc) or a contiguous float32 / float64
    torch tensor on the GPU (copied device to device into the instance).  Same methods and state machine as ``Wavelets3D``.
    Not available: non-separable and custom banks, cycle spinning, group_soft_threshold, shrink, proj_linf (ValueError)."""

    _hpfx = "pdwt_swt3d_"
    _cname = "StationaryWavelets3D"

    def __init__(self, vol, wname, levels, dtype=None, do_separable=1, do_cycle_spinning=0):
        if not do_separable or do_cycle_spinning:
            raise ValueError("StationaryWavelets3D: only the separable transform is available "
                             "(no non-separable transform or cycle spinning)")
        self._open(vol, wname, levels, dtype)

    def _refuse(self, name):
        raise ValueError("StationaryWavelets3D: %s is not available" % name)
