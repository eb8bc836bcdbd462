"""pdwt_amd -- MI355X-native (gfx950) implementation of PDWT's separable DWT hot path.

The product is native: hand-written HIP kernels behind a C-ABI (include/pdwt_hip.h,
pdwt_amd/lib/libpdwt_hip.so) and the reference's own C++ ``Wavelets`` class above it
(include/wt.h, libpdwt.so / libpdwtd.so).  This Python package is a thin ctypes view of those
libraries for tests, bench.py and Python callers -- the shape of the reference's external pypwt
binding (README.md:24).
"""
from ._native import Info, Info3D, hip, host, require_gpu  # noqa: F401
from .wavelets import DeviceArray, ImageBatch, Wavelets, W_CREATION_ERROR, W_FORWARD, W_INIT, W_INVERSE  # noqa: F401
from .wavelets3d import Wavelets3D  # noqa: F401
from .swt3d import StationaryWavelets3D  # noqa: F401
from .wpt import WaveletPacketBatch, WaveletPackets1D, WaveletPackets2D  # noqa: F401
from .boundary import BoundaryImageBatch, BoundaryWavelets1D, BoundaryWavelets2D, BoundaryWavelets3D  # noqa: F401
from . import functional  # noqa: F401
from .functional import dwt1, dwt1_adjoint, dwt2, dwt2_adjoint, dwt3, dwt3_adjoint, idwt1, idwt1_adjoint, idwt2, idwt2_adjoint, idwt3, idwt3_adjoint  # noqa: F401

__all__ = ["Wavelets", "Wavelets3D", "StationaryWavelets3D", "WaveletPackets2D", "WaveletPackets1D", "WaveletPacketBatch", "BoundaryWavelets2D", "BoundaryWavelets1D", "BoundaryWavelets3D", "BoundaryImageBatch", "ImageBatch", "DeviceArray", "functional", "dwt2", "idwt2", "dwt1", "idwt1", "dwt2_adjoint", "idwt2_adjoint", "dwt1_adjoint", "idwt1_adjoint", "dwt3", "idwt3", "dwt3_adjoint", "idwt3_adjoint", "Info", "hip", "host", "require_gpu"]
