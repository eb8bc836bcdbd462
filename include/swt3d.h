/*
 * swt3d.h -- `StationaryWavelets3D`: the separable, stationary (undecimated, a-trous) 3-D transform of a volume -- the
 * reference's do_swt with a third axis.  Same build as wt3d.h: plain host C++, DTYPE = float (libpdwt.so) or double
 * (-DDOUBLEPRECISION, libpdwtd.so), every device action a C-ABI call into libpdwt_hip.so (include/pdwt_hip.h).
 *
 * Volume: row-major Nz x Nr x Nc.  Level j = the 1-D a-trous level of Wavelets(..., do_swt=1, ndim=1) at tap spacing 2^(j-1)
 * along x, then y, then z; its input is the aaa band of level j-1.  No decimation: any size, odd sizes included.
 * Levels are clamped to ilog2(min(Nz, Nr, Nc) / (hlen - 1)); a clamp to 0 levels is W_CREATION_ERROR.
 * Sizes: Nz <= 65535 and Nr * Nc < 2^31 (the volume itself may be larger); otherwise W_CREATION_ERROR.
 * Device memory of an instance: the volume, 7L+1 full-size bands and a 4-volume scratch: (7L + 6) x the volume.
 * Bands: the indexing of Wavelets3D -- 0 = A_L, then for levels L .. 1 the details aad, ada, add, daa, dad, dda, ddd (first
 * letter = z axis) -- every band Nz x Nr x Nc.  inverse() leaves every band intact.
 * State machine: the one of Wavelets / Wavelets3D.  Not available: non-separable and custom banks, cycle spinning,
 * group_soft_threshold, shrink, proj_linf.
 */
#ifndef SWT3D_H
#define SWT3D_H

#include "wt3d.h"

class StationaryWavelets3D : public Transform3D {
  public:
    StationaryWavelets3D(DTYPE* vol, int Nz, int Nr, int Nc, const char* wname, int levels, int memisonhost = 1);
};

#endif
