#!/usr/bin/env python3
"""Forward + inverse pairs of the batched 2-D DWT with boundary modes (pdwt_amd.BoundaryImageBatch, dwt_ext2db.hip) on the MI355X.

Shapes: 256 x 64^2, 64 x 128^2 and 64 x 512^2 float32 db4 L3 `symmetric`, and 64 x 128^2 float64 db4 L3.  Per shape, in the same run:
  class    the new class (one launch per direction where the pyramid of an image fits LDS, else one per level)
  levels   the per-level form through the level drivers of the C ABI chained by hand (one launch per level and direction)
  loop     a loop over B BoundaryWavelets2D instances: the baseline the class replaces (2 L B launches per pair)
  periodic the periodised ImageBatch of the same shape, for context
Method of tools/bench_ext.py: HIP events on the library stream, --warmup pairs, then the median us per pair over --reps timed batches of
--steps pairs, the fastest batch beside it.  GB/s on COMPULSORY bytes: one read of the batch and one write of every band (forward),
the reverse (inverse).  No speed is asserted anywhere: this tool only measures.
usage: python tools/bench_ext2db.py [--steps 10] [--warmup 3] [--reps 5]     (prints one JSON line per shape)"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pdwt_amd  # noqa: E402
from pdwt_amd import _native as nat  # noqa: E402

SHAPES = [((256, 64, 64), np.float32), ((64, 128, 128), np.float32), ((64, 512, 512), np.float32), ((64, 128, 128), np.float64)]
WNAME, LEVELS, MODE = "db4", 3, "symmetric"


def time_pairs(H, ev, pair, sync, a):
    for _ in range(a.warmup):
        pair()
    sync()
    us = []
    for _ in range(a.reps):
        H.pdwt_event_record(ev[0])
        for _ in range(a.steps):
            pair()
        H.pdwt_event_record(ev[1])
        H.pdwt_event_sync(ev[1])
        us.append(1e3 * H.pdwt_event_elapsed_ms(ev[0], ev[1]) / a.steps)
    return round(float(np.median(us)), 1), round(float(min(us)), 1)


def level_pair(H, W, dt):
    """forward + inverse of all levels through pdwt_ext2db_*_level_* on the buffers of W (its bands, its image) and two scratch stacks"""
    sfx = "f32" if np.dtype(dt) == np.float32 else "f64"
    f = (nat.Filters32 if sfx == "f32" else nat.Filters64)()
    f.hlen = getattr(H, "pdwt_compute_filters_separable_" + sfx)(WNAME.encode(), 0, C.byref(f))
    B, Nr, Nc = W.shape
    L = W.levels
    shp = [(Nr, Nc)] + [W.coeff_shape(3 * l)[1:] for l in range(1, L + 1)]
    stack1 = B * shp[1][0] * shp[1][1] * np.dtype(dt).itemsize
    tmp = [H.pdwt_malloc(stack1), H.pdwt_malloc(stack1)]
    assert all(tmp)
    band = [W.coeff_int_ptr(k) for k in range(W.nbands)]
    img = W.image_int_ptr()
    fwd, inv = getattr(H, "pdwt_ext2db_forward_level_" + sfx), getattr(H, "pdwt_ext2db_inverse_level_" + sfx)
    approx = lambda l: band[0] if l == L else tmp[(l - 1) & 1]  # noqa: E731

    def pair():
        src = img
        for l in range(1, L + 1):
            d = band[3 * (l - 1) + 1:3 * l + 1]
            assert fwd(src, approx(l), d[0], d[1], d[2], B, shp[l - 1][0], shp[l - 1][1], 2, C.byref(f)) == 0
            src = approx(l)
        for l in range(L, 0, -1):
            d = band[3 * (l - 1) + 1:3 * l + 1]
            assert inv(img if l == 1 else approx(l - 1), approx(l), d[0], d[1], d[2], B, shp[l - 1][0], shp[l - 1][1], C.byref(f)) == 0

    return pair, tmp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    pdwt_amd.require_gpu()
    H = pdwt_amd.hip()
    H.pdwt_set_device(0)
    ev = (H.pdwt_event_create(), H.pdwt_event_create())
    for shape, dt in SHAPES:
        x = np.random.RandomState(0).standard_normal(shape).astype(dt)
        W = pdwt_amd.BoundaryImageBatch(x, WNAME, LEVELS, MODE)
        assert W.levels == LEVELS

        def pair_class():
            W.forward()
            W.inverse()

        cls = time_pairs(H, ev, pair_class, W.sync, a)
        err = float(np.abs(W.get_image().astype(np.float64) - x).max())
        item = np.dtype(dt).itemsize
        nb = 2 * item * (x.size + sum(int(np.prod(W.coeff_shape(k))) for k in range(W.nbands)))  # both directions
        pair_lv, tmp = level_pair(H, W, dt)
        lev = time_pairs(H, ev, pair_lv, W.sync, a)
        err_lv = float(np.abs(W.get_image().astype(np.float64) - x).max())
        W.sync()
        for p in tmp:
            H.pdwt_free(p)
        fused = W.fused
        W.close()
        singles = [pdwt_amd.BoundaryWavelets2D(x[b], WNAME, LEVELS, MODE) for b in range(shape[0])]

        def pair_loop():
            for S in singles:
                S.forward()
                S.inverse()

        loop = time_pairs(H, ev, pair_loop, singles[0].sync, a)
        for S in singles:
            S.close()
        P = pdwt_amd.ImageBatch(x, WNAME, LEVELS)

        def pair_periodic():
            P.forward()
            P.inverse()

        per = time_pairs(H, ev, pair_periodic, P.sync, a)
        P.close()
        print(json.dumps({"shape": "x".join(map(str, shape)), "dtype": np.dtype(dt).name, "wavelet": WNAME, "levels": LEVELS, "mode": MODE, "fused": fused,
                          "launches_per_pair": {"class": 2 if fused else 2 * LEVELS, "levels": 2 * LEVELS, "loop": 2 * LEVELS * shape[0]},
                          "us_per_pair": {"class": cls[0], "levels": lev[0], "loop": loop[0], "periodic_ImageBatch": per[0]},
                          "us_min": {"class": cls[1], "levels": lev[1], "loop": loop[1], "periodic_ImageBatch": per[1]},
                          "compulsory_MB": round(nb / 1e6, 2), "GBps_compulsory": {"class": round(nb / cls[0] / 1e3, 1), "levels": round(nb / lev[0] / 1e3, 1)},
                          "class_over_levels": round(cls[0] / lev[0], 2), "loop_over_class": round(loop[0] / cls[0], 1),
                          "roundtrip_maxerr": {"class": err, "levels": err_lv}}), flush=True)
    H.pdwt_event_destroy(ev[0])
    H.pdwt_event_destroy(ev[1])


if __name__ == "__main__":
    main()
