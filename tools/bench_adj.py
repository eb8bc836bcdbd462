#!/usr/bin/env python3
"""The adjoint drivers of the boundary-mode transforms (dwt_ext_adj.hip) next to the forward and inverse drivers of the same shape, on
the MI355X, straight through the C ABI on device buffers.

Shapes: 64 x 128^2 and 64 x 512^2 float32, 64 x 128^2 float64 (2-D, db4 L3 `symmetric`) and 4096 rows of 4096 samples float32 (1-D).
Per shape: us per call of forward, inverse, forward_adjoint (W^T: synthesis onto the extended grid + fold) and inverse_adjoint (S^T: the
forward driver in mode zero with the reversed bank).  The 2-D inverse may run its fused whole-pyramid form where an image fits LDS;
the 2-D forward adjoint always runs per level (two launches per level), so the two columns are not the same number of launches.
Method of tools/bench_ext2db.py: HIP events on the library stream, --warmup calls, then the median us per call over --reps timed batches
of --steps calls, the fastest batch beside it.  No speed is asserted anywhere: this tool only measures.
usage: python tools/bench_adj.py [--steps 10] [--warmup 3] [--reps 5]     (prints one JSON line per shape)"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pdwt_amd  # noqa: E402
from pdwt_amd import _native as nat  # noqa: E402

SHAPES = [((64, 128, 128), np.float32), ((64, 512, 512), np.float32), ((64, 128, 128), np.float64), ((4096, 4096), np.float32)]
WNAME, LEVELS, MODE = "db4", 3, 2  # symmetric


def time_calls(H, ev, call, a):
    for _ in range(a.warmup):
        assert call() >= 0
    H.pdwt_sync()
    us = []
    for _ in range(a.reps):
        H.pdwt_event_record(ev[0])
        for _ in range(a.steps):
            call()
        H.pdwt_event_record(ev[1])
        H.pdwt_event_sync(ev[1])
        us.append(1e3 * H.pdwt_event_elapsed_ms(ev[0], ev[1]) / a.steps)
    return round(float(np.median(us)), 1), round(float(min(us)), 1)


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
        item = np.dtype(dt).itemsize
        sfx = "f32" if item == 4 else "f64"
        f = (nat.Filters32 if sfx == "f32" else nat.Filters64)()
        f.hlen = getattr(H, "pdwt_compute_filters_separable_" + sfx)(WNAME.encode(), 0, C.byref(f))
        fp = C.byref(f)
        two_d = len(shape) == 3
        fam = "ext2db" if two_d else "ext1d"
        g = lambda name: getattr(H, "pdwt_%s_%s_%s" % (fam, name, sfx))  # noqa: E731
        if two_d:
            geo = (shape[0], shape[1], shape[2])
            nb = 3 * LEVELS + 1
            sizes = [shape[0] * H.pdwt_ext_band_shape(shape[1], shape[2], f.hlen, LEVELS, k, None, None) for k in range(nb)]
            tmp_n = max(H.pdwt_ext2db_tmp_elems(*geo, f.hlen, LEVELS, item), H.pdwt_ext2db_adjoint_tmp_elems(*geo, f.hlen, LEVELS, item))
            fused = H.pdwt_ext2db_fused(shape[1], shape[2], f.hlen, LEVELS, item)
        else:
            geo = (shape[0], shape[1])
            nb = LEVELS + 1
            sizes = [shape[0] * H.pdwt_ext1d_band_len(shape[1], f.hlen, LEVELS, k) for k in range(nb)]
            tmp_n = max(H.pdwt_ext1d_tmp_elems(*geo, f.hlen, LEVELS, item), H.pdwt_ext1d_adjoint_tmp_elems(*geo, f.hlen, LEVELS, item))
            fused = H.pdwt_ext1d_fused(shape[1], f.hlen, LEVELS, item)
        x = np.random.RandomState(0).standard_normal(shape).astype(dt)
        img, out = H.pdwt_malloc(x.nbytes), H.pdwt_malloc(x.nbytes)
        bands = [H.pdwt_malloc(n * item) for n in sizes]
        tmp = H.pdwt_malloc(max(tmp_n, 1) * item)
        assert img and out and tmp and all(bands)
        assert H.pdwt_memcpy_h2d(img, x.ctypes.data, x.nbytes) == 0
        tab = (C.c_void_p * nb)(*bands)
        res = {}
        res["forward"] = time_calls(H, ev, lambda: g("forward")(img, tab, *geo, LEVELS, MODE, fp, tmp), a)
        res["inverse"] = time_calls(H, ev, lambda: g("inverse")(out, tab, *geo, LEVELS, fp, tmp), a)
        res["forward_adjoint"] = time_calls(H, ev, lambda: g("forward_adjoint")(out, tab, *geo, LEVELS, MODE, fp, tmp), a)
        res["inverse_adjoint"] = time_calls(H, ev, lambda: g("inverse_adjoint")(img, tab, *geo, LEVELS, fp, tmp), a)
        H.pdwt_sync()
        nbytes = item * (x.size + sum(sizes))  # one read of the bands and one write of the image, or the reverse
        print(json.dumps({"shape": "x".join(map(str, shape)), "dtype": np.dtype(dt).name, "wavelet": WNAME, "levels": LEVELS, "mode": "symmetric",
                          "forward_and_inverse_fused": fused, "us_per_call": {k: v[0] for k, v in res.items()}, "us_min": {k: v[1] for k, v in res.items()},
                          "compulsory_MB": round(nbytes / 1e6, 2), "GBps_compulsory": {k: round(nbytes / v[0] / 1e3, 1) for k, v in res.items()},
                          "forward_adjoint_over_inverse": round(res["forward_adjoint"][0] / res["inverse"][0], 2)}), flush=True)
        for p in [img, out, tmp] + bands:
            H.pdwt_free(p)
    H.pdwt_event_destroy(ev[0])
    H.pdwt_event_destroy(ev[1])


if __name__ == "__main__":
    main()
