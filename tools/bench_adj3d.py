#!/usr/bin/env python3
"""The adjoint level drivers of the 3-D boundary-mode transform (dwt_ext3d_adj.hip) next to the forward and inverse level drivers of the
same shape, on the MI355X, straight through the C ABI on device buffers.

Shapes: 256^3 float32 and 128^3 float64, one level, db4 `symmetric`.  Per shape: us per call of forward_level, inverse_level,
forward_adjoint_level (W^T: the z pass with its fold, then the 2-D level adjoint on the nz planes -- three launches) and
inverse_adjoint_level (S^T: the forward level in mode zero with the reversed bank).  The forward adjoint is to be read against the
inverse level of the same shape: the same bytes the other way round, two launches.  `xy_adjoint_alone` is the second half of the forward
adjoint by itself (pdwt_ext2db_forward_adjoint_level on the nz planes, from the quadrants in scratch), so the z pass is the difference
(its GB/s figure is on the level's compulsory bytes like the others, not on its own traffic).
Method of tools/bench_adj.py: HIP events on the library stream, --warmup calls, then the median us per call over --reps timed batches of
--steps calls, the fastest batch beside it.  No speed is asserted anywhere: this tool only measures.
usage: python tools/bench_adj3d.py [--steps 10] [--warmup 3] [--reps 5]     (prints one JSON line per shape)"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pdwt_amd  # noqa: E402
from pdwt_amd import _native as nat  # noqa: E402

SHAPES = [((256, 256, 256), np.float32), ((128, 128, 128), np.float64)]
WNAME, MODE = "db4", 2  # symmetric


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
        g = lambda name: getattr(H, "pdwt_ext3d_%s_%s" % (name, sfx))  # noqa: E731
        band = int(np.prod([(n + f.hlen - 1) // 2 for n in shape]))
        tmp_n = H.pdwt_ext3d_adjoint_level_tmp_elems(*shape, f.hlen)
        assert tmp_n > 0
        x = np.random.RandomState(0).standard_normal(shape).astype(dt)
        vol, out = H.pdwt_malloc(x.nbytes), H.pdwt_malloc(x.nbytes)
        bands = [H.pdwt_malloc(band * item) for _ in range(8)]
        tmp = H.pdwt_malloc(tmp_n * item)
        assert vol and out and tmp and all(bands)
        assert H.pdwt_memcpy_h2d(vol, x.ctypes.data, x.nbytes) == 0
        tab = (C.c_void_p * 8)(*bands)
        res = {}
        res["forward"] = time_calls(H, ev, lambda: g("forward_level")(vol, tab, *shape, MODE, fp, tmp), a)
        res["inverse"] = time_calls(H, ev, lambda: g("inverse_level")(out, tab, *shape, fp, tmp), a)
        res["forward_adjoint"] = time_calls(H, ev, lambda: g("forward_adjoint_level")(out, tab, *shape, MODE, fp, tmp), a)
        res["inverse_adjoint"] = time_calls(H, ev, lambda: g("inverse_adjoint_level")(vol, tab, *shape, fp, tmp), a)
        # the x-y half alone: the four quadrant cotangents the z pass left in scratch -> the volume, the frames behind them
        nz, nr, nc = shape
        sq = nz * ((nr + f.hlen - 1) // 2) * ((nc + f.hlen - 1) // 2)
        quads = [tmp + q * sq * item for q in range(4)]
        frame = tmp + (4 * sq + 63) // 64 * 64 * item
        xy = getattr(H, "pdwt_ext2db_forward_adjoint_level_" + sfx)
        res["xy_adjoint_alone"] = time_calls(H, ev, lambda: xy(out, *quads, nz, nr, nc, MODE, fp, frame), a)
        H.pdwt_sync()
        nbytes = item * (x.size + 8 * band)  # one read of the bands and one write of the volume, or the reverse (the quadrants in scratch not counted)
        print(json.dumps({"shape": "x".join(map(str, shape)), "dtype": np.dtype(dt).name, "wavelet": WNAME, "levels": 1, "mode": "symmetric",
                          "runs": "%d batches of %d calls after %d warm-up calls" % (a.reps, a.steps, a.warmup),
                          "us_per_call": {k: v[0] for k, v in res.items()}, "us_min": {k: v[1] for k, v in res.items()},
                          "compulsory_MB": round(nbytes / 1e6, 2), "GBps_compulsory": {k: round(nbytes / v[0] / 1e3, 1) for k, v in res.items()},
                          "forward_adjoint_over_inverse": round(res["forward_adjoint"][0] / res["inverse"][0], 2)}), flush=True)
        for p in [vol, out, tmp] + bands:
            H.pdwt_free(p)
    H.pdwt_event_destroy(ev[0])
    H.pdwt_event_destroy(ev[1])


if __name__ == "__main__":
    main()
