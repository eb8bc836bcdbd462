#!/usr/bin/env python3
"""Forward + inverse pairs of the 3-D stationary transform (pdwt_amd.StationaryWavelets3D, swt3d.hip) on the MI355X.

Shapes: 256^3 float32 db4 L3, 512^3 float32 db4 L2, 256^3 float64 db20 L2 (what the level clamp allows: ilog2(256 / 39) = 2).
Per shape: median us per forward+inverse pair over --reps timed batches of --steps pairs (HIP events on the library stream),
and the rate on COMPULSORY bytes -- per level, the forward reads its input volume once and writes the 8 full-size bands once
(9 volumes), the inverse reads the 8 bands and writes its output (9 volumes) -- against the measured ~6.3 TB/s device copy rate.
Launch structure: two launches per level and direction (x-y tile kernel + z kernel), which move 17 volumes per
level and direction: the bound of that form is 9/17 = 53 % of the copy rate.
usage: python tools/bench_swt3d.py [--steps 10] [--warmup 3] [--reps 5]     (prints one JSON line per shape)"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pdwt_amd  # noqa: E402

COPY_TBS = 6.3
SHAPES = [((256, 256, 256), np.float32, "db4", 3), ((512, 512, 512), np.float32, "db4", 2), ((256, 256, 256), np.float64, "db20", 2)]


def compulsory_bytes(W):
    return 2 * 9 * int(np.prod(W.shape)) * W.levels * W.dtype.itemsize


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    pdwt_amd.require_gpu()
    H = pdwt_amd.hip()
    H.pdwt_set_device(0)
    e0, e1 = H.pdwt_event_create(), H.pdwt_event_create()
    for shape, dt, wname, levels in SHAPES:
        vol = np.random.RandomState(0).uniform(-1, 1, shape).astype(dt)
        W = pdwt_amd.StationaryWavelets3D(vol, wname, levels)
        assert W.levels == levels, (W.levels, levels)
        for _ in range(a.warmup):
            W.forward()
            W.inverse()
        W.sync()
        us = []
        for _ in range(a.reps):
            H.pdwt_event_record(e0)
            for _ in range(a.steps):
                W.forward()
                W.inverse()
            H.pdwt_event_record(e1)
            H.pdwt_event_sync(e1)
            us.append(1e3 * H.pdwt_event_elapsed_ms(e0, e1) / a.steps)
        err = float(np.abs(W.get_image().astype(np.float64) - vol).max())
        med = float(np.median(us))
        nb = compulsory_bytes(W)
        gbs = nb / (med * 1e-6) / 1e9
        print(json.dumps({"shape": "x".join(map(str, shape)), "dtype": np.dtype(dt).name, "wavelet": wname, "levels": W.levels,
                          "launches_per_pair": 4 * W.levels, "us_per_pair": round(med, 1), "us_min": round(min(us), 1),
                          "compulsory_MB": round(nb / 1e6, 1), "GBps_compulsory": round(gbs, 1),
                          "frac_of_copy": round(gbs / (COPY_TBS * 1e3), 3), "roundtrip_maxerr": err}), flush=True)
        W.close()
    H.pdwt_event_destroy(e0)
    H.pdwt_event_destroy(e1)


if __name__ == "__main__":
    main()
