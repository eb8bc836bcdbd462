#!/usr/bin/env python3
"""Forward + inverse pairs of the batched 1-D DWT with boundary modes (pdwt_amd.BoundaryWavelets1D, dwt_ext1d.hip) on the MI355X.

Shapes: 8192 x 8192 float32 sym8 L4 `symmetric` (the C4 batch), 65536 x 512 float32 db4 L3, 4096 x 8192 float64 db20 L3.
Per shape: median and minimum us per forward+inverse pair over --reps timed batches of --steps pairs (HIP events on the library stream),
and the rate on COMPULSORY bytes -- per direction one read of the batch and one write of every band (forward), the reverse (inverse);
the bands have the expanded length (n + hlen - 1) / 2 per level -- against the mixed-copy rate of profiles/r05_hbm_ceiling.md
(5.4 TB/s).  Beside each, in the same process, the periodised pair of pdwt_amd.Wavelets(ndim=1) on the same batch and levels.
No speed is asserted anywhere: this tool only measures.
usage: python tools/bench_ext1d.py [--steps 10] [--warmup 3] [--reps 5]     (prints one JSON line per shape)"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pdwt_amd  # noqa: E402

COPY_TBS = 5.4
SHAPES = [((8192, 8192), np.float32, "sym8", 4, "symmetric"), ((65536, 512), np.float32, "db4", 3, "symmetric"),
          ((4096, 8192), np.float64, "db20", 3, "symmetric")]


def time_pairs(H, ev, W, a):
    for _ in range(a.warmup):
        W.forward()
        W.inverse()
    W.sync()
    us = []
    for _ in range(a.reps):
        H.pdwt_event_record(ev[0])
        for _ in range(a.steps):
            W.forward()
            W.inverse()
        H.pdwt_event_record(ev[1])
        H.pdwt_event_sync(ev[1])
        us.append(1e3 * H.pdwt_event_elapsed_ms(ev[0], ev[1]) / a.steps)
    return float(np.median(us)), float(min(us))


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
    for shape, dt, wname, levels, mode in SHAPES:
        x = np.random.RandomState(0).uniform(-1, 1, shape).astype(dt)
        B = pdwt_amd.BoundaryWavelets1D(x, wname, levels, mode)
        assert B.levels == levels, (B.levels, levels)
        fused = bool(B.fused)
        med, best = time_pairs(H, ev, B, a)
        err = float(np.abs(B.get_image().astype(np.float64) - x).max())
        item = np.dtype(dt).itemsize
        nb = 2 * item * (shape[0] * shape[1] + sum(B.coeff_shape(k)[0] * B.coeff_shape(k)[1] for k in range(B.nbands)))  # both directions
        B.close()
        W = pdwt_amd.Wavelets(x, wname, levels, ndim=1)
        assert W.info.nlevels == levels, (W.info.nlevels, levels)
        wmed, wbest = time_pairs(H, ev, W, a)
        W.close()
        gbs = nb / (med * 1e-6) / 1e9
        print(json.dumps({"shape": "x".join(map(str, shape)), "dtype": np.dtype(dt).name, "wavelet": wname, "levels": levels, "mode": mode,
                          "one_launch": fused, "launches_per_pair": 2 if fused else 2 * levels, "us_per_pair": round(med, 1), "us_min": round(best, 1),
                          "compulsory_MB": round(nb / 1e6, 1), "GBps_compulsory": round(gbs, 1), "frac_of_copy": round(gbs / (COPY_TBS * 1e3), 3),
                          "wavelets_us_per_pair": round(wmed, 1), "wavelets_us_min": round(wbest, 1), "boundary_over_wavelets": round(med / wmed, 2),
                          "roundtrip_maxerr": err}), flush=True)
    H.pdwt_event_destroy(ev[0])
    H.pdwt_event_destroy(ev[1])


if __name__ == "__main__":
    main()
