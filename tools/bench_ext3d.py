#!/usr/bin/env python3
"""Forward + inverse pairs of the 3-D DWT with boundary modes (pdwt_amd.BoundaryWavelets3D, dwt_ext3d.hip) on the MI355X.

Shapes: 256^3 float32 db4 L3 `symmetric`, 128^3 float64 db20 L1 `symmetric`.
Per shape: median us per forward+inverse pair over --reps timed batches of --steps pairs (HIP events on the library stream), and the
rate on COMPULSORY bytes -- per level and pair one read and one write of the level's input, of the four x-y quadrants
(nz x hr x hc each) and of the eight expanded bands ((n + hlen - 1) / 2 per axis) -- against the measured ~6.3 TB/s device copy rate.
(The two-pass kernels move the quadrants twice per direction: "moved_MB" counts that.)  Two launches per level and direction.  Beside each, in the same process right after, the periodised pair of pdwt_amd.Wavelets3D on
the same volume and levels, and the halo growth of the bands: the elements of the eight bands over those of the level input, summed over
the levels (about ((n + hlen - 1) / n)^3).
No speed is asserted anywhere: this tool only measures.
usage: python tools/bench_ext3d.py [--steps 10] [--warmup 3] [--reps 5]     (prints one JSON line per shape)"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pdwt_amd  # noqa: E402

COPY_TBS = 6.3
SHAPES = [((256, 256, 256), np.float32, "db4", 3, "symmetric"), ((128, 128, 128), np.float64, "db20", 1, "symmetric")]


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
        vol = np.random.RandomState(0).uniform(-1, 1, shape).astype(dt)
        B = pdwt_amd.BoundaryWavelets3D(vol, wname, levels, mode)
        assert B.levels == levels, (B.levels, levels)
        med, best = time_pairs(H, ev, B, a)
        err = float(np.abs(B.get_image().astype(np.float64) - vol).max())
        item = np.dtype(dt).itemsize
        geo = [shape] + [B.coeff_shape(B.band_index(l, "ddd")) for l in range(1, levels + 1)]  # the approximation of level 0 .. L
        elems = moved = 0
        for l in range(1, levels + 1):
            (z0, r0, c0), (z1, r1, c1) = geo[l - 1], geo[l]
            elems += z0 * r0 * c0 + 4 * z0 * r1 * c1 + 8 * z1 * r1 * c1
            moved += z0 * r0 * c0 + 2 * 4 * z0 * r1 * c1 + 8 * z1 * r1 * c1  # the quadrants are written and read in each direction
        nb, nmoved = 2 * item * elems, 2 * item * moved  # one read and one write of each / both directions
        growth = sum(8 * np.prod(geo[l]) for l in range(1, levels + 1)) / sum(np.prod(geo[l - 1]) for l in range(1, levels + 1))
        B.close()
        W = pdwt_amd.Wavelets3D(vol, wname, levels)
        assert W.levels == levels, (W.levels, levels)
        wmed, _ = time_pairs(H, ev, W, a)
        W.close()
        gbs = nb / (med * 1e-6) / 1e9
        print(json.dumps({"shape": "x".join(map(str, shape)), "dtype": np.dtype(dt).name, "wavelet": wname, "levels": levels, "mode": mode,
                          "launches_per_pair": 4 * levels, "us_per_pair": round(med, 1), "us_min": round(best, 1), "runs": a.reps, "pairs_per_run": a.steps,
                          "compulsory_MB": round(nb / 1e6, 1), "moved_MB": round(nmoved / 1e6, 1), "GBps_compulsory": round(gbs, 1), "frac_of_copy": round(gbs / (COPY_TBS * 1e3), 3),
                          "wavelets3d_us_per_pair": round(wmed, 1), "boundary_over_wavelets3d": round(med / wmed, 2),
                          "band_elements_over_input": round(float(growth), 3), "roundtrip_maxerr": err}), flush=True)
    H.pdwt_event_destroy(ev[0])
    H.pdwt_event_destroy(ev[1])


if __name__ == "__main__":
    main()
