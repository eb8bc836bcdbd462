#!/usr/bin/env python3
"""Forward + inverse pairs of the batched 2-D wavelet packet transform (pdwt_amd.WaveletPacketBatch, wpt2db.hip) on the MI355X.

Shapes: 256 x 64^2 float32, 64 x 128^2 float32, 64 x 128^2 float64, 64 x 512^2 float32 and (one image per compute unit) 256 x 128^2
float32, all db4 L3.
Per shape: median and minimum us per forward+inverse pair (default basis: depth L) over --reps timed batches of --steps pairs (HIP
events on the library stream), the forward alone the same way (the inverse is the difference), the launches per pair, and the rate on
COMPULSORY bytes -- forward one read of the batch and one write of each of the L depths, inverse one read of depth L and one write of
the batch.  Beside each figure, in the same process: an instance on the same images with allow_fused=False (the level entries over the
forest: 2 L launches per pair while a depth has at most 16384 parents, 2 L batches of traffic per direction), and a loop over B
pdwt_amd.WaveletPackets2D instances (2 L B launches per pair).  Where the plan does not fuse (64 x 128^2 float64, 64 x 512^2 float32) the
first two are the same form.  Expected ratio of the fused form to the per-depth form: forward about (L + 1) / 2 L, inverse about 1 / L.
No speed is asserted anywhere: this tool only measures.
usage: python tools/bench_wptb.py [--steps 10] [--warmup 3] [--reps 5]     (prints one JSON line per shape)"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pdwt_amd  # noqa: E402

SHAPES = [((256, 64, 64), np.float32, "db4", 3), ((64, 128, 128), np.float32, "db4", 3), ((64, 128, 128), np.float64, "db4", 3),
          ((64, 512, 512), np.float32, "db4", 3), ((256, 128, 128), np.float32, "db4", 3)]


def timed(H, ev, a, step):
    for _ in range(a.warmup):
        step()
    H.pdwt_sync()
    us = []
    for _ in range(a.reps):
        H.pdwt_event_record(ev[0])
        for _ in range(a.steps):
            step()
        H.pdwt_event_record(ev[1])
        H.pdwt_event_sync(ev[1])
        us.append(1e3 * H.pdwt_event_elapsed_ms(ev[0], ev[1]) / a.steps)
    return round(float(np.median(us)), 1), round(float(min(us)), 1)


def pair_and_forward(H, ev, a, objs):
    def fwd():
        for o in objs:
            o.forward()

    def pair():
        for o in objs:
            o.forward()
            o.inverse()

    p = timed(H, ev, a, pair)
    f = timed(H, ev, a, fwd)  # (on whatever images the last pair left: the time does not depend on them)
    return p, f


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
    for shape, dt, wname, levels in SHAPES:
        B = shape[0]
        x = np.random.RandomState(0).uniform(-1, 1, shape).astype(dt)
        P = pdwt_amd.WaveletPacketBatch(x, wname, levels)
        assert P.levels == levels, (P.levels, levels)
        fused = bool(P.fused)
        pair_us, fwd_us = pair_and_forward(H, ev, a, [P])
        P.set_image(x)
        P.forward()
        P.inverse()
        err = float(np.abs(P.get_image().astype(np.float64) - x).max())
        item = np.dtype(dt).itemsize
        depth_elems = [B * 4 ** d * P.node_shape(d)[0] * P.node_shape(d)[1] for d in range(levels + 1)]
        nb_fwd, nb_inv = item * sum(depth_elems), item * (depth_elems[levels] + depth_elems[0])
        chunks = sum(-(-(B * 4 ** d) // 16384) for d in range(levels))  # level launches per direction
        P.close()
        D = pdwt_amd.WaveletPacketBatch(x, wname, levels, allow_fused=False)
        assert not D.fused
        d_pair_us, d_fwd_us = pair_and_forward(H, ev, a, [D])
        D.close()
        S = [pdwt_amd.WaveletPackets2D(x[b], wname, levels) for b in range(B)]
        s_pair_us, s_fwd_us = pair_and_forward(H, ev, a, S)
        for s in S:
            s.close()
        inv_us, d_inv_us, s_inv_us = (round(p[0] - f[0], 1) for p, f in ((pair_us, fwd_us), (d_pair_us, d_fwd_us), (s_pair_us, s_fwd_us)))
        gb = lambda nb, us: round(nb / (us * 1e-6) / 1e9, 1)  # noqa: E731
        print(json.dumps({"shape": "x".join(map(str, shape)), "dtype": np.dtype(dt).name, "wavelet": wname, "levels": levels, "fused": fused,
                          "launches_per_pair": 2 if fused else 2 * chunks, "pair_us": pair_us[0], "pair_us_min": pair_us[1], "fwd_us": fwd_us[0],
                          "fwd_us_min": fwd_us[1], "inv_us": inv_us,
                          "per_depth_launches_per_pair": 2 * chunks, "per_depth_pair_us": d_pair_us[0], "per_depth_pair_us_min": d_pair_us[1],
                          "per_depth_fwd_us": d_fwd_us[0], "per_depth_fwd_us_min": d_fwd_us[1], "per_depth_inv_us": d_inv_us,
                          "fwd_over_per_depth": round(fwd_us[0] / d_fwd_us[0], 3), "expected_fwd_over_per_depth": round((levels + 1) / (2.0 * levels), 3),
                          "inv_over_per_depth": round(inv_us / d_inv_us, 3), "expected_inv_over_per_depth": round(1.0 / levels, 3),
                          "loop_launches_per_pair": 2 * levels * B, "loop_pair_us": s_pair_us[0], "loop_pair_us_min": s_pair_us[1], "loop_fwd_us": s_fwd_us[0],
                          "loop_inv_us": s_inv_us, "loop_over_batch": round(s_pair_us[0] / pair_us[0], 1),
                          "fwd_compulsory_MB": round(nb_fwd / 1e6, 1), "inv_compulsory_MB": round(nb_inv / 1e6, 1),
                          "fwd_GBps": gb(nb_fwd, fwd_us[0]), "inv_GBps": gb(nb_inv, inv_us), "maxerr_after_one_pair": err}), flush=True)
    H.pdwt_event_destroy(ev[0])
    H.pdwt_event_destroy(ev[1])


if __name__ == "__main__":
    main()
