#!/usr/bin/env python3
"""Forward + inverse pairs of the batched 1-D wavelet packet transform (pdwt_amd.WaveletPackets1D, wpt1d.hip) on the MI355X.

Shapes: 8192 x 8192 float32 sym8 L4, 65536 x 512 float32 db4 L6, 4096 x 8192 float64 db20 L3.
Per shape: median and minimum us per forward+inverse pair (default basis: depth L) over --reps timed batches of --steps pairs (HIP
events on the library stream), the forward alone the same way (the inverse is the difference), and the rate on COMPULSORY bytes --
forward one read of the batch and one write of each of the L depths, inverse one read of depth L and one write of the batch -- against
the mixed-copy rate of profiles/r05_hbm_ceiling.md (5.4 TB/s).  Beside each figure, in the same process: the SAME instance forced
through the per-level entries of the C ABI (pdwt_wp1_forward_level_* / pdwt_wp1_inverse_level_*, L launches per direction, 2 L batches
of traffic per direction), and the pair of pdwt_amd.Wavelets(ndim=1) on the same batch and levels.
No speed is asserted anywhere: this tool only measures.
usage: python tools/bench_wpt1d.py [--steps 10] [--warmup 3] [--reps 5]     (prints one JSON line per shape)"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pdwt_amd  # noqa: E402
from pdwt_amd import _native as nat  # noqa: E402

COPY_TBS = 5.4
SHAPES = [((8192, 8192), np.float32, "sym8", 4), ((65536, 512), np.float32, "db4", 6), ((4096, 8192), np.float64, "db20", 3)]


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
        nr, nc = shape
        x = np.random.RandomState(0).uniform(-1, 1, shape).astype(dt)
        P = pdwt_amd.WaveletPackets1D(x, wname, levels)
        assert P.levels == levels, (P.levels, levels)

        def pair():
            P.forward()
            P.inverse()

        pair_us = timed(H, ev, a, pair)
        err = float(np.abs(P.get_image().astype(np.float64) - x).max())
        P.set_image(x)
        fwd_us = timed(H, ev, a, P.forward)
        # the same instance through the level entries: depth l -> l + 1 for every l, then back (all parents of every depth)
        sfx, FT = ("f32", nat.Filters32) if np.dtype(dt) == np.float32 else ("f64", nat.Filters64)
        f = FT()
        f.hlen = getattr(H, "pdwt_compute_filters_separable_" + sfx)(wname.encode(), 0, C.byref(f))
        ptr = [P.node_int_ptr((d, 0)) for d in range(levels + 1)]
        n = [P.node_shape(d)[1] for d in range(levels + 1)]
        lf, li = getattr(H, "pdwt_wp1_forward_level_" + sfx), getattr(H, "pdwt_wp1_inverse_level_" + sfx)

        def lev_fwd():
            for d in range(levels):
                assert lf(ptr[d], ptr[d + 1], nr, 2 ** d, n[d], C.byref(f)) == 0

        def lev_inv():
            for d in range(levels - 1, -1, -1):
                assert li(ptr[d], ptr[d + 1], nr, 2 ** d, n[d], None, 0, C.byref(f)) == 0

        lev_fwd_us = timed(H, ev, a, lev_fwd)
        lev_inv_us = timed(H, ev, a, lev_inv)
        item = np.dtype(dt).itemsize
        depth_elems = [nr * 2 ** d * n[d] for d in range(levels + 1)]
        nb_fwd, nb_inv = item * sum(depth_elems), item * (depth_elems[levels] + depth_elems[0])
        fused = bool(P.fused)
        P.close()
        W = pdwt_amd.Wavelets(x, wname, levels, ndim=1)
        assert W.info.nlevels == levels, (W.info.nlevels, levels)

        def wpair():
            W.forward()
            W.inverse()

        w_us = timed(H, ev, a, wpair)
        W.close()
        inv_us = round(pair_us[0] - fwd_us[0], 1)
        gb = lambda nb, us: round(nb / (us * 1e-6) / 1e9, 1)  # noqa: E731
        print(json.dumps({"shape": "x".join(map(str, shape)), "dtype": np.dtype(dt).name, "wavelet": wname, "levels": levels, "one_launch": fused,
                          "pair_us": pair_us[0], "pair_us_min": pair_us[1], "fwd_us": fwd_us[0], "fwd_us_min": fwd_us[1], "inv_us": inv_us,
                          "levels_fwd_us": lev_fwd_us[0], "levels_fwd_us_min": lev_fwd_us[1], "levels_inv_us": lev_inv_us[0], "levels_inv_us_min": lev_inv_us[1],
                          "fwd_over_levels": round(fwd_us[0] / lev_fwd_us[0], 3), "expected_fwd_over_levels": round((levels + 1) / (2.0 * levels), 3),
                          "inv_over_levels": round(inv_us / lev_inv_us[0], 3), "expected_inv_over_levels": round(1.0 / levels, 3),
                          "fwd_compulsory_MB": round(nb_fwd / 1e6, 1), "inv_compulsory_MB": round(nb_inv / 1e6, 1),
                          "fwd_GBps": gb(nb_fwd, fwd_us[0]), "inv_GBps": gb(nb_inv, inv_us), "fwd_frac_of_copy": round(gb(nb_fwd, fwd_us[0]) / (COPY_TBS * 1e3), 3),
                          "inv_frac_of_copy": round(gb(nb_inv, inv_us) / (COPY_TBS * 1e3), 3), "wavelets_pair_us": w_us[0], "wavelets_pair_us_min": w_us[1],
                          "packets_over_wavelets": round(pair_us[0] / w_us[0], 2), "maxerr_after_all_pairs": err}), flush=True)
    H.pdwt_event_destroy(ev[0])
    H.pdwt_event_destroy(ev[1])


if __name__ == "__main__":
    main()
