#!/usr/bin/env python3
"""Times the band statistics and the noise-adaptive thresholds of a whole ImageBatch (bandbatch.hip) on the MI355X:
  denoise("bayes"), denoise("visu"), estimate_sigma(), all_band_stats()
each timed with device events on the library stream over --reps repetitions after --warmup, median and minimum reported in us.  A
repetition is a WHOLE call: it ends with its results on the host.  Before every denoise the coefficients are restored from a second
batch, outside the timed window.

--loop times what the batched calls replace, `for b in range(B): batch[b].<same call>()`, through API that predates them, so the
same script measures an older checkout.
usage: python tools/bench_batch_stats.py [--batch 64] [--shape 512 512] [--dtype float32] [--wavelet db4] [--levels 3] [--reps 30]
                                         [--warmup 5] [--loop] [--only denoise_bayes]
(prints one JSON line)"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pdwt_amd  # noqa: E402

LEGS = ["denoise_bayes", "denoise_visu", "estimate_sigma", "all_band_stats"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--shape", type=int, nargs=2, default=[512, 512])
    ap.add_argument("--dtype", default="float32")
    ap.add_argument("--wavelet", default="db4")
    ap.add_argument("--levels", type=int, default=3)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--loop", action="store_true", help="image after image through the single-image methods")
    ap.add_argument("--only", choices=LEGS, default=None, help="one leg, once warm: for a kernel trace of a single call (--reps 1 allowed)")
    a = ap.parse_args()
    assert a.only or a.reps >= 30, "at least 30 repetitions"
    pdwt_amd.require_gpu()
    H = pdwt_amd.hip()
    H.pdwt_set_device(0)
    e0, e1 = H.pdwt_event_create(), H.pdwt_event_create()
    dt = np.dtype(a.dtype)
    B = a.batch
    x = np.random.RandomState(0).standard_normal((B, a.shape[0], a.shape[1])).astype(dt)
    batch, saved = pdwt_amd.ImageBatch(x, a.wavelet, a.levels), pdwt_amd.ImageBatch(x, a.wavelet, a.levels)
    batch.forward()
    saved.forward()
    batch.sync()
    views = [batch[b] for b in range(B)]
    keep = [saved[b] for b in range(B)]
    nb = views[0].nbands

    def restore():  # the coefficients as they were before the last denoise (device-to-device, outside the timed window)
        for b in range(B):
            for k in range(1, nb):
                views[b].set_coeff(keep[b].coeff_view(k), k)
        batch.sync()

    def timed(fn, before=None):
        us = []
        for i in range(a.warmup + a.reps):
            if before:
                before()
            H.pdwt_event_record(e0)
            fn()
            H.pdwt_event_record(e1)
            H.pdwt_event_sync(e1)
            if i >= a.warmup:
                us.append(1e3 * H.pdwt_event_elapsed_ms(e0, e1))
        return round(float(np.median(us)), 2), round(float(min(us)), 2)

    if a.loop:
        calls = {"denoise_bayes": lambda: [w.denoise("bayes") for w in views], "denoise_visu": lambda: [w.denoise("visu") for w in views],
                 "estimate_sigma": lambda: [w.estimate_sigma() for w in views],
                 "all_band_stats": lambda: [w.all_band_stats(with_median=False) for w in views]}
    else:
        calls = {"denoise_bayes": lambda: batch.denoise("bayes"), "denoise_visu": lambda: batch.denoise("visu"),
                 "estimate_sigma": batch.estimate_sigma, "all_band_stats": lambda: batch.all_band_stats(with_median=False)}
    out = {"mode": "loop" if a.loop else "batched", "batch": B, "shape": "x".join(map(str, a.shape)), "dtype": dt.name, "wavelet": a.wavelet,
           "levels": views[0].info.nlevels, "nbands": nb, "reps": a.reps, "transform_batched": bool(batch.batched)}
    for leg in ([a.only] if a.only else LEGS):
        out[leg + "_us"], out[leg + "_min_us"] = timed(calls[leg], before=restore if leg.startswith("denoise") else None)
    print(json.dumps(out), flush=True)
    H.pdwt_event_destroy(e0)
    H.pdwt_event_destroy(e1)


if __name__ == "__main__":
    main()
