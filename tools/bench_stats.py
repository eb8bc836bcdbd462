#!/usr/bin/env python3
"""Times the band statistics and the noise-adaptive thresholds (bandstats.hip) of one Wavelets instance on the MI355X, next to the
existing one-read reduction over the same bands, norm1_f64().

Legs, each timed with device events on the library stream over --reps repetitions after --warmup, median reported in us (every leg
ends in its own copy to the host, so a repetition is a whole call):
  (a) norm1_f64()  (norm cache off: a real reduction)      (b) all_band_stats(with_median=False)
  (c) estimate_sigma()                                      (d) denoise("bayes") (the coefficients are restored before each repetition,
                                                                outside the timed window)
  (e) the host round trip (d) replaces: get_coeff(finest diagonal band) + numpy median + soft_threshold, host clock
on the random-data coefficients ("random") and on the same coefficients after soft_threshold ("sparse": mostly zeros).
--norm1-only runs leg (a) alone through API that predates the statistics, so the same script measures an older checkout.
usage: python tools/bench_stats.py [--shape 4096 4096] [--dtype float32] [--wavelet db4] [--levels 3] [--reps 30] [--warmup 5] [--norm1-only]
(prints one JSON line)"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pdwt_amd  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=2, default=[4096, 4096])
    ap.add_argument("--dtype", default="float32")
    ap.add_argument("--wavelet", default="db4")
    ap.add_argument("--levels", type=int, default=3)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--norm1-only", action="store_true")
    a = ap.parse_args()
    assert a.reps >= 20, "at least 20 repetitions"
    pdwt_amd.require_gpu()
    H = pdwt_amd.hip()
    H.pdwt_set_device(0)
    e0, e1 = H.pdwt_event_create(), H.pdwt_event_create()
    dt = np.dtype(a.dtype)
    x = np.random.RandomState(0).standard_normal(a.shape).astype(dt)
    W = pdwt_amd.Wavelets(x, a.wavelet, a.levels, norm_cache=False)
    W.forward()
    W.sync()
    saved = None if a.norm1_only else W.copy()

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

    def restore():  # the coefficients as they were before the last denoise (device-to-device, outside the timed window)
        for k in range(W.nbands):
            W.set_coeff(saved.coeff_view(k), k)
        W.sync()

    fin = 3 if W.info.ndims == 2 else 1
    out = {"shape": "x".join(map(str, a.shape)), "dtype": dt.name, "wavelet": a.wavelet, "levels": W.info.nlevels, "reps": a.reps,
           "bytes_all_bands": int(sum(np.prod(W.band_shape(k)) for k in range(W.nbands)) * dt.itemsize),
           "bytes_finest_diagonal": int(np.prod(W.band_shape(fin)) * dt.itemsize)}
    for data in ("random", "sparse"):
        if data == "sparse":
            beta = 2.0 * float(np.median(np.abs(W.get_coeff(fin))))
            W.soft_threshold(beta)
            if saved is not None:
                saved.soft_threshold(beta)
            W.sync()
            out["sparse_zero_fraction_finest"] = round(float((W.get_coeff(fin) == 0).mean()), 3)
        r = {}
        r["norm1_f64_us"], r["norm1_f64_min_us"] = timed(W.norm1_f64)
        if not a.norm1_only:
            r["all_band_stats_us"], r["all_band_stats_min_us"] = timed(lambda: W.all_band_stats(with_median=False))
            r["estimate_sigma_us"], r["estimate_sigma_min_us"] = timed(W.estimate_sigma)
            r["denoise_bayes_us"], r["denoise_bayes_min_us"] = timed(lambda: W.denoise("bayes"), before=restore)
            host = []
            for i in range(3):
                restore()
                t0 = time.perf_counter()
                d1 = W.get_coeff(fin)
                sigma = float(np.median(np.abs(d1))) / 0.6744897501960817
                W.soft_threshold(sigma)
                W.sync()
                host.append(1e6 * (time.perf_counter() - t0))
            restore()
            r["host_round_trip_us"] = round(float(np.median(host)), 1)
            r["all_band_stats_over_norm1"] = round(r["all_band_stats_us"] / r["norm1_f64_us"], 3)
            r["estimate_sigma_over_norm1"] = round(r["estimate_sigma_us"] / r["norm1_f64_us"], 3)
        out[data] = r
    print(json.dumps(out), flush=True)
    H.pdwt_event_destroy(e0)
    H.pdwt_event_destroy(e1)


if __name__ == "__main__":
    main()
