#!/usr/bin/env python3
"""The batched 3-D boundary-mode drivers (dwt_ext3db.hip: a stack of V volumes, every level in one call) next to the loop they replace, on
the MI355X, straight through the C ABI on device buffers.

Settings: db2, 2 levels, `symmetric`.  Shapes: float32 at 64 x 32^3, 16 x 64^3 and 4 x 128^3; float64 at 16 x 64^3.  For each of the four
operators (forward, inverse, forward_adjoint, inverse_adjoint), us per call of
  (a) batched   pdwt_ext3db_<operator>_*: one call for the stack;
  (b) loop      the chain of level entries (pdwt_ext3d_<operator>_level_*) on each of the V volumes in turn, enqueued back to back with no
                host synchronisation inside the timed region (what pdwt_amd.functional did per volume, without its two synchronisations
                per call).
Method of tools/bench_adj3d.py: HIP events on the library stream, --warmup calls, then the median us per call over --reps timed batches of
--steps calls, with the fastest and the slowest batch beside it (their distance is the spread the comparison is read against).
The last line is the wall time of pdwt_amd.functional.dwt3 plus its backward pass on the 64 x 32^3 float32 tensor (shape (8, 8, 32, 32, 32)),
torch synchronised before and after; --functional-only prints that line alone and touches no batched symbol, so it also runs on a commit
that has none.  No speed is asserted anywhere: this tool only measures.
usage: python tools/bench_ext3db.py [--steps 10] [--warmup 3] [--reps 5] [--functional-only]     (prints one JSON line per shape)"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pdwt_amd  # noqa: E402
from pdwt_amd import _native as nat  # noqa: E402

SHAPES = [(64, (32, 32, 32), np.float32), (16, (64, 64, 64), np.float32), (4, (128, 128, 128), np.float32), (16, (64, 64, 64), np.float64)]
WNAME, LEVELS, MODE = "db2", 2, 2  # symmetric
OPS = ("forward", "inverse", "forward_adjoint", "inverse_adjoint")


def time_calls(H, ev, call, a):
    for _ in range(a.warmup):
        call()
    H.pdwt_sync()
    us = []
    for _ in range(a.reps):
        H.pdwt_event_record(ev[0])
        for _ in range(a.steps):
            call()
        H.pdwt_event_record(ev[1])
        H.pdwt_event_sync(ev[1])
        us.append(1e3 * H.pdwt_event_elapsed_ms(ev[0], ev[1]) / a.steps)
    return round(float(np.median(us)), 1), round(float(min(us)), 1), round(float(max(us)), 1)


def level_shapes(shape, hlen, levels):
    out = [tuple(shape)]
    for _ in range(levels):
        out.append(tuple((n + hlen - 1) // 2 for n in out[-1]))
    return out


def loop_calls(H, sfx, op, V, shapes, item, fp, vol, bands, approx, tmp):
    """the level-entry calls of the whole stack, prepared: [(function, arguments)] in the order they are enqueued"""
    L = len(shapes) - 1
    fn = getattr(H, "pdwt_ext3d_%s_level_%s" % (op, sfx))
    size = lambda l: int(np.prod(shapes[l])) * item  # noqa: E731
    calls = []
    down = op in ("forward", "inverse_adjoint")
    for v in range(V):
        for l in (range(1, L + 1) if down else range(L, 0, -1)):
            aaa = bands[0] + v * size(L) if l == L else approx[l - 1]
            fine = vol + v * size(0) if l == 1 else approx[l - 2]  # the volume of shape [l - 1]: read going down, written going up
            k0 = 1 + 7 * (L - l)
            tab = (C.c_void_p * 8)(aaa, *[b + v * size(l) for b in bands[k0:k0 + 7]])
            args = (fine, tab) + shapes[l - 1] + ((MODE,) if op in ("forward", "forward_adjoint") else ()) + (fp, tmp)
            calls.append((fn, args))
    return calls


def bench_shape(H, ev, V, shape, dt, a):
    item = np.dtype(dt).itemsize
    sfx = "f32" if item == 4 else "f64"
    f = (nat.Filters32 if sfx == "f32" else nat.Filters64)()
    f.hlen = getattr(H, "pdwt_compute_filters_separable_" + sfx)(WNAME.encode(), 0, C.byref(f))
    fp = C.byref(f)
    shapes = level_shapes(shape, f.hlen, LEVELS)
    tshapes = [shapes[LEVELS]] + [shapes[l] for l in range(LEVELS, 0, -1) for _ in range(7)]
    tmp_n = H.pdwt_ext3db_adjoint_tmp_elems(V, *shape, f.hlen, LEVELS)
    lvl_n = H.pdwt_ext3d_adjoint_level_tmp_elems(*shape, f.hlen)
    assert tmp_n > 0 and lvl_n > 0
    x = np.random.RandomState(0).standard_normal((V,) + shape).astype(dt)
    vol, out = H.pdwt_malloc(x.nbytes), H.pdwt_malloc(x.nbytes)
    bands = [H.pdwt_malloc(V * int(np.prod(s)) * item) for s in tshapes]
    approx = [H.pdwt_malloc(int(np.prod(shapes[l])) * item) for l in range(1, LEVELS)]  # aaa of the levels 1 .. L - 1 of one volume
    tmp, ltmp = H.pdwt_malloc(tmp_n * item), H.pdwt_malloc(lvl_n * item)
    assert vol and out and tmp and ltmp and all(bands) and all(approx)
    assert H.pdwt_memcpy_h2d(vol, x.ctypes.data, x.nbytes) == 0
    tab = (C.c_void_p * len(bands))(*bands)
    g = lambda op: getattr(H, "pdwt_ext3db_%s_%s" % (op, sfx))  # noqa: E731
    batched = {"forward": lambda: g("forward")(vol, tab, V, *shape, LEVELS, MODE, fp, tmp), "inverse": lambda: g("inverse")(out, tab, V, *shape, LEVELS, fp, tmp),
               "forward_adjoint": lambda: g("forward_adjoint")(out, tab, V, *shape, LEVELS, MODE, fp, tmp),
               "inverse_adjoint": lambda: g("inverse_adjoint")(vol, tab, V, *shape, LEVELS, fp, tmp)}
    res = {}
    for op in OPS:  # (forward first: it fills the bands the others read)
        assert batched[op]() == 0
        calls = loop_calls(H, sfx, op, V, shapes, item, fp, vol if op in ("forward", "inverse_adjoint") else out, bands, approx, ltmp)
        assert all(fn(*args) == 0 for fn, args in calls)

        def loop(calls=calls):
            for fn, args in calls:
                fn(*args)

        res[op] = {"batched": time_calls(H, ev, batched[op], a), "loop": time_calls(H, ev, loop, a)}
    H.pdwt_sync()
    print(json.dumps({"stack": "%d x %s" % (V, "x".join(map(str, shape))), "dtype": np.dtype(dt).name, "wavelet": WNAME, "levels": LEVELS, "mode": "symmetric",
                      "runs": "%d batches of %d calls after %d warm-up calls" % (a.reps, a.steps, a.warmup),
                      "us_per_call [median, min, max]": res,
                      "batched_over_loop": {op: round(res[op]["batched"][0] / res[op]["loop"][0], 3) for op in OPS},
                      "slower_by_more_than_the_spread": [op for op in OPS if res[op]["batched"][0] - res[op]["loop"][0]
                                                         > max(res[op]["batched"][2] - res[op]["batched"][1], res[op]["loop"][2] - res[op]["loop"][1])]}), flush=True)
    for p in [vol, out, tmp, ltmp] + bands + approx:
        H.pdwt_free(p)


def functional_wall(a):
    import torch
    F = pdwt_amd.functional
    g = torch.Generator().manual_seed(0)
    x = torch.randn((8, 8, 32, 32, 32), generator=g, dtype=torch.float32).cuda().requires_grad_(True)
    grads = None
    ms = []
    for it in range(a.warmup + a.reps):
        x.grad = None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        bands = F.dwt3(x, WNAME, LEVELS, "symmetric")
        if grads is None:
            grads = [torch.ones_like(b) for b in bands]
            torch.cuda.synchronize()
            t0 = time.perf_counter()  # (the first pass is a warm-up pass anyway)
        torch.autograd.backward(bands, grads)
        torch.cuda.synchronize()
        if it >= a.warmup:
            ms.append(1e3 * (time.perf_counter() - t0))
    print(json.dumps({"functional": "dwt3 + backward", "tensor": "8x8x32x32x32 float32", "wavelet": WNAME, "levels": LEVELS, "mode": "symmetric",
                      "wall_ms [median, min, max]": [round(float(np.median(ms)), 2), round(min(ms), 2), round(max(ms), 2)],
                      "runs": "%d after %d warm-up passes" % (a.reps, a.warmup)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--functional-only", action="store_true")
    a = ap.parse_args()
    pdwt_amd.require_gpu()
    H = pdwt_amd.hip()
    H.pdwt_set_device(0)
    if not a.functional_only:
        ev = (H.pdwt_event_create(), H.pdwt_event_create())
        for V, shape, dt in SHAPES:
            bench_shape(H, ev, V, shape, dt, a)
        H.pdwt_event_destroy(ev[0])
        H.pdwt_event_destroy(ev[1])
    functional_wall(a)


if __name__ == "__main__":
    main()
