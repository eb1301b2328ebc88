"""Cost of the robust affine fit on the device (mav_estimate_affine_dev, mav_flow_affine_dev) next to the homography fit and a host stand-in.

    python tools/affine_probe.py [--reps 50] [--sizes 1280x720,1920x1080] [--batches 1,64] [--out FILE]

Device-resident inputs, HIP-event time (mav_timer_start / stop around ONE enqueue, synchronised), median of --reps after 5 warm-up
enqueues; n = 1000 pairs, max_iters = 2000, triples from affine.sample_triples(seed 1).  Two scenes per frame size, float32 fields of an
affine camera motion with noise and one patch that moves on its own:
  clean       every other pair follows the motion: the early stop leaves after a few hypotheses' worth of niters
  outliers40  40 % of the sampled pixels carry a gross vector of their own
Per row (form = pairs: mav_estimate_affine_dev on resident pairs; form = flow: mav_flow_affine_dev, coords from the host with the call):
  ms                     the whole enqueue
  gather_ms, score_ms, choose_ms, finish_ms
                         the call's launches in order, from the library's own profile (mav_profile_enable(1): mav_profile_get reports the
                         class total, all four being class "misc"; mav_profile_intervals splits it by launch), median of 10 profiled calls
  iters_run, inliers     of item 0's record
  homography_ms          mav_find_homography_dev (pairs) / mav_flow_homography_dev (flow) on the same pairs, alternating with the affine
                         enqueue in the same process: for scale, no ratio is demanded
  standin_ms             in the same process: tests/affine_ref.py's numpy restatement on ONE item, times the batch.  A STAND-IN for the host
                         route, not cv2 (there is no cv2 here)
  equals_standin         M, mask and record of item 0 against the stand-in's bytes
One JSON line per configuration."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "mav-detection_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import affine_ref as R  # noqa: E402
from mavflow import _lib, affine  # noqa: E402
from mavflow._lib import check  # noqa: E402

WARM, N, ITERS, PROFILED = 5, 1000, 2000, 10


def scene(W, H, B, outliers, seed):
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    flow = np.empty((B, H, W, 2), np.float32)
    coords = np.column_stack([rng.integers(20, W - 20, N), rng.integers(20, H - 20, N)]).astype(np.int32)
    for b in range(B):
        M = np.array([[1.004, 0.003, -1.25], [-0.002, 0.997, 0.75]]) + 1e-4 * b
        f = np.stack([M[0, 0] * xs + M[0, 1] * ys + M[0, 2] - xs, M[1, 0] * xs + M[1, 1] * ys + M[1, 2] - ys], axis=-1)
        f += rng.normal(0, 0.15, f.shape)
        f[H // 3:H // 3 + 24, W // 2:W // 2 + 24] += (3.0, -2.0)
        if outliers:
            bad = rng.permutation(N)[:int(N * outliers)]
            f[coords[bad, 1], coords[bad, 0]] += rng.uniform(-40, 40, (len(bad), 2))
        flow[b] = f
    return flow, coords


def alternating(ctx, calls, reps):
    """median ms of each enqueue, the calls taking turns"""
    for _ in range(WARM):
        for call in calls:
            call()
    ctx.sync()
    ts = [[] for _ in calls]
    for _ in range(reps):
        for k, call in enumerate(calls):
            ctx.timer_start()
            call()
            ts[k].append(ctx.timer_stop())
    return [float(np.median(t)) for t in ts]


def per_launch(ctx, call, launches):
    """median ms of the call's launches, in order, from the library's profile"""
    ctx.sync()
    ctx.profile_enable(1)
    for _ in range(PROFILED):
        call()
    ctx.sync()
    total = ctx.profile_get()
    _, _, t0, t1 = ctx.profile_intervals()
    ctx.profile_enable(0)
    d = (t1 - t0)[-PROFILED * launches:].reshape(PROFILED, launches)
    return [float(v) for v in np.median(d, axis=0)], {k: v for k, v in total.items() if v[1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--sizes", default="1280x720,1920x1080")
    ap.add_argument("--batches", default="1,64")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    vp = lambda b: C.c_void_p(int(b.ptr))
    for size in args.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        for B in (int(v) for v in args.batches.split(",")):
            for sname, share in (("clean", 0.0), ("outliers40", 0.4)):
                flow, coords = scene(W, H, B, share, W + B)
                tri = affine.sample_triples(1, N, ITERS, B)
                src, dst = R.flow_pairs(flow, coords)
                t0 = time.perf_counter()
                ref = R.estimate_one(src[0], dst[0], tri[0])
                standin = (time.perf_counter() - t0) * 1e3 * B
                with _lib.Context(W, H, B) as ctx:
                    need = ctx.estimate_affine_workspace_bytes(N, B, ITERS)
                    bufs = [ctx.alloc(flow.nbytes).upload(flow), ctx.alloc(src.nbytes).upload(src), ctx.alloc(dst.nbytes).upload(dst),
                            ctx.alloc(tri.nbytes).upload(tri), ctx.alloc(48 * B), ctx.alloc(N * B), ctx.alloc(32 * B), ctx.alloc(need), ctx.alloc(72 * B),
                            ctx.alloc(4 * B)]
                    df, ds, dd, dt, dM, di, dr, dw, dH, dok = bufs
                    cptr = coords.ctypes.data_as(C.c_void_p)
                    forms = {
                        "pairs": (lambda: ctx.estimate_affine_enqueue(ds, dd, N, B, dt, dM, di, dr, dw, need),
                                  lambda: check(ctx.lib.mav_find_homography_dev(ctx.h, vp(ds), vp(dd), N, B, vp(dH), vp(dok))), 3),
                        "flow": (lambda: ctx.flow_affine_enqueue(df, coords, B, dt, dM, di, dr, dw, need),
                                 lambda: check(ctx.lib.mav_flow_homography_dev(ctx.h, vp(df), cptr, N, B, vp(dH), vp(dok))), 4),
                    }
                    for form, (fit, hom, launches) in forms.items():
                        ms, hom_ms = alternating(ctx, (fit, hom), args.reps)
                        parts, total = per_launch(ctx, fit, launches)
                        parts = [0.0] * (4 - launches) + parts
                        rec = dr.download(affine.RECORD_DTYPE, (B,))
                        same = bool(dM.download(np.float64, (B, 2, 3))[0].tobytes() == ref["M"].tobytes() and rec[0].tobytes() == ref["record"].tobytes()
                                    and np.array_equal(di.download(np.uint8, (B, N))[0], ref["inliers"]))
                        lines.append(dict(probe="affine", form=form, scene=sname, W=W, H=H, n=N, max_iters=ITERS, batch=B, ms=round(ms, 4),
                                          gather_ms=round(parts[0], 4), score_ms=round(parts[1], 4), choose_ms=round(parts[2], 4), finish_ms=round(parts[3], 4),
                                          profile_get={k: [round(v[0], 4), v[1]] for k, v in total.items()},
                                          iters_run=int(rec[0]["iters_run"]), inliers=int(rec[0]["inliers"]), refined=int(rec[0]["refined"]),
                                          homography_ms=round(hom_ms, 4), workspace_kb=round(need / 1e3, 1),
                                          standin="tests/affine_ref.py (numpy), not cv2", standin_ms=round(standin, 1),
                                          device_faster_by=round(standin / ms, 1), not_slower=bool(ms <= standin), equals_standin=same))
                        print(json.dumps(lines[-1]), flush=True)
                    for b in bufs:
                        b.free()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(json.dumps(x) for x in lines) + "\n")


if __name__ == "__main__":
    main()
