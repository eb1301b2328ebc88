"""Cost of the robust essential-matrix fit on the device (mav_find_essential_dev, mav_flow_essential_dev) next to the fundamental fit of
the same pairs and a host stand-in.

    python tools/essential_probe.py [--reps 50] [--sizes 1280x720] [--batches 1,16] [--out FILE]

Device-resident inputs, HIP-event time (mav_timer_start / stop around ONE enqueue, synchronised), median of --reps after 5 warm-up
enqueues; n = 1000 pairs, max_iters = 1000 hypotheses, subsets from essential.sample_subsets(seed 1).  The scene per frame size is
tools/fundamental_probe.py's (30 % of the sampled pixels carry a gross vector of their own), the camera its K.
Per row:
  form = pairs   mav_find_essential_dev on resident pairs
  form = flow    mav_flow_essential_dev, coords from the host with the call
  ms             the whole enqueue
  parts_ms       the call's launches in order (flow: gather first; fit: models, score, choose, finish) from the library's own profile
                 (mav_profile_intervals), median of 10 profiled calls
  fundamental_ms mav_find_fundamental_dev (n = 1000, max_iters = 1000) on the same pairs, alternating with the enqueue in the same
                 process: for scale, no ratio is demanded
  standin_ms     in the same process: tests/essential_ref.py's restatement on ONE item, times the batch.  A STAND-IN for the host route,
                 not cv2 (there is no cv2 here)
  equals_standin E, F, mask and record of item 0 against the stand-in's bytes
One JSON line per configuration."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "mav-detection_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import essential_ref as R  # noqa: E402
import fundamental_ref as FR  # noqa: E402
from fundamental_probe import N, ITERS, alternating, per_launch, scene  # noqa: E402
from mavflow import _lib, essential, fundamental  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--sizes", default="1280x720")
    ap.add_argument("--batches", default="1,16")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    for size in args.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        cam = (0.8 * W, 0.8 * W, (W - 1) / 2, (H - 1) / 2)
        for B in (int(v) for v in args.batches.split(",")):
            flow, coords = scene(W, H, B, W + B)
            sub = essential.sample_subsets(1, N, ITERS, B)
            sub7 = fundamental.sample_subsets(1, N, ITERS, B)
            src, dst = FR.flow_pairs(flow, coords)
            t0 = time.perf_counter()
            ref = R.find_one(src[0], dst[0], sub[0], 1.0, 0.999, cam)
            standin = (time.perf_counter() - t0) * 1e3 * B
            with _lib.Context(W, H, B) as ctx:
                need = ctx.find_essential_workspace_bytes(N, B, ITERS)
                fneed = ctx.find_fundamental_workspace_bytes(N, B, ITERS)
                bufs = [ctx.alloc(flow.nbytes).upload(flow), ctx.alloc(src.nbytes).upload(src), ctx.alloc(dst.nbytes).upload(dst),
                        ctx.alloc(sub.nbytes).upload(sub), ctx.alloc(72 * B), ctx.alloc(72 * B), ctx.alloc(N * B), ctx.alloc(32 * B), ctx.alloc(need),
                        ctx.alloc(sub7.nbytes).upload(sub7), ctx.alloc(72 * B), ctx.alloc(fneed)]
                df, ds, dd, dt, dE, dF, di, dr, dw, dt7, dF7, dfw = bufs
                fund = lambda: ctx.find_fundamental_enqueue(ds, dd, N, B, dt7, dF7, di, dr, dfw, fneed, threshold=1.0, max_iters=ITERS)
                kw = dict(threshold=1.0, confidence=0.999, max_iters=ITERS, camera=cam)
                forms = {
                    "pairs": (lambda: ctx.find_essential_enqueue(ds, dd, N, B, dt, dE, dF, di, dr, dw, need, **kw), 4),
                    "flow": (lambda: ctx.flow_essential_enqueue(df, coords, B, dt, dE, dF, di, dr, dw, need, **kw), 5),
                }
                for form, (call, launches) in forms.items():
                    ms, fund_ms = alternating(ctx, (call, fund), args.reps)
                    call()
                    parts = per_launch(ctx, call, launches)
                    rec = dr.download(essential.RECORD_DTYPE, (B,))
                    same = bool(dE.download(np.float64, (B, 3, 3))[0].tobytes() == ref["E"].tobytes()
                                and dF.download(np.float64, (B, 3, 3))[0].tobytes() == ref["F"].tobytes()
                                and rec[0].tobytes() == ref["record"].tobytes() and np.array_equal(di.download(np.uint8, (B, N))[0], ref["inliers"]))
                    row = dict(probe="essential", form=form, W=W, H=H, n=N, max_iters=ITERS, batch=B, ms=round(ms, 4), parts_ms=parts,
                               fundamental_ms=round(fund_ms, 4), iters_run=int(rec[0]["iters_run"]), inliers=int(rec[0]["inliers"]),
                               valid=int(rec[0]["valid"]), workspace_kb=round(need / 1e3, 1), standin="tests/essential_ref.py (numpy), not cv2",
                               standin_ms=round(standin, 1), device_faster_by=round(standin / ms, 1), equals_standin=same)
                    lines.append(row)
                    print(json.dumps(row), flush=True)
                for b in bufs:
                    b.free()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(json.dumps(x) for x in lines) + "\n")


if __name__ == "__main__":
    main()
