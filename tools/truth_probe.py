"""Cost of the ground-truth flow (mav_gt_flow_dev) and of the radial-error histogram (mav_radial_error_hist_dev) on the device, next to
the host restatements of the same arithmetic.

    python tools/truth_probe.py [--reps 50] [--host-reps 2] [--out FILE]

Device-resident, HIP-event time (mav_timer_start / stop around ONE enqueue, synchronised), median of --reps after 5 warm-up enqueues, at
1280x720 and 1920x1080, batch 1 and 16.
  gt_flow      both output depths; model bytes = 5 B/px read (float32 depth + uint8 segmentation) + 8 (float32) or 16 (float64) written
  radial_hist  the default 159 x 159 bins on a synthetic scene (tests/truth_cases.py: targets spread over the bins) and on the one-cell
               field (every pixel in one cell: every wave adds once); model bytes = 17 B/px read (two float32 fields + uint8 sky)
  membw_*      mav_membw_probe (a 3-read-1-write stream kernel) of the same run, at a cache-resident (4 x 32 MB) and an HBM (4 x 512 MB) size
  host_restatement_ms   tests/truth_ref.py (numpy, the reference's operation order) on the host for ONE frame, best of --host-reps in
               the same process, times the batch: a stand-in for the reference's functions, which are not on the GPU machine (the
               restatement is held bit for bit to their arrays by tests/test_truth_ref_cpu.py; the reference's own loop adds its
               transposes and np.save on top)
One JSON line per configuration."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "mav-detection_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import truth_cases as T  # noqa: E402
import truth_ref as R  # noqa: E402
from mavflow import _lib, _truth  # noqa: E402

WARM = 5


def best_of(fn, reps):
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best * 1e3


def timed(ctx, enqueue, reps):
    for _ in range(WARM):
        enqueue()
    ctx.sync()
    ts = []
    for _ in range(reps):
        ctx.timer_start()
        enqueue()
        ts.append(ctx.timer_stop())
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    for (W, H) in ((1280, 720), (1920, 1080)):
        rng = np.random.default_rng(W)
        npx = W * H
        depth1 = rng.uniform(1, 200, (H, W)).astype(np.float32)
        seg1 = ((rng.random((H, W)) < 0.02) * 255).astype(np.uint8)
        vp1, vp2 = T.view_proj(1, W, H), T.view_proj(2, W, H)
        inv, disp = np.linalg.inv(vp2), np.array([12.5, -3.25, 7.0])
        host_gt = best_of(lambda: R.gt_flow(depth1, seg1, vp1, inv, disp, 100.0), args.host_reps)
        flow1, gt1, sky1 = T.scene(W, W, H, 1, *T.DEFAULT_EDGES)
        one_flow = np.broadcast_to(np.array(T.ONE_CELL_FLOW, np.float32), (1, H, W, 2)).copy()
        one_gt = np.broadcast_to(np.array(T.ONE_CELL_GT, np.float32), (1, H, W, 2)).copy()
        host_hist = {"scene": best_of(lambda: R.radial_hist(flow1, gt1, sky1), args.host_reps),
                     "one cell": best_of(lambda: R.radial_hist(one_flow, one_gt, sky1), args.host_reps)}
        for B in (1, 16):
            with _lib.Context(W, H, B) as ctx:
                membw_cache, membw_hbm = ctx.membw_probe(32 << 20), ctx.membw_probe(512 << 20, reps=5)
                common = dict(W=W, H=H, batch=B, membw_cache_gbps=round(membw_cache, 1), membw_hbm_gbps=round(membw_hbm, 1))
                # ---- the reprojection
                d_depth = ctx.alloc(npx * 4 * B).upload(np.broadcast_to(depth1, (B, H, W)).copy())
                d_seg = ctx.alloc(npx * B).upload(np.broadcast_to(seg1, (B, H, W)).copy())
                par = _truth.gt_flow_params(vp1, inv, disp, 100.0, B)
                d_par = ctx.alloc(par.nbytes).upload(par)
                d_out = ctx.alloc(npx * 16 * B)
                for dtype in (np.float32, np.float64):
                    ms = timed(ctx, lambda: ctx.gt_flow_enqueue(d_depth, d_seg, d_par, B, d_out, dtype=dtype), args.reps)
                    model = (5 + 2 * np.dtype(dtype).itemsize) * npx * B
                    got = d_out.download(dtype, (B, H, W, 2))[B - 1]
                    with np.errstate(all="ignore"):
                        same = R.same_bits(got, R.gt_flow(depth1, seg1, vp1, inv, disp, 100.0).astype(dtype)) if B == 1 else None
                    lines.append(dict(probe="gt_flow", out=np.dtype(dtype).name, **common, ms=round(ms, 4), model_mb=round(model / 1e6, 1),
                                      model_gbps=round(model / (ms * 1e-3) / 1e9, 1), host_restatement_ms=round(host_gt * B, 1),
                                      device_faster_by=round(host_gt * B / ms, 1), equals_restatement=same))
                for b in (d_depth, d_seg, d_par, d_out):
                    b.free()
                # ---- the histogram
                d_sky = ctx.alloc(npx * B).upload(np.broadcast_to(sky1.astype(np.uint8), (B, H, W)).copy())
                for field, (fl, gt) in (("scene", (flow1, gt1)), ("one cell", (one_flow, one_gt))):
                    d_fl = ctx.alloc(npx * 8 * B).upload(np.broadcast_to(fl, (B, H, W, 2)).copy())
                    d_gt = ctx.alloc(npx * 8 * B).upload(np.broadcast_to(gt, (B, H, W, 2)).copy())
                    acc = ctx.radial_error_accumulator()
                    ms = timed(ctx, lambda: acc.add_enqueue(d_fl, d_gt, d_sky, B), args.reps)
                    acc.reset()
                    acc.add_enqueue(d_fl, d_gt, d_sky, B)
                    got, want = acc.counts(), R.radial_hist(fl, gt, sky1)
                    same = bool(np.array_equal(got["counts"], B * want["counts"]) and got["non_sky"] == B * want["non_sky"])
                    model = 17 * npx * B
                    lines.append(dict(probe="radial_hist", field=field, bins="159x159", **common, ms=round(ms, 4), model_mb=round(model / 1e6, 1),
                                      model_gbps=round(model / (ms * 1e-3) / 1e9, 1), host_restatement_ms=round(host_hist[field] * B, 1),
                                      device_faster_by=round(host_hist[field] * B / ms, 1), equals_restatement=same))
                    acc.close()
                    d_fl.free()
                    d_gt.free()
                d_sky.free()
    text = "\n".join(json.dumps(x) for x in lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
