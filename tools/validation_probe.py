"""Cost of the validation tail on the device (mav_gt_stats_dev) next to the host tail the loops run with validation="host".

    python tools/validation_probe.py [--reps 50] [--host-reps 3] [--out FILE]
    python tools/validation_probe.py --loop [--frames 33] [--rounds 2] [--out FILE]

Default: device-resident inputs, HIP-event time (mav_timer_start / stop around ONE enqueue, synchronised), median of --reps after 5
warm-up enqueues, at 1280x720 and 1920x1080, batch 1 and 16, with a 24x24 and a 256x256 MAV (the second shows the sequential sum's cost;
max_pixels = 65536 so that it is not truncated).
  ms, phases_ms    the whole call; the four phases from mav_profile_get over --reps more enqueues (classes gt_stats_max / _count / _list / _sum)
  model_gbps       11 B/px (segmentation and depth read twice, sky once; the ground-truth flow is gathered at the listed pixels only) over ms
  membw_*          mav_membw_probe (a 3-read-1-write stream kernel) of the same run, at a cache-resident (4 x 32 MB) and an HBM (4 x 512 MB) size
  host_*_ms        in the same process, best of --host-reps, for ONE frame, times the batch: what the loop runs per frame with
                   validation="host": Processor._segmentation's np.nonzero(seg > 127) (host_nonzero_ms), Processor._gt_center's
                   get_simple_bounding_box through the helpers' context (host_center_ms) and the reference-rule validate_sky_segment --
                   as the reference writes it in numpy (host_sky_numpy_ms: tests/validation_ref.py's literal int64 sums) and through
                   mavflow.im_helpers.calculate_tpr_fpr (host_sky_helpers_ms); host_tail_ms adds the first two and the FASTER sky form
  equals_restatement   the records and lists of this run against tests/validation_ref.py (batch 1 rows)
--loop: Processor.run_detection() and run_detection_batched(16) over --frames frames of a moving-MAV dataset at 1920x1080 (Farneback
seam; segmentation, sky and depth change per frame, validate_sky_segment is the reference's rule), validation="host" and "device" in
alternation, --rounds times: ms per frame, wall clock around the loop.
One JSON line per configuration."""
from __future__ import annotations

import argparse
import json
import logging
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "mav-detection_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import validation_ref as R  # noqa: E402
from mavflow import _lib, _validation as V, im_helpers  # noqa: E402

WARM = 5
MAX_PIXELS = 65536
PHASES = ("gt_stats_max", "gt_stats_count", "gt_stats_list", "gt_stats_sum")


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


def scene(W, H, mav, seed):
    rng = np.random.default_rng(seed)
    seg = np.zeros((H, W), np.uint8)
    seg[H // 4:H // 4 + mav, W // 4:W // 4 + mav] = 255
    depth = rng.uniform(1, 99, (H, W)).astype(np.float32)
    depth[H // 2, W // 2] = 100.0
    sky = ((depth > 80) ^ (rng.random((H, W)) < 0.1))
    gt = rng.normal(0, 3, (H, W, 2)).astype(np.float32)
    return seg, gt, sky, depth


def reference_rule(sky_mask, depth_buffer):
    """Dataset.validate_sky_segment (src/datasets/dataset.py:173-175) through this package's calculate_tpr_fpr"""
    sky_mask_gt = depth_buffer > 0.80 * np.max(depth_buffer)
    return im_helpers.calculate_tpr_fpr(sky_mask_gt * 255, sky_mask)


def kernels(args):
    lines = []
    omega, dt = np.array([0.12, -0.06, 0.03]), 1 / 30.0
    for (W, H) in ((1280, 720), (1920, 1080)):
        npx = W * H
        for mav in (24, 256):
            seg, gt, sky, depth = scene(W, H, mav, W + mav)
            seg3 = np.repeat(seg[..., None], 3, axis=2)
            host = dict(host_nonzero_ms=best_of(lambda: np.nonzero(np.ascontiguousarray(seg3[..., 0]) > 127), args.host_reps),
                        host_center_ms=best_of(lambda: im_helpers.get_simple_bounding_box(seg).get_center(), args.host_reps),
                        host_sky_numpy_ms=best_of(lambda: R.sky_counts(sky, depth), args.host_reps),
                        host_sky_helpers_ms=best_of(lambda: reference_rule(sky, depth), args.host_reps))
            tail1 = host["host_nonzero_ms"] + host["host_center_ms"] + min(host["host_sky_numpy_ms"], host["host_sky_helpers_ms"])
            want = R.gt_stats(seg, gt, sky, depth, omega, dt, 0, MAX_PIXELS)
            for B in (1, 16):
                with _lib.Context(W, H, B) as ctx:
                    membw_cache, membw_hbm = ctx.membw_probe(32 << 20), ctx.membw_probe(512 << 20, reps=5)
                    rep = lambda a: np.ascontiguousarray(np.broadcast_to(a, (B,) + a.shape))
                    par = V.gt_stats_params(omega, dt, batch=B)
                    bufs = [ctx.alloc(a.nbytes).upload(a) for a in (rep(seg), rep(gt), rep(sky.astype(np.uint8)), rep(depth), par)]
                    d_rec, d_idx = ctx.alloc(96 * B), ctx.alloc(4 * MAX_PIXELS * B)
                    call = lambda: ctx.gt_stats_enqueue(bufs[0], bufs[1], bufs[2], bufs[3], bufs[4], B, MAX_PIXELS, d_rec, d_idx)
                    ms = timed(ctx, call, args.reps)
                    ctx.profile_enable(True)
                    for _ in range(args.reps):
                        call()
                    ctx.sync()
                    prof = ctx.profile_get()
                    ctx.profile_enable(False)
                    rec, idx = d_rec.download(V.RECORD_DTYPE, (B,)), d_idx.download(np.int32, (B, MAX_PIXELS))
                    same = bool(all(rec[b].tobytes() == want[0].tobytes() and np.array_equal(idx[b], want[1]) for b in range(B)))
                    model = 11 * npx * B
                    lines.append(dict(probe="gt_stats", W=W, H=H, batch=B, mav=f"{mav}x{mav}", ms=round(ms, 4),
                                      phases_ms={k[len("gt_stats_"):]: round(prof[k][0] / max(prof[k][1], 1), 4) for k in PHASES},
                                      model_mb=round(model / 1e6, 1), model_gbps=round(model / (ms * 1e-3) / 1e9, 1),
                                      membw_cache_gbps=round(membw_cache, 1), membw_hbm_gbps=round(membw_hbm, 1),
                                      **{k: round(v * B, 2) for k, v in host.items()}, host_tail_ms=round(tail1 * B, 2),
                                      device_faster_by=round(tail1 * B / ms, 1), equals_restatement=same))
                    for b in bufs + [d_rec, d_idx]:
                        b.free()
    return lines


def loops(args):
    from mavflow.processor import Processor, SyntheticDataset
    from mavflow.run_config import RunConfig
    W, H, N = 1920, 1080, args.frames

    class Moving(SyntheticDataset):
        """SyntheticDataset (four distinct pairs) whose MAV patch moves and whose sky and depth change per frame; nothing declared constant"""
        def __init__(self):
            super().__init__(W, H, N, use_farneback=True, dangle=(0.004, -0.002, 0.001), distinct=4)
            self.constant_segmentation = self.constant_sky_segmentation = False
            self._img = {}

        def _images(self, i):
            if i not in self._img:
                seg, _, sky, depth = scene(W, H, 24, 1000 + i)
                seg3 = np.zeros((H, W, 3), np.uint8)
                seg3[H // 4 + 5 * i:H // 4 + 5 * i + 24, W // 4 + 7 * i:W // 4 + 7 * i + 24] = 255
                self._img[i] = (seg3, sky, depth)
            return self._img[i]

        def get_segmentation(self, i):
            return self._images(i)[0]

        def get_sky_segmentation(self, i):
            return self._images(i)[1]

        def get_depth(self, i):
            return self._images(i)[2]

        def validate_sky_segment(self, sky_mask, depth_buffer):
            return reference_rule(sky_mask, depth_buffer)

    lines = []
    ds = Moving()
    for i in range(N):
        ds._images(i)
        ds._pair(i)
    for rnd in range(args.rounds):
        for loop in ("run_detection", "run_detection_batched"):
            for mode in ("host", "device"):
                ds._frame_cursor = 0
                np.random.seed(5)
                p = Processor(RunConfig(logging.getLogger("probe"), ds, "", False, False, False, True, False, False, "FLOW_FOE_CLUSTERING"), validation=mode)
                try:
                    run = (lambda: p.run_detection_batched(batch=16)) if loop == "run_detection_batched" else p.run_detection
                    if rnd == 0:                                   # contexts, workspaces and code objects exist after one pass
                        run()
                        p.frame_index = 0
                        p.detection_results.clear()
                    t0 = time.perf_counter()
                    res = run()
                    dt = time.perf_counter() - t0
                    r = res[N - 2]
                    lines.append(dict(probe="loop", loop=loop + ("(16)" if loop.endswith("batched") else ""), validation=mode, W=W, H=H, frames=N - 1, round=rnd,
                                      ms_per_frame=round(dt * 1e3 / (N - 1), 3), last_frame=dict(sky_tpr=float(r.sky_tpr), sky_fpr=float(r.sky_fpr),
                                                                                                  drone_size_pixels=int(r.drone_size_pixels),
                                                                                                  center_phi=float(r.center_phi))))
                finally:
                    p.release()
    ds.release()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--loop", action="store_true")
    ap.add_argument("--frames", type=int, default=33)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = loops(args) if args.loop else kernels(args)
    text = "\n".join(json.dumps(x) for x in lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
