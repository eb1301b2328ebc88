"""Cost of the flow pictures on the device (include/mavflow_vis.h), next to the host route and the existing flow_to_color pass.

    python tools/vis_probe.py [--reps 50] [--rounds 5] [--frames 12] [--out FILE]

Device-resident, HIP-event time (mav_timer_start / stop around ONE enqueue, synchronised), median of --reps after 3 warm-up enqueues, at
1280x720 and 1920x1080, batch 1 and 64, on the synthetic scene's flow (synth.true_flow):
  mav_flow_hsv_dev      MAV_HSV_PROCESS (records' initialisation + minimum / maximum pass + picture) and MAV_HSV_DRAW (one launch)
  mav_cvt_color_dev     COLOR_HSV2BGR and COLOR_BGR2HSV
  mav_draw_flow_dev     step 8, threshold 1
  flow_to_color         mav_render_dev with only the flow image asked for -- the existing pass of the same shape (a reduction, then a
                        render, 8 B/px in and 3 out; a one-block launch packs its per-pair constants in every call) -- against MAV_HSV_PROCESS:
                        --rounds medians of each, taken in alternation in this process; the margin is the pool's spread, 2 %
Per line: ms (one enqueue of the whole batch), model_mb (what the pass must read and write, once each: PROCESS reads the flow twice),
model_gbps beside membw_*: mav_membw_probe (a 3-read-1-write stream kernel) of the same process at a cache-resident (4 x 32 MB) and an HBM
(4 x 512 MB) size.
Then, per frame size: the host route for one frame (mavflow.farneback.flow_to_hsv + hsv_to_bgr, best of 3) and Farneback.process() per
frame in both `vis` modes on a synthetic video held in memory (wall clock over --frames frames after 2 warm-up frames; each process()
ends with the picture on the host).  One JSON line per configuration."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "mav-detection_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from mavflow import _lib, synth, vis  # noqa: E402
from mavflow.farneback import Farneback, flow_to_hsv, hsv_to_bgr  # noqa: E402

SIZES = ((1280, 720), (1920, 1080))
BATCHES = (1, 64)


class MemoryCapture:
    def __init__(self, frames):
        self.frames, self.i = frames, 0

    def read(self):
        f = self.frames[self.i % len(self.frames)]
        self.i += 1
        return True, f


def timed(ctx, reps, enqueue):
    for _ in range(3):
        enqueue()
    ctx.sync()
    ts = []
    for _ in range(reps):
        ctx.timer_start()
        enqueue()
        ts.append(ctx.timer_stop())
    return float(np.median(ts))


def replicate(ctx, a, B):
    d = ctx.alloc(B * a.nbytes)
    for b in range(B):
        _lib.check(ctx.lib.mav_memcpy_h2d(ctx.h, d.ptr + b * a.nbytes, _lib._ptr(a), a.nbytes))
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)

    rng = np.random.default_rng(1)
    for W, H in SIZES:
        flow = np.ascontiguousarray(synth.true_flow(W, H), np.float32)
        pic = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        n0 = W * H
        for B in BATCHES:
            with _lib.Context(W, H, B) as ctx:
                common = dict(probe="vis", size=[W, H], batch=B, membw_probe_cache_gbps=round(ctx.membw_probe(32 << 20), 1),
                              membw_probe_hbm_gbps=round(ctx.membw_probe(512 << 20, reps=5), 1))
                d_flow, d_pic = replicate(ctx, flow, B), replicate(ctx, pic, B)
                d_bgr, d_rec = ctx.alloc(3 * n0 * B), ctx.alloc(16 * B)
                d_frame0 = ctx.alloc(B).upload(np.ones(B, np.uint8))            # mav_render_dev reads its per-pair flags on the device
                assert vis.vis_form(W, H, B, d_flow.ptr, d_bgr.ptr, None) == vis.FORM_FAST

                def line(case, enqueue, model):
                    ms = timed(ctx, args.reps, enqueue)
                    emit(dict(common, case=case, ms=round(ms, 4), model_mb=round(model / 1e6, 2), model_gbps=round(model / (ms * 1e-3) / 1e9, 1)))

                process = lambda: ctx.flow_hsv_enqueue(d_flow, d_bgr, d_rec, "process", batch=B)
                to_color = lambda: ctx.render_dev(d_flow.ptr, None, B, flow_img_ptr=d_bgr.ptr, frame0_ptr=d_frame0.ptr)
                line("mav_flow_hsv_dev PROCESS", process, B * n0 * (8 + 8 + 3))
                line("mav_flow_hsv_dev DRAW", lambda: ctx.flow_hsv_enqueue(d_flow, d_bgr, d_rec, "draw", batch=B), B * n0 * (8 + 3))
                line("mav_cvt_color_dev HSV2BGR", lambda: ctx.cvt_color_enqueue(d_pic, vis.COLOR_HSV2BGR, d_bgr, batch=B), B * n0 * 6)
                line("mav_cvt_color_dev BGR2HSV", lambda: ctx.cvt_color_enqueue(d_pic, vis.COLOR_BGR2HSV, d_bgr, batch=B), B * n0 * 6)
                nx, ny = len(range(4, W, 8)), len(range(4, H, 8))
                line("mav_draw_flow_dev step 8", lambda: ctx.draw_flow_enqueue(d_pic, d_flow, 8, 1.0, (0, 255, 0), batch=B), B * nx * ny * 8)
                ours, theirs = [], []
                for _ in range(args.rounds):
                    theirs.append(timed(ctx, args.reps, to_color))
                    ours.append(timed(ctx, args.reps, process))
                mo, mt = float(np.median(ours)), float(np.median(theirs))
                emit(dict(common, case="MAV_HSV_PROCESS against flow_to_color (mav_render_dev, flow image only), in alternation", rounds=args.rounds,
                          process_ms=[round(v, 4) for v in ours], flow_to_color_ms=[round(v, 4) for v in theirs], process_median_ms=round(mo, 4),
                          flow_to_color_median_ms=round(mt, 4), ratio=round(mo / mt, 3), process_slower_than_2_percent=bool(mo > 1.02 * mt)))
                for b in (d_flow, d_pic, d_bgr, d_rec, d_frame0):
                    b.free()
        # the host route for one frame, and the class in both modes
        host = []
        for _ in range(3):
            t0 = time.perf_counter()
            hsv_to_bgr(flow_to_hsv(flow)[0])
            host.append(time.perf_counter() - t0)
        emit(dict(probe="vis", size=[W, H], case="host route, one frame: flow_to_hsv + hsv_to_bgr (numpy)", ms=round(min(host) * 1e3, 2)))
        video = [np.ascontiguousarray(np.repeat(f[..., None], 3, axis=2)) for f in synth.make_sequence(W, H, 6)]
        per = {}
        for mode in ("host", "device"):
            fb = Farneback(MemoryCapture(video), None, vis=mode)
            for _ in range(2):
                fb.process()
            t0 = time.perf_counter()
            for _ in range(args.frames):
                fb.process()
            per[mode] = (time.perf_counter() - t0) / args.frames * 1e3
            fb.close()
            fb.ctx.close()
        emit(dict(probe="vis", size=[W, H], case="Farneback.process() per frame, BGR frames in memory", frames=args.frames,
                  host_ms=round(per["host"], 3), device_ms=round(per["device"], 3), speedup=round(per["host"] / per["device"], 2)))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
