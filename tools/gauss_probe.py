"""Probe: what the Gaussian window (cv2.OPTFLOW_FARNEBACK_GAUSSIAN, mav_set_window) costs against the box window.

    python tools/gauss_probe.py [--steps 200] [--warmup 5] [--out profiles/gaussian/gauss_probe.txt]

One process, two shapes -- 1920x1080 x 64 pairs (bench.py's flagship shape, steps and warm-up) and 1280x720 x 1 pair -- device-
resident frames, the call bench.py times (mav_process_batch_dev).  Per shape a box and a Gaussian context take turns, block by
block (box, gaussian, box, gaussian ...: drift of the machine falls on both alike), then each runs a few profiled steps of its own
for the sweep kernels' busy time (mav_profile_busy, run mode: the union of the sweep launches' intervals over both streams).
The two windows move identical bytes: whatever the ratio exceeds 1 by is arithmetic, LDS or occupancy.
"""
import argparse
import sys
import time

sys.path.insert(0, "mav-detection_amd")
import numpy as np
from mavflow import _lib, synth

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--blocks", type=int, default=4, help="alternating blocks per window; steps are split among them")
ap.add_argument("--profiled", type=int, default=10, help="profiled steps per window for the busy time")
ap.add_argument("--out", default=None, help="append the result lines to this file too")
args = ap.parse_args()
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def setup(W, H, B, window, prev, nxt, smp):
    c = _lib.Context(W, H, B, window=window)
    bufs = [c.alloc(prev.nbytes).upload(prev), c.alloc(nxt.nbytes).upload(nxt), c.alloc(smp.nbytes).upload(smp), c.alloc(32 * B),
            c.alloc(B * W * H), c.alloc(B * W * H)]
    return c, bufs


def run(cb, B, n):
    c, b = cb
    for _ in range(n):
        c.process_batch_dev(b[0].ptr, b[1].ptr, b[2].ptr, B, b[3].ptr, mf_ptr=b[4].ptr, md_ptr=b[5].ptr)
    c.sync()


for W, H, B, steps in ((1920, 1080, 64, args.steps), (1280, 720, 1, args.steps * 5)):
    prev, nxt = synth.make_batch(W, H, B, distinct=min(B, 4))
    smp = np.stack([synth.foe_samples(W, H, b) for b in range(B)])
    ctxs = {w: setup(W, H, B, w, prev, nxt, smp) for w in ("box", "gaussian")}
    per_block = max(1, steps // args.blocks)
    total = {w: 0.0 for w in ctxs}
    for w in ctxs:
        run(ctxs[w], B, args.warmup)
    for _ in range(args.blocks):
        for w in ctxs:
            t0 = time.perf_counter()
            run(ctxs[w], B, per_block)
            total[w] += time.perf_counter() - t0
    ms = {w: 1e3 * total[w] / (per_block * args.blocks) for w in ctxs}
    busy = {}
    for w, (c, _) in ctxs.items():
        c.profile_enable(2)
        run(ctxs[w], B, args.profiled)
        busy[w] = c.profile_busy("blur_iter", "blur_iter_coarse") / args.profiled
        c.profile_enable(False)
    say(f"{W}x{H} x {B} pair(s), {per_block * args.blocks} steps in {args.blocks} alternating blocks, warm-up {args.warmup}")
    for w in ctxs:
        say(f"  {w:8s} {ms[w]:8.3f} ms/step  {B / ms[w] * 1e3:8.0f} pairs/s  sweeps busy {busy[w]:7.3f} ms/step")
    say(f"  gaussian / box: step {ms['gaussian'] / ms['box']:.3f}, sweeps busy {busy['gaussian'] / busy['box']:.3f}")
    for c, _ in ctxs.values():
        c.close()

if args.out:
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
