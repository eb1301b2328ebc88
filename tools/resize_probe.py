"""Cost of the image resize on the device (include/mavflow_resize.h), next to a host stand-in.

    python tools/resize_probe.py [--reps 50] [--rounds 7] [--host-reps 3] [--out FILE]

Device-resident, HIP-event time (mav_timer_start / stop around ONE enqueue, synchronised), median of --reps after 3 warm-up enqueues, at
the sizes a user of the detection loop runs, batch 1 and 16:
  sky picture             U8C3   960x512  -> 1920x1024  linear        (the HRNet prediction, Dataset.get_sky_segmentation)
  fused sky mask          U8C3   960x512  -> 1920x1024  linear + key  (mav_sky_mask_dev: the picture is never written)
  half-resolution images  U8C3  1920x1080 ->  960x540   area          (resize_percent(img, 50), the 2 x 2 form)
  flow, enlarging         F32C2  960x512  -> 1920x1024  linear        (get_gt_of)
  flow, general area      F32C2 1920x1080 -> 1280x720   area          (ratio 1.5)
  nearest                 U8C1   960x512  -> 1920x1024  nearest
Per line:
  ms          one enqueue of the whole batch
  model_mb    the source read once plus the destination written once
  model_gbps  model bytes over ms, beside membw_* : mav_membw_probe (a 3-read-1-write stream kernel) of the same process at a
              cache-resident (4 x 32 MB) and an HBM (4 x 512 MB) size
  host_standin_ms_per_image   torch.nn.functional.interpolate on the CPU (bilinear / area / nearest; float32, the uint8 cases converted
              before the clock starts) on one image, best of --host-reps: a stand-in, not cv2 (not installed), and not the same arithmetic
The fused sky mask against mav_resize_dev of the same picture: --rounds medians of each, taken in alternation in this process; the margin
is the spread (max - min) of the unfused call's own medians.  One JSON line per configuration."""
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

from mavflow import _lib, resize, warp  # noqa: E402

FORMATS = {"U8C1": (warp.WARP_U8C1, np.uint8, 1), "U8C3": (warp.WARP_U8C3, np.uint8, 3), "F32C2": (warp.WARP_F32C2, np.float32, 2)}
CASES = [("sky picture", "U8C3", (960, 512), (1920, 1024), resize.INTER_LINEAR, False),
         ("fused sky mask", "U8C3", (960, 512), (1920, 1024), resize.INTER_LINEAR, True),
         ("half-resolution images", "U8C3", (1920, 1080), (960, 540), resize.INTER_AREA, False),
         ("flow, enlarging", "F32C2", (960, 512), (1920, 1024), resize.INTER_LINEAR, False),
         ("flow, general area", "F32C2", (1920, 1080), (1280, 720), resize.INTER_AREA, False),
         ("nearest", "U8C1", (960, 512), (1920, 1024), resize.INTER_NEAREST, False)]
METHOD = {resize.INTER_LINEAR: "linear", resize.INTER_AREA: "area", resize.INTER_NEAREST: "nearest"}


def host_standin(img, dsize, interp, reps):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(img.reshape(img.shape[0], img.shape[1], -1).transpose(2, 0, 1)[None].astype(np.float32)))
    mode = {resize.INTER_LINEAR: "bilinear", resize.INTER_AREA: "area", resize.INTER_NEAREST: "nearest"}[interp]
    kw = dict(align_corners=False) if mode == "bilinear" else {}
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        torch.nn.functional.interpolate(t, size=(dsize[1], dsize[0]), mode=mode, **kw)
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best * 1e3


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)

    rng = np.random.default_rng(1)
    host_ms = {}
    for B in (1, 16):
        with _lib.Context(1920, 1024, B) as ctx:
            membw_cache, membw_hbm = ctx.membw_probe(32 << 20), ctx.membw_probe(512 << 20, reps=5)
            common = dict(probe="resize", batch=B, membw_probe_cache_gbps=round(membw_cache, 1), membw_probe_hbm_gbps=round(membw_hbm, 1))
            for name, fname, (sw, sh), (dw, dh), interp, sky in CASES:
                fmt, dt, ch = FORMATS[fname]
                img = rng.integers(0, 256, (sh, sw, ch), dtype=np.uint8) if dt == np.uint8 else rng.normal(0, 3, (sh, sw, ch)).astype(np.float32)
                if sky:
                    img[: sh // 3] = (180, 130, 70)
                out_px = 1 if sky else img.dtype.itemsize * ch
                d_src, d_dst = ctx.alloc(B * img.nbytes), ctx.alloc(B * dw * dh * out_px)
                for b in range(B):
                    _lib.check(ctx.lib.mav_memcpy_h2d(ctx.h, d_src.ptr + b * img.nbytes, _lib._ptr(img), img.nbytes))
                if sky:
                    enqueue = lambda: ctx.sky_mask_enqueue(d_src, sw, sh, dw, dh, d_dst, batch=B)
                else:
                    enqueue = lambda: ctx.resize_enqueue(d_src, fmt, sw, sh, dw, dh, interp, B, d_dst)
                ms = timed(ctx, args.reps, enqueue)
                if B == 1 and args.host_reps > 0:
                    host_ms[name] = host_standin(img, (dw, dh), interp, args.host_reps)
                hs = host_ms.get(name)
                model = B * (img.nbytes + dw * dh * out_px)
                emit(dict(common, case=name, format=fname, src=[sw, sh], dst=[dw, dh], method=METHOD[interp] + (" + key" if sky else ""), ms=round(ms, 4),
                          model_mb=round(model / 1e6, 2), model_gbps=round(model / (ms * 1e-3) / 1e9, 1),
                          host_standin_ms_per_image=None if hs is None else round(hs, 2), host_standin="torch on the CPU: a stand-in, not cv2"))
                d_src.free(); d_dst.free()
            # the fused sky mask against the unfused resize of the same picture, in alternation
            sw, sh, dw, dh = 960, 512, 1920, 1024
            img = rng.integers(0, 256, (sh, sw, 3), dtype=np.uint8)
            d_src, d_pic, d_sky = ctx.alloc(B * img.nbytes), ctx.alloc(B * dw * dh * 3), ctx.alloc(B * dw * dh)
            for b in range(B):
                _lib.check(ctx.lib.mav_memcpy_h2d(ctx.h, d_src.ptr + b * img.nbytes, _lib._ptr(img), img.nbytes))
            unfused, fused = [], []
            for _ in range(args.rounds):
                unfused.append(timed(ctx, args.reps, lambda: ctx.resize_enqueue(d_src, warp.WARP_U8C3, sw, sh, dw, dh, resize.INTER_LINEAR, B, d_pic)))
                fused.append(timed(ctx, args.reps, lambda: ctx.sky_mask_enqueue(d_src, sw, sh, dw, dh, d_sky, batch=B)))
            spread = max(unfused) - min(unfused)
            emit(dict(common, case="fused sky mask against mav_resize_dev, in alternation", rounds=args.rounds, unfused_ms=[round(v, 4) for v in unfused],
                      fused_ms=[round(v, 4) for v in fused], unfused_median_ms=round(float(np.median(unfused)), 4), fused_median_ms=round(float(np.median(fused)), 4),
                      margin_ms_spread_of_unfused=round(spread, 4), fused_not_slower=bool(np.median(fused) <= np.median(unfused) + spread)))
            for b in (d_src, d_pic, d_sky):
                b.free()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
