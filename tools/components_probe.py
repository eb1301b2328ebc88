"""Cost of the connected components on the device, next to the only route the parent commit had.

    python tools/components_probe.py [--reps 50] [--out FILE]

Device-resident, HIP-event time (mav_timer_start / stop around ONE enqueue of mav_components_dev, synchronised), median of --reps, at
1280x720 and 1920x1080, batch 1 and batch 64, 8-connectivity, min_area 1, max_blobs 256, no label image, two masks:
  detect   the fixed mask of the synthetic detection scene (synth.make_batch -> mav_process_batch): a handful of blobs
  noise41  seeded noise at density 0.41, next to the 8-connectivity percolation threshold: thousands of ragged components
The passes move at least 29 bytes per pixel (tile pass 1 read + 8 written, flatten 4 + 4, count 4, rank 4, statistics 4; the root
chases, the per-root words and the atomics come on top and are not counted): passes_gbps = 29 B/px / time is therefore a LOWER bound
of what the passes reach, printed beside mav_membw_probe (a 3-read-1-write stream kernel) of the same run.  The per-class time is
the "components" class of mav_profile_get over one more enqueue (its events sit around the whole chain of a call).
Parent's route, same masks, batch 1, host clock, median of min(--reps, 5): download the mask (mav_memcpy_d2h) and
scipy.ndimage.label + find_objects + bincount areas and coordinate sums on the host; "not measured" when scipy is absent.
One JSON line per configuration."""
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

from mavflow import _lib, synth  # noqa: E402

BYTES_PER_PIXEL = 29


def median_ms(ctx, fn, reps):
    fn()
    ctx.sync()
    ts = []
    for _ in range(reps):
        ctx.timer_start()
        fn()
        ts.append(ctx.timer_stop())
    return float(np.median(ts))


def host_route_ms(buf, W, H, reps):
    try:
        import scipy.ndimage as ndi
    except ImportError:
        return "not measured"
    yy, xx = np.mgrid[0:H, 0:W]
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        mask = buf.download(np.uint8, (H, W))
        labels, n = ndi.label(mask, structure=np.ones((3, 3), int))
        ndi.find_objects(labels)
        flat = labels.ravel()
        np.bincount(flat, minlength=n + 1)
        np.bincount(flat, weights=xx.ravel(), minlength=n + 1)
        np.bincount(flat, weights=yy.ravel(), minlength=n + 1)
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    for (W, H) in ((1280, 720), (1920, 1080)):
        prev, nxt = synth.make_batch(W, H, 1, distinct=1)
        samples = np.stack([synth.foe_samples(W, H, 0)])
        masks = {"noise41": (np.random.default_rng(41).random((H, W)) < 0.41).astype(np.uint8)}
        with _lib.Context(W, H, 1) as c1:
            masks["detect"] = np.ascontiguousarray(c1.process_batch(prev, nxt, samples)["mask_fixed"][0]).view(np.uint8)
        for B in (1, 64):
            with _lib.Context(W, H, B) as ctx:
                membw = ctx.membw_probe(32 << 20)
                counts, table = ctx.alloc(B * 8), ctx.alloc(B * 256 * 40)
                for name in ("detect", "noise41"):
                    buf = ctx.alloc(B * W * H).upload(np.broadcast_to(masks[name], (B, H, W)))

                    def call():
                        ctx.components_dev(buf, B, counts, table)

                    ms = median_ms(ctx, call, args.reps)
                    ctx.profile_enable(1)
                    call()
                    ctx.sync()
                    prof = ctx.profile_get()
                    ctx.profile_enable(0)
                    got = counts.download(_lib.CC_COUNTS_DTYPE, (B,))
                    rec = dict(probe="components", W=W, H=H, batch=B, mask=name, n_components=int(got["n_components"][0]),
                               ms=round(ms, 4), ms_per_image=round(ms / B, 4), class_ms={k: round(v[0], 4) for k, v in prof.items() if v[1]},
                               passes_gbps_lower_bound=round(BYTES_PER_PIXEL * W * H * B / (ms * 1e-3) / 1e9, 1), membw_probe_gbps=round(membw, 1),
                               workspace_bytes=ctx.mem_info()["ctx_bytes"],
                               host_route_ms=host_route_ms(buf, W, H, min(args.reps, 5)) if B == 1 else "not measured")
                    if isinstance(rec["host_route_ms"], float):
                        rec["host_route_ms"] = round(rec["host_route_ms"], 3)
                    line = json.dumps(rec)
                    print(line, flush=True)
                    lines.append(line)
                    buf.free()
                counts.free()
                table.free()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
