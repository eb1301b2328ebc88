"""Cost of the threshold sweep on the device, next to the only route the parent commit had for the same answer.

    python tools/roc_probe.py [--reps 50] [--out FILE]

Device-resident, HIP-event time (mav_timer_start / stop around ONE enqueue, synchronised), median of --reps, at 1280x720 and 1920x1080,
batch 1 and batch 64, threshold grids 1x1, 22x7 and 64x16, two inputs:
  scene   the flow of the synthetic detection scene (synth.make_batch -> mav_process_batch), its FoE, the scene's fixed mask as the
          ground truth: most pixels lie below the smallest thresholds
  onebin  an exactly anti-radial field of 13 px and more: every pixel lands in the top bin of every grid (the histogram's worst case)
sweep_ms: mav_roc_sweep_dev (table fill, sweep kernel, suffix kernel).  route_ms: ONE threshold pair by the parent's route, enqueue only
as well: mav_detect_dev (the phi / mask stage with the single-precision screen, and in front of it the two FoE launches on 16 line
pairs, because no enqueue-only entry point takes a caller's FoE) + mav_tpr_fpr_counts_dev of the fixed mask; measured in the same
process in alternation with the sweep (one sweep, one route, one sweep, ...).  Those kernels are the parent's, untouched.  The parent
needs Ka * Km such runs: route_total_ms = Ka * Km * route_ms, and break_even = the smallest Ka * Km at which the sweep of THIS grid is
the cheaper one (sweep_ms / route_ms, rounded up).  sweep_gbps counts the 10 bytes per pixel the sweep has to read (flow 8, sky 1,
ground truth 1), beside mav_membw_probe (a 3-read-1-write stream kernel) of the same run.  One JSON line per configuration."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "mav-detection_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from mavflow import _lib, synth  # noqa: E402

ANG = [0.5, 1, 2, 3.5, 5, 7.5, 10, 12.5, 15, 17.5, 20, 25, 30, 40, 50, 60, 75, 89, 91, 120, 150, 179]
MAG = [0.25, 0.5, 0.75, 1, 1.5, 2, 3]
GRIDS = {"1x1": ([15.0], [1.0]), "22x7": (ANG, MAG), "64x16": (list(np.linspace(0.25, 179.75, 64)), list(np.linspace(0.125, 4.0, 16)))}
ROUTE_PAIRS = 16


def alternate_ms(ctx, fa, fb, reps):
    """medians of fa and fb, timed one after the other `reps` times"""
    fa(); fb()
    ctx.sync()
    ta, tb = [], []
    for _ in range(reps):
        for fn, ts in ((fa, ta), (fb, tb)):
            ctx.timer_start()
            fn()
            ts.append(ctx.timer_stop())
    return float(np.median(ta)), float(np.median(tb))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    for (W, H) in ((1280, 720), (1920, 1080)):
        prev, nxt = synth.make_batch(W, H, 1, distinct=1)
        samples = np.stack([synth.foe_samples(W, H, 0)])
        with _lib.Context(W, H, 1) as c1:
            out = c1.process_batch(prev, nxt, samples)
        foe = np.array(out["results"]["foe"][0], np.float64)
        ys, xs = np.mgrid[0:H, 0:W]
        far = np.array([-10.5, -7.25])
        inputs = {"scene": (np.ascontiguousarray(out["flow"][0]), foe, 255 * np.ascontiguousarray(out["mask_fixed"][0]).view(np.uint8)),
                  "onebin": (np.stack([-(xs - far[0]), -(ys - far[1])], axis=-1).astype(np.float32), far,
                             np.where((xs + ys) % 3 == 0, 255, 0).astype(np.uint8))}
        smp = np.ascontiguousarray(synth.foe_samples(W, H, 0, n_pairs=ROUTE_PAIRS))
        for B in (1, 64):
            with _lib.Context(W, H, B) as ctx:
                lib = ctx.lib
                membw = ctx.membw_probe(32 << 20)
                fp, tp = _lib.foe_defaults(), _lib.thr_defaults()
                fp.n_pairs = ROUTE_PAIRS
                mf, md, res, cf = ctx.alloc(B * W * H), ctx.alloc(B * W * H), ctx.alloc(B * 32), ctx.alloc(B * 32)
                d_smp = ctx.alloc(B * smp.nbytes).upload(np.broadcast_to(smp, (B,) + smp.shape))
                table = ctx.alloc(B * 8 * _lib.roc_table_words(64, 16))
                for name, (flow, fe, gt) in inputs.items():
                    d_flow = ctx.alloc(B * flow.nbytes).upload(np.broadcast_to(flow, (B,) + flow.shape))
                    d_foe = ctx.alloc(B * 16).upload(np.broadcast_to(fe, (B, 2)))
                    d_gt = ctx.alloc(B * W * H).upload(np.broadcast_to(gt, (B, H, W)))

                    def route():
                        _lib.check(lib.mav_detect_dev(ctx.h, d_flow.ptr, d_smp.ptr, None, None, None, None, B, C.byref(fp), C.byref(tp), None,
                                                      mf.ptr, md.ptr, res.ptr))
                        _lib.check(lib.mav_tpr_fpr_counts_dev(ctx.h, d_gt.ptr, B, mf.ptr, None, 255, B, cf.ptr, None))

                    for gname, (a, m) in GRIDS.items():
                        def sweep():
                            ctx.roc_sweep_dev(d_flow, d_foe, d_gt, B, B, a, m, table)

                        s_ms, r_ms = alternate_ms(ctx, sweep, route, args.reps)
                        cells = len(a) * len(m)
                        top = table.download(np.int64, (_lib.roc_table_words(len(a), len(m)),))
                        rec = dict(probe="roc_sweep", W=W, H=H, batch=B, input=name, grid=gname, cells=cells, sweep_ms=round(s_ms, 4),
                                   route_ms=round(r_ms, 4), route_total_ms=round(r_ms * cells, 3), speedup=round(r_ms * cells / s_ms, 1),
                                   break_even=int(math.ceil(s_ms / r_ms)), sweep_gbps=round(10.0 * W * H * B / (s_ms * 1e-3) / 1e9, 1),
                                   membw_probe_gbps=round(membw, 1), tp_first_cell=int(top[2]), tp_last_cell=int(top[-2]))
                        line = json.dumps(rec)
                        print(line, flush=True)
                        lines.append(line)
                    for b in (d_flow, d_foe, d_gt):
                        b.free()
                for b in (mf, md, res, cf, d_smp, table):
                    b.free()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
