"""Cost of the flow history on the device (mav_history_push_dev), next to the host chain the reference runs for the same answer.

    python tools/history_probe.py [--reps 50] [--host-reps 2] [--out FILE] [--lib OTHER_BUILD.so --tag NAME]

Device-resident, HIP-event time (mav_timer_start / stop around ONE enqueue, synchronised), median of --reps, at 1280x720 and 1920x1080,
ring of 20 fields, float32 and float64 ring (float32 fields in), after 2 L warm-up pushes (every slot holds a field) of a smooth seeded
field of about 2 px that changes from push to push.
  push_ms    one mav_history_push_dev: the ring write and the trajectory kernel
  put_ms / trace_ms   the two kernels separately: classes "history_put" / "history_trace" of mav_profile_get over --reps more pushes
             (HIP events around every launch), mean per launch
  model_gbps the bytes the trajectory kernel cannot avoid -- n_slots * 2 * sizeof(element) per pixel read (one tap's worth per step; the
             four taps of neighbouring pixels overlap) plus the output written -- over trace_ms: a LOWER bound of the traffic
  membw_*    mav_membw_probe (a 3-read-1-write stream kernel) of the same run, at a cache-resident (4 x 32 MB) and an HBM (4 x 512 MB) size
  ring_mb    the ring: beside the 256 MiB Infinity Cache (720p float32 fits, the others do not)
  host_standin_ms   the reference's function (detector.py:365-388) on the host at batch 1 with scipy.ndimage.map_coordinates(order=1,
             mode="grid-constant") STANDING IN for cv2.remap (cv2 is not installed), float64 ring as the reference's, best of
             --host-reps in the same process: what the reference's route costs, not a measurement of cv2
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

from mavflow import _lib  # noqa: E402

L = 20
N_FIELDS = 4


def field(W, H, i):
    rng = np.random.default_rng(7 + i)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    u = 2.0 * np.sin(xx / 170.0 + 0.3 * i) + 0.5 * np.cos(yy / 110.0)
    v = 1.5 * np.cos(yy / 130.0 - 0.2 * i) - 0.7 * np.sin(xx / 230.0)
    return (np.stack([u, v], axis=-1) + rng.normal(0, 0.05, (H, W, 2))).astype(np.float32)


def host_standin(fields, reps):
    """Detector.get_history with map_coordinates in cv2.remap's place; seconds of the best of `reps` calls after the ring is full."""
    import scipy.ndimage as ndi
    H, W = fields[0].shape[:2]
    ring = np.zeros((L, H, W, 2))
    for i in range(L):
        ring[i] = fields[i % N_FIELDS]
    y_coords, x_coords = np.mgrid[0:H, 0:W]
    best, index = None, 0
    for rep in range(reps):
        t0 = time.perf_counter()
        ring[index, ...] = fields[rep % N_FIELDS]
        k = (index + 1) % (L - 1)
        orig_map = np.zeros((H, W, 2))
        orig_map[..., 0], orig_map[..., 1] = y_coords, x_coords
        lookup_map = np.copy(orig_map)
        while k != index % (L - 1):
            warped = lookup_map.astype(np.float32)
            coords = [warped[..., 0], warped[..., 1]]
            step = np.stack([ndi.map_coordinates(ring[k, ..., ch], coords, order=1, mode="grid-constant", cval=0.0) for ch in range(2)], axis=-1)
            lookup_map += step
            k = (k + 1) % L
        index = (index + 1) % L
        _ = lookup_map - orig_map
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--lib", default=None, help="another build of libmavflow.so (an A/B build of kernels_history.hip with -DHIST_PX / -DHIST_CAP)")
    ap.add_argument("--tag", default=None, help="a label for the lines of this run")
    args = ap.parse_args()
    if args.lib:
        _lib.load(args.lib)
    lines = []
    for (W, H) in ((1280, 720), (1920, 1080)):
        fields = [field(W, H, i) for i in range(N_FIELDS)]
        host_ms = host_standin(fields, args.host_reps) * 1e3 if args.host_reps > 0 else None
        with _lib.Context(W, H, 1) as ctx:
            membw_cache, membw_hbm = ctx.membw_probe(32 << 20), ctx.membw_probe(512 << 20, reps=5)
            d_fields = [ctx.alloc(f.nbytes).upload(f) for f in fields]
            d_out = ctx.alloc(W * H * 16)
            for dtype in (np.float32, np.float64):
                es = np.dtype(dtype).itemsize
                hist = ctx.flow_history(L, dtype)
                for i in range(2 * L):
                    hist.push_enqueue(d_fields[i % N_FIELDS], d_out)
                ctx.sync()
                ts, steps = [], []
                for i in range(args.reps):
                    steps.append(len(_lib.history_schedule(L, hist.index)))
                    ctx.timer_start()
                    hist.push_enqueue(d_fields[i % N_FIELDS], d_out)
                    ts.append(ctx.timer_stop())
                ctx.profile_enable(1)
                for i in range(args.reps):
                    hist.push_enqueue(d_fields[i % N_FIELDS], d_out)
                ctx.sync()
                prof = ctx.profile_get()
                ctx.profile_enable(0)
                put_ms = prof["history_put"][0] / max(prof["history_put"][1], 1)
                trace_ms = prof["history_trace"][0] / max(prof["history_trace"][1], 1)
                n_slots = float(np.mean(steps))
                model = (n_slots * 2 * es + 16) * W * H
                acc = d_out.download(np.float64, (H, W, 2))
                rec = dict(probe="flow_history", **({"tag": args.tag} if args.tag else {}), W=W, H=H, length=L, ring=np.dtype(dtype).name, ring_mb=round(hist.ring_bytes / 1e6, 1),
                           pushes=hist.pushes, push_ms=round(float(np.median(ts)), 4), put_ms=round(put_ms, 4), trace_ms=round(trace_ms, 4),
                           n_slots=round(n_slots, 2), model_mb=round(model / 1e6, 1), model_gbps_lower_bound=round(model / (trace_ms * 1e-3) / 1e9, 1),
                           membw_probe_cache_gbps=round(membw_cache, 1), membw_probe_hbm_gbps=round(membw_hbm, 1),
                           host_standin_ms=None if host_ms is None else round(host_ms, 1),
                           speedup_vs_standin=None if host_ms is None else round(host_ms / float(np.median(ts)), 1),
                           acc_abs_mean_px=round(float(np.abs(acc).mean()), 3))
                line = json.dumps(rec)
                print(line, flush=True)
                lines.append(line)
                hist.close()
            for b in d_fields + [d_out]:
                b.free()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
