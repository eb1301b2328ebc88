"""Cost of k-means on the device (mav_kmeans_dev) next to a host stand-in.

    python tools/kmeans_probe.py [--reps 50] [--sizes 1280x720,1920x1080] [--batches 1,16] [--out FILE]

Device-resident inputs, HIP-event time (mav_timer_start / stop around ONE enqueue, synchronised), median of --reps after 5 warm-up
enqueues, at 1280x720 and 1920x1080, batch 1 and 16.  The samples come from a synthetic global-motion scene (an affine camera motion, noise
and one patch that moves on its own, through Context.global_motion):
  mag3   the reference's shape (src/detector.py:396-428): the residual magnitude's values three at a time, float32, D = 3, K = 8, 10 attempts
  gray1  the grey image of the same residual, uint8, D = 1, K = 8, 10 attempts
Initial centres: clustering.random_centers, seed 1.  Per row:
  ms                       the whole call
  iterations, repairs      of the record (the best attempt's assignments; samples moved into empty clusters, all attempts)
  launches, left_on_flag   the call's launch count and how many of them left at once for an image (record.skipped)
  gdist_per_s              float32 distances per second: batch * N * K * (assignments over all attempts + the final pass) / ms
  membw_*                  mav_membw_probe of the same run, at a cache-resident (4 x 32 MB) and an HBM (4 x 512 MB) size
  standin_ms               in the same process: tests/kmeans_ref.py's numpy restatement on ONE image, times the batch.  A STAND-IN for the host
                           route, not cv2 (there is no cv2 here)
  equals_standin           labels, centres and counts of image 0 against the stand-in's (uint8 rows: the sums are exact; float32 rows may part
                           where a float64 sum's last bit decides)
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

import kmeans_ref as R  # noqa: E402
from mavflow import _lib, clustering  # noqa: E402

WARM = 5
K, A, MAX_ITER, EPS = 8, 10, 10, 1.0


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


def scene(ctx, W, H, seed):
    """(mag float32 (H, W), gray uint8 (H, W)) of a synthetic global-motion frame"""
    rng = np.random.default_rng(seed)
    M = np.array([[1.004, 0.003, -1.25], [-0.002, 0.997, 0.75]])
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    flow = np.stack([M[0, 0] * xs + M[0, 1] * ys + M[0, 2] - xs, M[1, 0] * xs + M[1, 1] * ys + M[1, 2] - ys], axis=-1)
    flow += rng.normal(0, 0.15, flow.shape)
    flow[H // 3:H // 3 + 24, W // 2:W // 2 + 24] += (3.0, -2.0)
    out = ctx.global_motion(flow.astype(np.float32), M, outputs=("mag", "gray"))
    return out["mag"][0], out["gray"][0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--sizes", default="1280x720,1920x1080")
    ap.add_argument("--batches", default="1,16")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    for size in args.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        with _lib.Context(W, H, 1) as c0:
            mag, gray = scene(c0, W, H, W)
        for form, x in (("mag3", np.ascontiguousarray(mag.reshape(-1, 3))), ("gray1", np.ascontiguousarray(gray.reshape(-1, 1)))):
            N, D = x.shape
            init = clustering.random_centers(x, K, A, rng=1)
            t0 = time.perf_counter()
            ref = R.kmeans(x, init, MAX_ITER, EPS)
            standin = (time.perf_counter() - t0) * 1e3
            passes = sum(q["iterations"] for q in ref["attempts"]) + A
            for B in (int(v) for v in args.batches.split(",")):
                with _lib.Context(W, H, B) as ctx:
                    membw_cache, membw_hbm = ctx.membw_probe(32 << 20), ctx.membw_probe(512 << 20, reps=5)
                    rep = lambda a: np.ascontiguousarray(np.broadcast_to(a, (B,) + a.shape))
                    need = ctx.kmeans_workspace_bytes(N, B, K, A, D, x.dtype)
                    d_x, d_init = ctx.alloc(x.nbytes * B).upload(rep(x)), ctx.alloc(init.nbytes * B).upload(rep(init))
                    d_lab, d_cen, d_rec, d_ws = ctx.alloc(4 * N * B), ctx.alloc(4 * K * D * B), ctx.alloc(96 * B), ctx.alloc(need)
                    call = lambda: ctx.kmeans_enqueue(d_x, N, B, d_init, d_lab, d_cen, d_rec, d_ws, need, K=K, attempts=A, max_iter=MAX_ITER, eps=EPS,
                                                      dims=D, dtype=x.dtype)
                    ms = timed(ctx, call, args.reps)
                    rec = d_rec.download(clustering.RECORD_DTYPE, (B,))
                    lab, cen = d_lab.download(np.int32, (B, N)), d_cen.download(np.float32, (B, K, D))
                    same = bool(np.array_equal(lab[0], ref["labels"]) and cen[0].tobytes() == ref["centers"].tobytes()
                                and np.array_equal(rec[0]["counts"], ref["counts"]))
                    lines.append(dict(probe="kmeans", form=form, W=W, H=H, N=N, D=D, dtype=str(x.dtype), K=K, attempts=A, batch=B, ms=round(ms, 4),
                                      iterations=int(rec[0]["iterations"]), repairs=int(rec[0]["repairs"]), best_attempt=int(rec[0]["best_attempt"]),
                                      launches=1 + (MAX_ITER - 1) * (3 + 2 * (K - 1)) + 3, left_on_flag=int(rec[0]["skipped"]),
                                      gdist_per_s=round(B * N * K * passes / (ms * 1e-3) / 1e9, 1), workspace_mb=round(need / 1e6, 1),
                                      membw_cache_gbps=round(membw_cache, 1), membw_hbm_gbps=round(membw_hbm, 1),
                                      standin="tests/kmeans_ref.py (numpy), not cv2", standin_ms=round(standin * B, 1),
                                      device_faster_by=round(standin * B / ms, 1), not_slower=bool(ms <= standin * B), equals_standin=same,
                                      all_images_same_bytes=bool(all(rec[b].tobytes() == rec[0].tobytes() and np.array_equal(lab[b], lab[0]) for b in range(B)))))
                    print(json.dumps(lines[-1]), flush=True)
                    for b in (d_x, d_init, d_lab, d_cen, d_rec, d_ws):
                        b.free()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(json.dumps(x) for x in lines) + "\n")


if __name__ == "__main__":
    main()
