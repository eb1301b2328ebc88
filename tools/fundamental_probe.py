"""Cost of the robust fundamental-matrix fit and the dense epipolar residual on the device (mav_find_fundamental_dev,
mav_flow_fundamental_dev, mav_epipolar_residual_dev) next to the affine fit and a host stand-in.

    python tools/fundamental_probe.py [--reps 50] [--sizes 1280x720,1920x1080] [--batches 1,16] [--out FILE]

Device-resident inputs, HIP-event time (mav_timer_start / stop around ONE enqueue, synchronised), median of --reps after 5 warm-up
enqueues; n = 1000 pairs, max_iters = 1000, subsets from fundamental.sample_subsets(seed 1).  The scene per frame size: float32 fields of
a static scene with smoothly varying depth under a small camera motion with a forward component, noise of sigma 0.05, one 24 x 24 patch
that moves on its own, and 30 % of the sampled pixels carrying a gross vector of their own.
Per row:
  form = pairs   mav_find_fundamental_dev on resident pairs
  form = flow    mav_flow_fundamental_dev, coords from the host with the call
  form = dense   mav_epipolar_residual_dev with both outputs, F where the fit left it; gbps = (8 + 4 + 1) bytes per pixel over the time
  ms             the whole enqueue
  parts_ms       the call's launches in order (flow: gather first; fit: models, score, choose, finish; dense: its three launches as one
                 interval) from the library's own profile (mav_profile_intervals), median of 10 profiled calls
  affine_ms      mav_estimate_affine_dev (n = 1000, max_iters = 2000) on the same pairs, alternating with the enqueue in the same
                 process: for scale, no ratio is demanded
  standin_ms     in the same process: tests/fundamental_ref.py's restatement on ONE item, times the batch.  A STAND-IN for the host route,
                 not cv2 (there is no cv2 here)
  equals_standin F, mask and record (dense: map, mask and record) of item 0 against the stand-in's bytes
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

import fundamental_cases as T  # noqa: E402
import fundamental_ref as R  # noqa: E402
from mavflow import _lib, affine, fundamental  # noqa: E402

WARM, N, ITERS, AFF_ITERS, PROFILED = 5, 1000, 1000, 2000, 10


def scene(W, H, B, seed):
    rng = np.random.default_rng(seed)
    K = np.array([[0.8 * W, 0.0, (W - 1) / 2], [0.0, 0.8 * W, (H - 1) / 2], [0.0, 0.0, 1.0]])
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    flow = np.empty((B, H, W, 2), np.float32)
    coords = np.column_stack([rng.integers(20, W - 20, N), rng.integers(20, H - 20, N)]).astype(np.int32)
    Ki = np.linalg.inv(K)
    rays = Ki @ np.stack([xs.ravel(), ys.ravel(), np.ones(W * H)])
    for b in range(B):
        Rm, t = T.pose(b % 4)
        depth = 8.0 + 3.0 * np.sin(xs / 90.0 + b) + 2.0 * np.cos(ys / 70.0)
        Q = K @ (Rm @ (rays * depth.ravel()) + 0.2 * t[:, None])
        f = np.stack([(Q[0] / Q[2]).reshape(H, W) - xs, (Q[1] / Q[2]).reshape(H, W) - ys], axis=-1)
        f += rng.normal(0, 0.05, f.shape)
        f[H // 3:H // 3 + 24, W // 2:W // 2 + 24] += (-3.0, 6.0)
        bad = rng.permutation(N)[:int(N * 0.3)]
        f[coords[bad, 1], coords[bad, 0]] += rng.uniform(-40, 40, (len(bad), 2))
        flow[b] = f
    return flow, coords


def alternating(ctx, calls, reps):
    """median ms of each enqueue, the calls taking turns"""
    for _ in range(WARM):
        for call in calls:
            call()
    ctx.sync()
    ts = [[] for _ in calls]
    for _ in range(reps):
        for k, call in enumerate(calls):
            ctx.timer_start()
            call()
            ts[k].append(ctx.timer_stop())
    return [float(np.median(t)) for t in ts]


def per_launch(ctx, call, launches):
    """median ms of the call's launches, in order, from the library's profile"""
    ctx.sync()
    ctx.profile_enable(1)
    for _ in range(PROFILED):
        call()
    ctx.sync()
    _, _, t0, t1 = ctx.profile_intervals()
    ctx.profile_enable(0)
    d = (t1 - t0)[-PROFILED * launches:].reshape(PROFILED, launches)
    return [round(float(v), 4) for v in np.median(d, axis=0)]


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
        for B in (int(v) for v in args.batches.split(",")):
            flow, coords = scene(W, H, B, W + B)
            sub = fundamental.sample_subsets(1, N, ITERS, B)
            tri = affine.sample_triples(1, N, AFF_ITERS, B)
            src, dst = R.flow_pairs(flow, coords)
            t0 = time.perf_counter()
            ref = R.find_one(src[0], dst[0], sub[0], threshold=1.0)
            standin = (time.perf_counter() - t0) * 1e3 * B
            t0 = time.perf_counter()
            ref_epi = R.epipolar_residual(flow[:1], ref["F"][None], 1.0)
            standin_epi = (time.perf_counter() - t0) * 1e3 * B
            with _lib.Context(W, H, B) as ctx:
                need = ctx.find_fundamental_workspace_bytes(N, B, ITERS)
                aneed = ctx.estimate_affine_workspace_bytes(N, B, AFF_ITERS)
                bufs = [ctx.alloc(flow.nbytes).upload(flow), ctx.alloc(src.nbytes).upload(src), ctx.alloc(dst.nbytes).upload(dst),
                        ctx.alloc(sub.nbytes).upload(sub), ctx.alloc(72 * B), ctx.alloc(N * B), ctx.alloc(32 * B), ctx.alloc(need),
                        ctx.alloc(tri.nbytes).upload(tri), ctx.alloc(48 * B), ctx.alloc(aneed), ctx.alloc(4 * B * W * H), ctx.alloc(B * W * H),
                        ctx.alloc(32 * B)]
                df, ds, dd, dt, dF, di, dr, dw, dtri, dM, daw, dres, dmask, derec = bufs
                aff = lambda: ctx.estimate_affine_enqueue(ds, dd, N, B, dtri, dM, di, dr, daw, aneed)
                forms = {
                    "pairs": (lambda: ctx.find_fundamental_enqueue(ds, dd, N, B, dt, dF, di, dr, dw, need, threshold=1.0, max_iters=ITERS), 4),
                    "flow": (lambda: ctx.flow_fundamental_enqueue(df, coords, B, dt, dF, di, dr, dw, need, threshold=1.0, max_iters=ITERS), 5),
                    "dense": (lambda: ctx.epipolar_residual_enqueue(df, dF, B, dres, dmask, derec, threshold=1.0), 1),
                }
                for form, (call, launches) in forms.items():
                    ms, aff_ms = alternating(ctx, (call, aff), args.reps)
                    call()
                    parts = per_launch(ctx, call, launches)
                    row = dict(probe="fundamental", form=form, W=W, H=H, n=N, max_iters=ITERS, batch=B, ms=round(ms, 4), parts_ms=parts,
                               affine_ms=round(aff_ms, 4), standin="tests/fundamental_ref.py (numpy), not cv2")
                    if form == "dense":
                        erec = derec.download(fundamental.EPI_DTYPE, (B,))
                        same = bool(dres.download(np.float32, (B, H, W))[0].tobytes() == ref_epi["residual"][0].tobytes()
                                    and dmask.download(np.uint8, (B, H, W))[0].tobytes() == ref_epi["mask"][0].tobytes()
                                    and erec[0].tobytes() == ref_epi["records"][0].tobytes())
                        row.update(gbps=round(13.0 * W * H * B / ms / 1e6, 1), movers=int(erec[0]["movers"]), max_residual=float(erec[0]["max_residual"]),
                                   standin_ms=round(standin_epi, 1), device_faster_by=round(standin_epi / ms, 1), equals_standin=same)
                    else:
                        rec = dr.download(fundamental.RECORD_DTYPE, (B,))
                        same = bool(dF.download(np.float64, (B, 3, 3))[0].tobytes() == ref["F"].tobytes() and rec[0].tobytes() == ref["record"].tobytes()
                                    and np.array_equal(di.download(np.uint8, (B, N))[0], ref["inliers"]))
                        row.update(iters_run=int(rec[0]["iters_run"]), inliers=int(rec[0]["inliers"]), valid=int(rec[0]["valid"]),
                                   workspace_kb=round(need / 1e3, 1), standin_ms=round(standin, 1), device_faster_by=round(standin / ms, 1),
                                   equals_standin=same)
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
