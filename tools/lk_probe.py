"""Cost of the sparse optical-flow path per frame of a device-resident video.

    python tools/lk_probe.py [--frames 50] [--warmup 8] [--sizes 1280x720,1920x1080]

Per size: a synthetic zoom sequence (synth.make_sequence) is uploaded once; every frame then does what LucasKanade.get_features does on
the device -- corner detection on the resident frame (mav_good_features_dev(NULL): eigenvalue map, threshold, non-maximum test,
compaction, sort and greedy pick on the device, the corners brought back), then one mav_lk_track_dev from the resident frame to the
next one (the new frame's pyramid, the previous frame's Scharr pairs, the tracker).  Reported per frame, median over the timed frames:
  corners_dev_ms   HIP-event time of the class "lk_corners"            corners_host_ms  wall time of the call minus that
  pick_ms          class "lk_pick" (sort + pick; inside corners_host_ms: corners_dev_ms + corners_host_ms is the call's wall time)
  pyramid_ms       class "lk_pyramid" (pyrDown chain + Scharr)          track_ms         class "lk_track"
  pick_chunks, pick_rounds  what the pick did (mav_gftt_last_pick)
  get_features_ms  wall time of detector.LucasKanade.get_features on host BGR frames (gray conversion, uploads and downloads included)
  chain_ms         wall time per frame of the enqueue-only chain, in a pass of its own without profiling: good_features_enqueue(None)
                   then lk_track_enqueue reading the count on the device, one sync() per frame
and the histogram of tracker iterations per (point, level) over all timed frames.  Prints one JSON line.

    python tools/lk_probe.py --track [--points 2000] [--reps 30] [--rounds 3] [--sizes 1280x720,1920x1080]

The tracker kernel alone, with and without cv2's `err`: one context per size in ONE process, the sizes taken in alternation `rounds`
times, `reps` calls per visit and form on one frame pair with `points` points (the pair's corners, filled up with random points).
Per form the HIP-event time of the class "lk_track" per call, median and minimum over all visits:
  plain     mav_lk_track_dev                                  err_null  mav_lk_track_err_dev, flags 0, no err buffer
  err       mav_lk_track_err_dev with an err buffer           min_eig   the same with OPTFLOW_LK_GET_MIN_EIGENVALS
A library without the err form (an older build the script is pointed at) reports `plain` alone.  Prints one JSON line."""
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
from mavflow.detector import LucasKanade  # noqa: E402


def probe(W: int, H: int, frames: int, warmup: int) -> dict:
    n = frames + warmup + 1
    seq = synth.make_sequence(W, H, n, seed=0)
    rows = {k: [] for k in ("corners_dev_ms", "corners_host_ms", "pick_ms", "pyramid_ms", "track_ms", "pick_chunks", "pick_rounds",
                           "candidates_points")}
    hist = np.zeros(_lib.LK_HIST_BINS, np.int64)
    with _lib.Context(W, H, 1) as c:
        dev = [c.alloc(W * H).upload(f) for f in seq]
        d_pts, d_out, d_status = c.alloc(_lib.LK_MAX_POINTS * 8), c.alloc(_lib.LK_MAX_POINTS * 8), c.alloc(_lib.LK_MAX_POINTS)
        pts = c.good_features_dev(dev[0].ptr)
        c.profile_enable(1)
        last = {k: 0.0 for k in ("lk_corners", "lk_pick", "lk_pyramid", "lk_track")}
        for i in range(1, n):
            t0 = time.perf_counter()
            corners = c.good_features_dev(None)
            wall = (time.perf_counter() - t0) * 1e3
            chunks, rounds = c.gftt_last_pick()
            d_pts.upload(corners)
            c.lk_track_dev(None, dev[i].ptr, d_pts.ptr, len(corners), d_out.ptr, d_status.ptr)
            c.sync()
            prof = c.profile_get()
            step = {k: prof[k][0] - last[k] for k in last}
            last = {k: prof[k][0] for k in last}
            if i > warmup:
                rows["corners_dev_ms"].append(step["lk_corners"])
                rows["corners_host_ms"].append(wall - step["lk_corners"])
                rows["pick_ms"].append(step["lk_pick"])
                rows["pick_chunks"].append(chunks)
                rows["pick_rounds"].append(rounds)
                rows["pyramid_ms"].append(step["lk_pyramid"])
                rows["track_ms"].append(step["lk_track"])
                rows["candidates_points"].append(len(corners))
                hist += c.lk_last_iterations()
        c.profile_enable(0)
        # the enqueue-only chain: the corner count never leaves the device
        mc = _lib.gftt_defaults().max_corners
        d_count = c.alloc(4)
        c.good_features_dev(dev[0].ptr)
        chain = []
        for i in range(1, n):
            t0 = time.perf_counter()
            c.good_features_enqueue(None, d_pts.ptr, d_count.ptr)
            c.lk_track_enqueue(None, dev[i].ptr, d_pts.ptr, mc, d_count.ptr, d_out.ptr, d_status.ptr)
            c.sync()
            if i > warmup:
                chain.append((time.perf_counter() - t0) * 1e3)
    # the Python class on host frames
    bgr = [np.repeat(f[..., None], 3, axis=2) for f in seq]
    lk = LucasKanade(bgr[0])
    wall = []
    for i in range(1, n):
        t0 = time.perf_counter()
        lk.get_features(bgr[i])
        if i > warmup:
            wall.append((time.perf_counter() - t0) * 1e3)
    out = dict(W=W, H=H, frames=frames, points_median=int(np.median(rows.pop("candidates_points"))))
    out.update({k: round(float(np.median(v)), 4) for k, v in rows.items()})
    out["get_features_ms"] = round(float(np.median(wall)), 4)
    out["chain_ms"] = round(float(np.median(chain)), 4)
    nz = np.nonzero(hist)[0]
    out["iterations_mean"] = round(float((hist * np.arange(len(hist))).sum() / max(hist.sum(), 1)), 3)
    out["iterations_hist"] = {int(i): int(hist[i]) for i in nz}
    return out


def track_probe(sizes, points: int, reps: int, rounds: int) -> list:
    has_err = hasattr(_lib.Context, "lk_track_err_enqueue")
    forms = ["plain"] + (["err_null", "err", "min_eig"] if has_err else [])
    state = []
    for W, H in sizes:
        f0, f1 = synth.make_sequence(W, H, 2, seed=0)
        c = _lib.Context(W, H, 1)
        d0, d1 = c.alloc(W * H).upload(f0), c.alloc(W * H).upload(f1)
        pts = c.good_features(f0, max_corners=points)
        fill = (np.random.default_rng(5).random((points - len(pts), 2)) * (W - 1, H - 1)).astype(np.float32)
        pts = np.concatenate([pts, fill])
        d_pts, d_out, d_status, d_err = c.alloc(points * 8).upload(pts), c.alloc(points * 8), c.alloc(points), c.alloc(points * 4)
        c.profile_enable(1)
        state.append(dict(W=W, H=H, c=c, d0=d0, d1=d1, bufs=(d_pts, d_out, d_status, d_err), corners=int(points - len(fill)),
                          ms={f: [] for f in forms}))

    def call(st, form):
        c, (d_pts, d_out, d_status, d_err) = st["c"], st["bufs"]
        if form == "plain":
            c.lk_track_dev(st["d0"].ptr, st["d1"].ptr, d_pts.ptr, points, d_out.ptr, d_status.ptr)
        else:
            c.lk_track_err_enqueue(st["d0"].ptr, st["d1"].ptr, d_pts.ptr, points, None, d_out.ptr, d_status.ptr,
                                   None if form == "err_null" else d_err.ptr, flags=8 if form == "min_eig" else 0)
        c.sync()

    for r in range(rounds + 1):                               # round 0 warms up
        for st in state:
            for form in forms:
                for i in range(reps):
                    before = st["c"].profile_get()["lk_track"][0]
                    call(st, form)
                    if r:
                        st["ms"][form].append(st["c"].profile_get()["lk_track"][0] - before)
    res = []
    for st in state:
        row = dict(W=st["W"], H=st["H"], points=points, corners=st["corners"], calls=rounds * reps)
        for f in forms:
            row[f + "_ms"] = round(float(np.median(st["ms"][f])), 4)
            row[f + "_min_ms"] = round(float(np.min(st["ms"][f])), 4)
        res.append(row)
        st["c"].close()
    return res


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--sizes", default="1280x720,1920x1080")
    ap.add_argument("--track", action="store_true", help="the tracker kernel with and without err (see the module text)")
    ap.add_argument("--points", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if a.track:
        sizes = [tuple(int(v) for v in s.split("x")) for s in a.sizes.split(",")]
        print(json.dumps(dict(tool="lk_probe", mode="track", results=track_probe(sizes, a.points, a.reps, a.rounds))))
        return
    res = [probe(*(int(v) for v in s.split("x")), a.frames, a.warmup) for s in a.sizes.split(",")]
    print(json.dumps(dict(tool="lk_probe", results=res)))


if __name__ == "__main__":
    main()
