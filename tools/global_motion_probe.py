"""Cost of the global-motion branch on the device, next to the only route the parent commit had.

    python tools/global_motion_probe.py [--reps 50] [--out FILE] [--lib LIBMAVFLOW.so] [--loop [--frames 128]]

Device-resident, HIP-event time (mav_timer_start / stop around ONE enqueue, synchronised), median of --reps, at 1280x720 and
1920x1080, batch 1 and batch 64, 1000 pairs:
  fit            mav_flow_homography_dev       pair gather + the one-workgroup-per-item homography fit
  subtract_scan  mav_global_motion_dev         passes A and B, the pyramid, the level scans, the record (no optimize_window)
  step           mav_global_motion_step_dev    all of it in one enqueue
  batch_call     mav_global_motion_batch_dev   frames in, records out: Farneback + step in one enqueue (frames device-resident)
`subtract_scan` moves 17 B per pixel in its two passes (flow 8 B read twice, 1 B image written) plus the u8 pyramid and scans (under
2 B/px more, not counted): passes_gbps = 17 B/px / time is therefore a LOWER bound of what the two passes reach, printed beside
mav_membw_probe (a 3-read-1-write stream kernel) of the same run.
Parent's route, same job, host clock, median of min(--reps, 10): the numpy restatement of detector.py:164-185 on the host
(global_motion, subtraction, magnitude, argmax, to_rgb's channel) plus mav_analyze_pyramid on the resulting image, batch 1 only --
the flow is on the host already (its download from the device is not charged).  One JSON line per configuration.

--lib: another build of the same ABI (csrc/build_diag/, never inside the package), loaded before anything else -- an A/B of two
builds is this tool run on each in alternation in one job; every line names the library it measured.
--loop: instead of the enqueues, Processor(algorithm=HOMOGRAPHY) end to end on SyntheticDataset (frames -> Farneback -> the branch;
distinct = 4 pictures, --frames frame indices) at the same two sizes, host clock, the second of two runs over the same processor:
frames per second of run_detection() and of run_detection_batched(64)."""
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


def median_ms(ctx, fn, reps):
    fn()
    ctx.sync()
    ts = []
    for _ in range(reps):
        ctx.timer_start()
        fn()
        ts.append(ctx.timer_stop())
    return float(np.median(ts))


def host_route_ms(ctx, flow, M, reps):
    H, W = flow.shape[:2]
    x_coords = np.tile(np.arange(W), (H, 1))
    y_coords = np.tile(np.arange(H), (W, 1)).T
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        gm = np.zeros_like(flow)
        gm[..., 0] = M[0, 0] * x_coords + M[0, 1] * y_coords + M[0, 2] - x_coords
        gm[..., 1] = M[1, 0] * x_coords + M[1, 1] * y_coords + M[1, 2] - y_coords
        warped = gm - flow
        mag = np.sqrt(warped[..., 0] ** 2.0 + warped[..., 1] ** 2.0)
        np.unravel_index(mag.argmax(), mag.shape)
        gray = np.around(np.abs(mag) * 255 / np.max(mag)).astype(np.uint8)
        ctx.analyze_pyramid(gray)
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def probe(W, H, B, reps, n_pairs=1000):
    rng = np.random.default_rng(W + B)
    flow1 = synth.synthetic_flow(W, H, seed=1).astype(np.float32)
    flow1[H // 3:H // 3 + 40, W // 2:W // 2 + 40] += np.float32(6.0)
    coords = np.c_[rng.integers(20, W - 20, n_pairs), rng.integers(20, H - 20, n_pairs)].astype(np.int32)
    with _lib.Context(W, H, B) as ctx:
        flow = ctx.alloc(flow1.nbytes * B)
        for b in range(B):
            _lib.check(ctx.lib.mav_memcpy_h2d(ctx.h, flow.ptr + b * flow1.nbytes, _lib._ptr(flow1), flow1.nbytes))
        Hd, ok, res, gray = ctx.alloc(72 * B), ctx.alloc(4 * B), ctx.alloc(_lib.MOTION_DTYPE.itemsize * B), ctx.alloc(W * H * B)
        lib, h = ctx.lib, ctx.h
        cp = _lib._ptr(coords)

        def fit():
            _lib.check(lib.mav_flow_homography_dev(h, flow.ptr, cp, n_pairs, B, Hd.ptr, ok.ptr))

        def sub():
            _lib.check(lib.mav_global_motion_dev(h, flow.ptr, Hd.ptr, B, 1.5, 0, None, None, gray.ptr, res.ptr))

        def step():
            _lib.check(lib.mav_global_motion_step_dev(h, flow.ptr, cp, n_pairs, B, 1.5, 0, Hd.ptr, ok.ptr, gray.ptr, res.ptr))

        t_fit = median_ms(ctx, fit, reps)
        assert ok.download(np.int32, (B,)).all()
        M9 = Hd.download(np.float64, (B, 9))
        M6 = ctx.alloc(48 * B).upload(np.ascontiguousarray(M9[:, :6]))

        def sub6():
            _lib.check(lib.mav_global_motion_dev(h, flow.ptr, M6.ptr, B, 1.5, 0, None, None, gray.ptr, res.ptr))

        t_sub = median_ms(ctx, sub6, reps)
        t_step = median_ms(ctx, step, reps)
        prev, nxt = synth.make_batch(W, H, B, distinct=min(B, 4))
        dp, dn = ctx.alloc(prev.nbytes).upload(prev), ctx.alloc(nxt.nbytes).upload(nxt)

        def batch_call():
            ctx.global_motion_batch_dev(dp.ptr, dn.ptr, coords, B, res.ptr, H_ptr=Hd.ptr, ok_ptr=ok.ptr, gray_ptr=gray.ptr)

        t_batch = median_ms(ctx, batch_call, reps)
        line = dict(W=W, H=H, batch=B, pairs=n_pairs, reps=reps, fit_ms=round(t_fit, 4), subtract_scan_ms=round(t_sub, 4), step_ms=round(t_step, 4),
                    batch_call_ms=round(t_batch, 4),
                    passes_gbps_lower_bound=round(17.0 * W * H * B / (t_sub * 1e-3) / 1e9, 1),
                    membw_probe_gbps=round(ctx.membw_probe(min(256 << 20, max(1 << 20, 8 * W * H * B))), 1))
        if B == 1:
            line["parent_route_host_ms"] = round(host_route_ms(ctx, flow1, M9[0].reshape(3, 3), min(reps, 10)), 3)
            line["step_beats_parent_route"] = bool(t_step < line["parent_route_host_ms"])
        for buf in (flow, Hd, ok, res, gray, M6, dp, dn):
            buf.free()
    return line


def loop_probe(W, H, frames, batch=64):
    import logging
    from mavflow.detector import Detector
    from mavflow.processor import Processor, SyntheticDataset
    from mavflow.run_config import RunConfig
    line = dict(W=W, H=H, frames=frames, batch=batch)
    for name in ("run_detection", "run_detection_batched"):
        np.random.seed(1)
        ds = SyntheticDataset(W=W, H=H, N=frames + 1, use_farneback=True, distinct=4)
        p = Processor(RunConfig(logging.getLogger("probe"), ds, "", False, False, False, True, False, False, "FLOW_FOE_CLUSTERING"),
                      algorithm=Detector.Algorithm.HOMOGRAPHY)
        run = p.run_detection if name == "run_detection" else (lambda: p.run_detection_batched(batch))
        try:
            for _ in range(2):                           # the first run creates contexts and buffers and draws the pictures
                p.frame_index = 0
                t0 = time.perf_counter()
                run()
                dt = time.perf_counter() - t0
            assert len(p.detection_windows) == frames
            line[name + "_fps"] = round(frames / dt, 1)
        finally:
            p.release()
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--lib", default=None)
    ap.add_argument("--loop", action="store_true")
    ap.add_argument("--frames", type=int, default=128)
    a = ap.parse_args()
    name = os.path.basename(_lib.load(a.lib)._name)
    sizes = ((1280, 720), (1920, 1080))
    if a.loop:
        lines = [json.dumps(dict(lib=name, **loop_probe(W, H, a.frames))) for (W, H) in sizes]
    else:
        lines = [json.dumps(dict(lib=name, **probe(W, H, B, a.reps))) for (W, H) in sizes for B in (1, 64)]
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a" if a.lib else "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
