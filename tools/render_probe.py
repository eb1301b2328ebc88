"""Cost of the result images (mav_render_dev) and of writing them as PNG files.

    python tools/render_probe.py [--reps 20] [--png-frames 48]

Device: HIP-event time of one mav_render_dev call with all three images, at 1920x1080 x 64 pairs and 1280x720 x 1, on a synthetic
float32 flow with rotation, a sky mask and a frame-0 pair.  The kernels move 26 B per pixel: the flow twice (8 B each: the max |flow|
reduction, then the render), the sky once (1 B) and three 3-byte images; 18 B/px is the floor of a single pass.  Both are reported as
a fraction of 8 TB/s.  Host: PNG files per second for three 1080p images per frame, encoded by 16 threads (frame_source.imwrite).
Prints one JSON line."""
from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "mav-detection_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from mavflow import _lib, frame_source, synth  # noqa: E402

PEAK_BPS = 8e12


def device_time(W: int, H: int, B: int, reps: int):
    flow1 = synth.synthetic_flow(W, H, seed=1)
    flow = np.ascontiguousarray(np.broadcast_to(flow1, (B, H, W, 2)))
    rng = np.random.default_rng(0)
    foe = np.stack([rng.uniform(0.3 * W, 0.7 * W, B), rng.uniform(0.3 * H, 0.7 * H, B)], axis=1)
    omega = rng.normal(0.0, 0.02, (B, 3))
    dt = np.full(B, 1 / 30.0)
    frame0 = np.zeros(B, np.uint8)
    frame0[0] = 1
    sky = np.zeros((B, H, W), np.uint8)
    sky[:, : H // 8] = 1
    with _lib.Context(W, H, B) as c:
        d = {k: c.alloc(a.nbytes).upload(np.ascontiguousarray(a)) for k, a in
             dict(flow=flow, foe=foe, omega=omega, dt=dt, frame0=frame0, sky=sky).items()}
        imgs = [c.alloc(B * H * W * 3) for _ in range(3)]

        def run():
            c.render_dev(d["flow"].ptr, d["foe"].ptr, B, *(x.ptr for x in imgs), omega_ptr=d["omega"].ptr, dt_ptr=d["dt"].ptr,
                         frame0_ptr=d["frame0"].ptr, sky_ptr=d["sky"].ptr)
        run(); run()
        c.sync()
        ms = []
        for _ in range(reps):
            c.timer_start()
            run()
            ms.append(c.timer_stop())
        sample = {k: x.download(np.uint8, (1, H, W, 3))[0] for k, x in zip(("result", "flow", "phi"), imgs)}
    ms = np.array(ms)
    px = W * H * B
    med = float(np.median(ms))
    return dict(W=W, H=H, B=B, ms_median=med, ms_min=float(ms.min()), ms_max=float(ms.max()),
                frac_peak_actual_26Bpx=26 * px / (med * 1e-3) / PEAK_BPS, frac_peak_floor_18Bpx=18 * px / (med * 1e-3) / PEAK_BPS), sample


def png_rate(sample: dict, frames: int, workers: int = 16):
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(max_workers=workers) as pool:
        t0 = time.perf_counter()
        jobs = [pool.submit(frame_source.imwrite, os.path.join(tmp, f"{k}_{i:05d}.png"), img)
                for i in range(frames) for k, img in sample.items()]
        for j in jobs:
            j.result()
        dt = time.perf_counter() - t0
        size = sum(os.path.getsize(os.path.join(tmp, f)) for f in os.listdir(tmp)) / frames
    return dict(workers=workers, frames=frames, frames_per_s=frames / dt, mbytes_per_frame=size / 1e6)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--png-frames", type=int, default=48)
    a = ap.parse_args()
    big, sample = device_time(1920, 1080, 64, a.reps)
    small, _ = device_time(1280, 720, 1, a.reps)
    out = dict(render_1080p_x64=big, render_720p_x1=small, png_1080p=png_rate(sample, a.png_frames),
               render_share_of_24ms_step=big["ms_median"] / 24.0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
