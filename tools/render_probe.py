"""Cost of the result images (mav_render_dev), of the processed.mp4 frame (mav_overlay_dev, mav_last_overlay) and of writing them as
PNG files.

    python tools/render_probe.py [--reps 20] [--png-frames 48] [--loop-frames 128]

Device: HIP-event time of one mav_render_dev call with all three images, at 1920x1080 x 64 pairs and 1280x720 x 1, on a synthetic
float32 flow with rotation, a sky mask and a frame-0 pair.  The kernels move 26 B per pixel: the flow twice (8 B each: the max |flow|
reduction, then the render), the sky once (1 B) and three 3-byte images; 18 B/px is the floor of a single pass.  Both are reported as
a fraction of 8 TB/s.  Host: PNG files per second for three 1080p images per frame, encoded by 16 threads (frame_source.imwrite).
Overlay: HIP-event time of one mav_overlay_dev call at the same two sizes (frame 3 B + mask 1 B in, 3 B out: 7 B/px), next to the
result image alone (mav_render_dev, which recomputes the fixed mask from the flow instead of reading it); the per-frame cost of
Context.overlay_last at 1080p after a detection call, host clock, BGR upload and download included; frames per second of
Processor.run_detection and run_detection_batched(64) at 1080p with processed_path off and on (PNG files included), alternated.
Prints one JSON line."""
from __future__ import annotations

import argparse
import json
import logging
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


def overlay_time(W: int, H: int, B: int, reps: int):
    rng = np.random.default_rng(0)
    frames = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    mask = (rng.random((B, H, W)) < 0.05).astype(np.uint8)
    foe = np.stack([rng.uniform(0.3 * W, 0.7 * W, B), rng.uniform(0.3 * H, 0.7 * H, B)], axis=1)
    gt = np.tile([0.55 * W, 0.45 * H], (B, 1))
    flow = np.ascontiguousarray(np.broadcast_to(synth.synthetic_flow(W, H, seed=1), (B, H, W, 2)))
    with _lib.Context(W, H, B) as c:
        d = {k: c.alloc(a.nbytes).upload(np.ascontiguousarray(a)) for k, a in
             dict(frames=frames, mask=mask, foe=foe, gt=gt, flow=flow).items()}
        out, wr, res = c.alloc(frames.nbytes), c.alloc(B), c.alloc(frames.nbytes)

        def timed(run):
            run(); run()
            c.sync()
            ms = []
            for _ in range(reps):
                c.timer_start()
                run()
                ms.append(c.timer_stop())
            return np.array(ms)
        ov = timed(lambda: c.overlay_dev(d["frames"].ptr, d["mask"].ptr, d["foe"].ptr, d["gt"].ptr, B, out.ptr, wr.ptr))
        rs = timed(lambda: c.render_dev(d["flow"].ptr, d["foe"].ptr, B, res.ptr))
    px = W * H * B
    med = float(np.median(ov))
    return dict(W=W, H=H, B=B, ms_median=med, ms_min=float(ov.min()), ms_max=float(ov.max()),
                frac_peak_7Bpx=7 * px / (med * 1e-3) / PEAK_BPS, result_image_from_flow_ms_median=float(np.median(rs)))


def overlay_last_cost(W: int, H: int, reps: int):
    """ms per Context.overlay_last(frame) of one pair after process_batch: BGR up, kernel, overlay down, synchronous."""
    prev, nxt = synth.make_batch(W, H, 1, distinct=1)
    smp = synth.foe_samples(W, H, 0)[None]
    frame = np.repeat(nxt[0][..., None], 3, axis=2)
    with _lib.Context(W, H, 1) as c:
        c.process_batch(prev, nxt, smp)
        c.overlay_last(frame, [(0.55 * W, 0.45 * H)])
        ms = []
        for _ in range(reps):
            t0 = time.perf_counter()
            c.overlay_last(frame, [(0.55 * W, 0.45 * H)])
            ms.append((time.perf_counter() - t0) * 1e3)
    ms = np.array(ms)
    return dict(W=W, H=H, ms_median=float(np.median(ms)), ms_min=float(ms.min()), ms_max=float(ms.max()),
                pcie_bytes_per_frame=2 * 3 * W * H)


def loop_rate(W: int, H: int, n: int, batch, processed: bool) -> float:
    """Frames per second of one Processor loop over n frames (4 distinct synthetic pairs, synthesised before the clock starts)."""
    from mavflow.processor import Processor, SyntheticDataset
    from mavflow.run_config import RunConfig
    ds = SyntheticDataset(W, H, n + 1, use_farneback=True, distinct=4)
    for i in range(4):
        ds.frame_pair(i)
    with tempfile.TemporaryDirectory() as tmp:
        p = Processor(RunConfig(logging.getLogger("probe"), ds, "", False, False, False, True, False, False, "FLOW_FOE_CLUSTERING"),
                      processed_path=os.path.join(tmp, "processed") if processed else None)
        np.random.seed(0)
        t0 = time.perf_counter()
        p.run_detection() if batch is None else p.run_detection_batched(batch)
        dt = time.perf_counter() - t0
        p.release()
    return n / dt


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--png-frames", type=int, default=48)
    ap.add_argument("--loop-frames", type=int, default=128)
    a = ap.parse_args()
    big, sample = device_time(1920, 1080, 64, a.reps)
    small, _ = device_time(1280, 720, 1, a.reps)
    out = dict(render_1080p_x64=big, render_720p_x1=small, png_1080p=png_rate(sample, a.png_frames),
               render_share_of_24ms_step=big["ms_median"] / 24.0)
    out["overlay_1080p_x64"] = overlay_time(1920, 1080, 64, a.reps)
    out["overlay_720p_x1"] = overlay_time(1280, 720, 1, a.reps)
    out["overlay_last_1080p"] = overlay_last_cost(1920, 1080, a.reps)
    loops = {}
    for rnd in range(2):                                   # off / on alternated, twice
        for name, batch in (("run_detection", None), ("run_detection_batched_64", 64)):
            for processed in (False, True):
                key = f"{name}_processed_{'on' if processed else 'off'}"
                loops.setdefault(key, []).append(loop_rate(1920, 1080, a.loop_frames, batch, processed))
    out["loops_1080p_frames_per_s"] = loops
    print(json.dumps(out))


if __name__ == "__main__":
    main()
