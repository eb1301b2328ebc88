"""Cost and yield of the device PNG encoder (mav_png_encode_dev) next to the host encoder it can replace.

    python tools/png_probe.py [--reps 20] [--loop-frames 128] [--skip-loops]

Device: HIP-event time of one mav_png_encode_dev call on the three rendered images of 64 pairs at 1920x1080 and of one pair at
1280x720 (median and range over --reps calls), bytes in and out, (in + out) / time, next to the mav_render_dev call that produced the
images; the HIP-event time of the encoder's kernel class alone is what mav_profile_get reports under "misc".  Sizes: per image kind
the device stream's bytes over frame_source.encode_png's of the same array (Processor's three images of real Farneback pairs, and a
textured overlay frame).  Loops: frames per second of Processor.run_detection and run_detection_batched(64) at 1080p with the files
on, png_encoder host / device alternated twice, images only and images + processed frames.  Prints one JSON line."""
from __future__ import annotations

import argparse
import json
import logging
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "mav-detection_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from mavflow import _lib, frame_source, synth  # noqa: E402


def _timed(c, run, reps):
    run(); run()
    c.sync()
    ms = []
    for _ in range(reps):
        c.timer_start()
        run()
        ms.append(c.timer_stop())
    ms = np.array(ms)
    return dict(ms_median=float(np.median(ms)), ms_min=float(ms.min()), ms_max=float(ms.max()))


def device_time(W: int, H: int, B: int, reps: int):
    """render + encode of the three images of B pairs (a synthetic flow with rotation, a sky mask, a frame-0 pair)"""
    flow = np.ascontiguousarray(np.broadcast_to(synth.synthetic_flow(W, H, seed=1), (B, H, W, 2)))
    rng = np.random.default_rng(0)
    foe = np.stack([rng.uniform(0.3 * W, 0.7 * W, B), rng.uniform(0.3 * H, 0.7 * H, B)], axis=1)
    omega = rng.normal(0.0, 0.02, (B, 3))
    dt = np.full(B, 1 / 30.0)
    frame0 = np.zeros(B, np.uint8)
    frame0[0] = 1
    sky = np.zeros((B, H, W), np.uint8)
    sky[:, : H // 8] = 1
    n_img = 3 * B
    with _lib.Context(W, H, B) as c:
        d = {k: c.alloc(a.nbytes).upload(np.ascontiguousarray(a)) for k, a in
             dict(flow=flow, foe=foe, omega=omega, dt=dt, frame0=frame0, sky=sky).items()}
        per = B * H * W * 3
        imgs = c.alloc(3 * per)
        bound = c.lib.mav_png_bound(W, H, 3) * n_img
        out, idx = c.alloc(bound), c.alloc(16 * n_img)

        def render():
            c.render_dev(d["flow"].ptr, d["foe"].ptr, B, imgs.ptr, imgs.ptr + per, imgs.ptr + 2 * per, omega_ptr=d["omega"].ptr,
                         dt_ptr=d["dt"].ptr, frame0_ptr=d["frame0"].ptr, sky_ptr=d["sky"].ptr)

        def encode():
            _lib.check(c.lib.mav_png_encode_dev(c.h, imgs.ptr, n_img, 3, out.ptr, bound, idx.ptr))
        r = _timed(c, render, reps)
        e = _timed(c, encode, reps)
        index = idx.download(np.uint64, (n_img, 2))
    bytes_in, bytes_out = 3 * per, int(index[-1].sum())
    e.update(images=n_img, bytes_in=bytes_in, bytes_out=bytes_out, gbytes_per_s=(bytes_in + bytes_out) / (e["ms_median"] * 1e-3) / 1e9,
             out_over_in=bytes_out / bytes_in, times_the_render=e["ms_median"] / r["ms_median"])
    return dict(W=W, H=H, B=B, render=r, encode=e)


def size_ratios(W: int, H: int, B: int):
    """device stream bytes / host file bytes per image kind, on the images of real Farneback pairs"""
    prev, nxt = synth.make_batch(W, H, B, distinct=B)
    smp = np.stack([synth.foe_samples(W, H, b) for b in range(B)])
    frames = np.ascontiguousarray(np.stack([nxt, np.roll(nxt, 3, axis=-1), 255 - nxt], -1))
    out = {}
    with _lib.Context(W, H, B) as c:
        c.process_batch(prev, nxt, smp)
        imgs = c.render_last(B)
        files = c.render_last_png(B)
        over = np.array(c.overlay_last(frames, [(0.55 * W, 0.45 * H)] * B)[0])
        files["overlay_textured"] = c.overlay_last_png(frames, [(0.55 * W, 0.45 * H)] * B)[0]
    imgs["overlay_textured"] = over
    tot_d = tot_h = 0
    for k, fl in files.items():
        dev = sum(len(f) for f in fl)
        host = sum(len(frame_source.encode_png(im)) for im in imgs[k])
        out[k] = dict(device_bytes=dev, host_bytes=host, ratio=dev / host, raw_bytes=int(imgs[k].nbytes))
        if k != "overlay_textured":
            tot_d, tot_h = tot_d + dev, tot_h + host
    out["result_flow_phi_total"] = dict(device_bytes=tot_d, host_bytes=tot_h, ratio=tot_d / tot_h)
    return out


def loop_rate(W: int, H: int, n: int, batch, processed: bool, encoder: str) -> float:
    """Frames per second of one Processor loop over n frames with the files on (4 distinct synthetic pairs, made before the clock starts)"""
    from mavflow.processor import Processor, SyntheticDataset
    from mavflow.run_config import RunConfig
    ds = SyntheticDataset(W, H, n + 1, use_farneback=True, distinct=4)
    for i in range(4):
        ds.frame_pair(i)
    with tempfile.TemporaryDirectory() as tmp:
        p = Processor(RunConfig(logging.getLogger("probe"), ds, "", False, False, False, True, False, False, "FLOW_FOE_CLUSTERING"),
                      images_path=os.path.join(tmp, "img"), processed_path=os.path.join(tmp, "processed") if processed else None,
                      png_encoder=encoder)
        np.random.seed(0)
        t0 = time.perf_counter()
        p.run_detection() if batch is None else p.run_detection_batched(batch)
        dt = time.perf_counter() - t0
        p.release()
    return n / dt


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--loop-frames", type=int, default=128)
    ap.add_argument("--skip-loops", action="store_true")
    a = ap.parse_args()
    out = dict(encode_1080p_x64=device_time(1920, 1080, 64, a.reps), encode_720p_x1=device_time(1280, 720, 1, a.reps),
               sizes_1080p=size_ratios(1920, 1080, 2))
    if not a.skip_loops:
        loops = {}
        for rnd in range(2):                                   # host / device alternated, twice
            for name, batch in (("run_detection", None), ("run_detection_batched_64", 64)):
                for processed in (False, True):
                    for enc in ("host", "device"):
                        key = f"{name}_{'images+processed' if processed else 'images'}_{enc}"
                        loops.setdefault(key, []).append(loop_rate(1920, 1080, a.loop_frames, batch, processed, enc))
        out["loops_1080p_frames_per_s"] = loops
    print(json.dumps(out))


if __name__ == "__main__":
    main()
