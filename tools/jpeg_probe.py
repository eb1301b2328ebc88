"""Cost of JPEG decode on the device (mav_jpeg_decode_dev), next to the host route in the same process, in alternation.

    python tools/jpeg_probe.py [--reps 5] [--out FILE] [--files NPZ] [--make-files NPZ]

Synthetic textured frames, 4:2:0 at quality 90, at 1280x720, 1920x1080 and one ragged VisDrone-like 1904x1071; batches of 1, 16 and 64
(four different pictures, repeated); restart markers three ways: none, one per MCU row, one per 8 MCUs.  Per configuration one JSON line:
  device_ms          one mav_jpeg_decode_dev call on device-resident files, enqueue to synchronised, median of --reps
  launch_ms          the four launches separately: classes "jpeg_intervals" / "jpeg_entropy" / "jpeg_idct" / "jpeg_finish" of
                     mav_profile_get (HIP events around every launch) over --reps more calls, mean per call
  host16_ms          mav_jpeg_decode_host (the same source) over the batch on 16 threads
  pillow16_ms        PIL.Image.open(...).load() over the batch on 16 threads, where Pillow imports
  upload_ms          the upload of the decoded BGR frames that the host route then needs (about 6 MB per 1080p frame)
The files come from Pillow's encoder: --make-files writes them to an NPZ (no GPU needed), --files reads one where Pillow is absent."""
from __future__ import annotations

import argparse
import io
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "mav-detection_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

SIZES = [(1280, 720), (1920, 1080), (1904, 1071)]
BATCHES = [1, 16, 64]
RESTARTS = ["none", "row", "8"]
PICTURES = 4
THREADS = 16


def picture(W, H, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    base = np.stack([128 + 90 * np.sin(xx / 37.0 + seed) * np.cos(yy / 53.0), 128 + 80 * np.cos(xx / 91.0 - yy / 29.0), (xx * 0.13 + yy * 0.21 + 40 * seed) % 256], -1)
    return np.clip(base + rng.normal(0, 12, (H, W, 3)), 0, 255).astype(np.uint8)


def make_files():
    from PIL import Image
    out = {}
    for W, H in SIZES:
        for r in RESTARTS:
            for k in range(PICTURES):
                kw = {"row": {"restart_marker_rows": 1}, "8": {"restart_marker_blocks": 8}, "none": {}}[r]
                b = io.BytesIO()
                Image.fromarray(picture(W, H, k)).save(b, "JPEG", quality=90, subsampling=2, **kw)
                out[f"{W}x{H}_{r}_{k}"] = np.frombuffer(b.getvalue(), np.uint8)
    return out


def median_ms(f, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out")
    ap.add_argument("--files")
    ap.add_argument("--make-files")
    args = ap.parse_args()
    if args.make_files:
        np.savez(args.make_files, **make_files())
        return
    files = dict(np.load(args.files)) if args.files else make_files()
    try:
        from PIL import Image
    except ImportError:
        Image = None
    from mavflow import _lib
    lib = _lib.load()
    pool = ThreadPoolExecutor(THREADS)
    lines = []
    for W, H in SIZES:
        with _lib.Context(W, H, 1) as ctx:
            for r in RESTARTS:
                four = [files[f"{W}x{H}_{r}_{k}"].tobytes() for k in range(PICTURES)]
                for n in BATCHES:
                    batch = [four[k % PICTURES] for k in range(n)]
                    _, _, comps, packed, index, infos = ctx._jpeg_pack(batch)
                    bufs = [ctx.alloc(packed.nbytes).upload(packed), ctx.alloc(index.nbytes).upload(index), ctx.alloc(infos.nbytes).upload(infos),
                            ctx.alloc(n * H * W * 3), ctx.alloc(40 * n), ctx.alloc(ctx.jpeg_decode_scratch_bytes(W, H, comps, n))]
                    raws = [np.frombuffer(f + b"\0", np.uint8) for f in batch]
                    outs = [np.empty((H, W, 3), np.uint8) for _ in batch]
                    sts = [np.zeros(1, _lib.JPEG_STATUS_DTYPE) for _ in batch]
                    frames = np.empty((n, H, W, 3), np.uint8)

                    def device():
                        ctx.jpeg_decode_dev(bufs[0], bufs[1], bufs[2], n, W, H, "bgr", bufs[3], bufs[4], bufs[5])
                        ctx.sync()

                    def host_one(k):
                        lib.mav_jpeg_decode_host(raws[k].ctypes.data, len(batch[k]), infos[k:k + 1].ctypes.data, 1, outs[k].ctypes.data, sts[k].ctypes.data)

                    def host16():
                        list(pool.map(host_one, range(n)))

                    def pillow16():
                        list(pool.map(lambda f: Image.open(io.BytesIO(f)).load(), batch))

                    def upload():
                        bufs[3].upload(frames)
                        ctx.sync()

                    try:
                        device()
                        status = bufs[4].download(_lib.JPEG_STATUS_DTYPE, (n,))
                        assert not status["code"].any(), status["code"]
                        host16()
                        assert np.array_equal(bufs[3].download(np.uint8, (n, H, W, 3))[0], outs[0])
                        t = {"device_ms": [], "host16_ms": [], "pillow16_ms": [], "upload_ms": []}
                        for _ in range(args.reps):                       # in alternation
                            t["device_ms"].append(median_ms(device, 1))
                            t["host16_ms"].append(median_ms(host16, 1))
                            if Image is not None:
                                t["pillow16_ms"].append(median_ms(pillow16, 1))
                            t["upload_ms"].append(median_ms(upload, 1))
                        ctx.profile_enable(1)
                        for _ in range(args.reps):
                            device()
                        prof = ctx.profile_get()
                        ctx.profile_enable(0)
                    finally:
                        ctx.sync()
                        for b in bufs:
                            b.free()
                    line = {"W": W, "H": H, "restart": r, "batch": n, "file_kb": round(sum(len(f) for f in batch) / n / 1024, 1),
                            "intervals": int(status["intervals"][0]), "reps": args.reps}
                    for k, v in t.items():
                        if v:
                            line[k] = round(float(np.median(v)), 3)
                            line[k.replace("_ms", "_ms_per_image")] = round(float(np.median(v)) / n, 3)
                    line["launch_ms"] = {k[5:]: round(prof[k][0] / max(args.reps, 1), 3) for k in ("jpeg_intervals", "jpeg_entropy", "jpeg_idct", "jpeg_finish")}
                    print(json.dumps(line), flush=True)
                    lines.append(json.dumps(line))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
