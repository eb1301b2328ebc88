"""Cost of the device PNG decoder (mav_png_decode_dev) next to the host route it can replace (frame_source.imread).

    python tools/png_decode_probe.py [--reps 50] [--budget-s 4] [--counts 1,16,64,256,1024] [--out FILE]

Per shape (1280x720, 1920x1080), colour (RGB, gray) and input (a smooth synthetic frame, a textured one; files as cv2.imwrite's
defaults lay them out: frame_source.encode_png), in ONE process, the two routes alternating:
  host    ms per frame of frame_source.imread over files on disk, on one thread and over a pool of 16 threads;
  device  HIP-event time of one mav_png_decode_dev call of `count` files to BGR frames left on the device (the memset, the inflate,
          Adler-32 and un-filter launches), median over --reps calls after two warm-up calls -- fewer where --budget-s seconds per
          configuration run out, and the line says how many.  The compressed bytes are resident (the upload is count x a few hundred KB
          and is reported as bytes, not timed); the same file is decoded `count` times through an index whose entries all name it.
One JSON line per configuration; nothing is printed for a configuration that was not run."""
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

from mavflow import _lib, frame_source  # noqa: E402


def frame(W, H, colour, kind):
    rng = np.random.default_rng(1)
    y, x = np.mgrid[0:H, 0:W]
    base = (96 + 64 * np.sin(x / 97.0) + 48 * np.cos(y / 61.0))
    ch = 3 if colour == "rgb" else 1
    img = np.stack([base + 9 * k for k in range(ch)], axis=2)
    if kind == "textured":
        img = img + rng.integers(-16, 17, (H, W, ch))
    img = np.clip(img, 0, 255).astype(np.uint8)
    return img if ch == 3 else img[..., 0]


def host_ms(paths, threads):
    t0 = time.perf_counter()
    if threads == 1:
        for p in paths:
            assert frame_source.imread(p) is not None
    else:
        with ThreadPoolExecutor(threads) as ex:
            assert all(f is not None for f in ex.map(frame_source.imread, paths))
    return 1e3 * (time.perf_counter() - t0) / len(paths)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--budget-s", type=float, default=4.0)
    ap.add_argument("--counts", default="1,16,64,256,1024")
    ap.add_argument("--shapes", default="1280x720,1920x1080")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    counts = [int(v) for v in a.counts.split(",")]
    lines = []

    def emit(d):
        s = json.dumps(d)
        print(s, flush=True)
        lines.append(s)

    with tempfile.TemporaryDirectory() as tmp:
        for shape in a.shapes.split(","):
            W, H = (int(v) for v in shape.split("x"))
            with _lib.Context(W, H, 1) as c:
                for colour in ("rgb", "gray"):
                    for kind in ("smooth", "textured"):
                        img = frame(W, H, colour, kind)
                        data = frame_source.encode_png(img)
                        paths = []
                        for k in range(64):
                            paths.append(os.path.join(tmp, f"{shape}_{colour}_{kind}_{k:03d}.png"))
                            with open(paths[-1], "wb") as f:
                                f.write(data)
                        want = frame_source.imread(paths[0])
                        Wd, Hd, ch, streams, _ = c._png_streams([data])
                        nz = streams.size - 1
                        d_z = c.alloc(streams.nbytes).upload(streams)
                        host1, host16 = [], []
                        for count in counts:
                            host1.append(host_ms(paths[:4], 1))                     # the routes alternate: host, device, host, ...
                            host16.append(host_ms(paths, 16))
                            index = np.tile(np.array([[0, nz]], np.uint64), (count, 1))
                            bufs = [c.alloc(index.nbytes).upload(index), c.alloc(count * Hd * Wd * 3), c.alloc(48 * count),
                                    c.alloc(c.png_decode_scratch_bytes(Wd, Hd, ch, count))]
                            try:
                                def run():
                                    c.png_decode_dev(d_z, bufs[0], count, Wd, Hd, ch, "bgr", bufs[1], bufs[2], bufs[3])
                                run()
                                c.sync()
                                st = bufs[2].download(_lib.PNG_STATUS_DTYPE, (count,))
                                first = bufs[1].download(np.uint8, (Hd, Wd, 3))
                                assert not st["code"].any() and np.array_equal(first, want), "the device route decoded something else"
                                run()
                                c.sync()
                                ms, t0 = [], time.perf_counter()
                                while len(ms) < a.reps and (len(ms) < 3 or time.perf_counter() - t0 < a.budget_s):
                                    c.timer_start()
                                    run()
                                    ms.append(c.timer_stop())
                                ms = np.array(ms)
                                emit(dict(shape=shape, colour=colour, input=kind, count=count, file_bytes=len(data), stream_bytes=int(nz),
                                          raw_bytes=int(st["produced"][0]), device_ms_per_call=float(np.median(ms)),
                                          device_ms_per_frame=float(np.median(ms)) / count, device_ms_min=float(ms.min()), device_ms_max=float(ms.max()),
                                          reps=int(ms.size), host_1_thread_ms_per_frame=host1[-1], host_16_threads_ms_per_frame=host16[-1]))
                            finally:
                                c.sync()
                                for b in bufs:
                                    b.free()
                        d_z.free()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
