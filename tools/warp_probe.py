"""Cost of the image warps on the device (include/mavflow_warp.h), next to a host resampler standing in for cv2.

    python tools/warp_probe.py [--reps 50] [--host-reps 2] [--out FILE] [--lib OTHER_BUILD.so --tag NAME]

Device-resident, HIP-event time (mav_timer_start / stop around ONE enqueue, synchronised), median of --reps after 3 warm-up enqueues, at
1280x720 and 1920x1080, batch 1 and 16.  Every coordinate route (remap, remap_planes, warp_flow, warp_affine, warp_perspective) on U8C3 and
F32C2, plus warp_method (perspective), each on two warps: "smooth" (a displacement of a few pixels: neighbouring lanes read neighbouring
taps) and "rot90" (a quarter turn about the centre, the gather's unfriendly case: a row of lanes walks down a column of the source).
  ms          one enqueue of the whole batch
  model_gbps  destination written + source read once + the map or flow where one is read (warp_method: the field read, diff and mag
              written), over ms: a LOWER bound of the traffic (the four taps of neighbouring pixels overlap in cache, not in this count)
  membw_*     mav_membw_probe (a 3-read-1-write stream kernel) of the same process, at a cache-resident (4 x 32 MB) and an HBM (4 x 512 MB) size
  host_standin_ms   scipy.ndimage.map_coordinates(order=1, mode="grid-constant") per channel at batch 1, best of --host-reps in the same
              process, on the same coordinates: a STAND-IN for cv2 (not installed), not a measurement of cv2; given per image, so that a
              batch-16 row compares ms / 16 with it
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

from mavflow import _lib, warp  # noqa: E402

FORMATS = {"U8C3": (warp.WARP_U8C3, np.uint8, 3), "F32C2": (warp.WARP_F32C2, np.float32, 2)}


def maps_of(W, H):
    """name -> ((H, W, 2) float32 absolute coordinates, the 2x3 matrix that maps destination to source, its 3x3 form)"""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    out = {}
    a = np.deg2rad(2.0)
    c, s, cx, cy = 1.01 * np.cos(a), 1.01 * np.sin(a), (W - 1) / 2, (H - 1) / 2
    A = np.array([[c, s, (1 - c) * cx - s * cy + 1.3], [-s, c, s * cx + (1 - c) * cy - 0.7]])
    out["smooth"] = A
    out["rot90"] = np.array([[0.0, 1.0, cx - cy], [-1.0, 0.0, cx + cy]])
    res = {}
    for name, A in out.items():
        m = np.stack([A[0, 0] * x + A[0, 1] * y + A[0, 2], A[1, 0] * x + A[1, 1] * y + A[1, 2]], axis=-1).astype(np.float32)
        res[name] = (m, A, np.vstack([A, [0.0, 0.0, 1.0]]))
    return res


def host_standin(img, m, reps):
    import scipy.ndimage as ndi
    coords = [m[..., 1].astype(np.float64), m[..., 0].astype(np.float64)]
    src = img.astype(np.float64) if img.dtype == np.uint8 else img
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = np.stack([ndi.map_coordinates(src[..., ch], coords, order=1, mode="grid-constant", cval=0.0) for ch in range(src.shape[2])], axis=-1)
        if img.dtype == np.uint8:
            out = np.floor(out + 0.5).astype(np.uint8)
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best * 1e3


def timed(ctx, reps, enqueue):
    for _ in range(3):
        enqueue()
    ctx.sync()
    ts = []
    for _ in range(reps):
        ctx.timer_start()
        enqueue()
        ts.append(ctx.timer_stop())
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--lib", default=None, help="another build of libmavflow.so (an A/B build of kernels_warp.hip with -DWARP_CAP)")
    ap.add_argument("--tag", default=None, help="a label for the lines of this run")
    args = ap.parse_args()
    if args.lib:
        _lib.load(args.lib)
    lines = []

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        lines.append(line)

    for (W, H) in ((1280, 720), (1920, 1080)):
        n0 = W * H
        warps = maps_of(W, H)
        rng = np.random.default_rng(W)
        host_ms = {}
        for B in (1, 16):
            with _lib.Context(W, H, B) as ctx:
                membw_cache, membw_hbm = ctx.membw_probe(32 << 20), ctx.membw_probe(512 << 20, reps=5)
                common = dict(probe="warp", **({"tag": args.tag} if args.tag else {}), W=W, H=H, batch=B, membw_probe_cache_gbps=round(membw_cache, 1),
                              membw_probe_hbm_gbps=round(membw_hbm, 1))
                for fname, (fmt, dt, ch) in FORMATS.items():
                    img = (rng.integers(0, 256, (H, W, ch), dtype=np.uint8) if dt == np.uint8 else rng.normal(0, 3, (H, W, ch)).astype(np.float32))
                    px = img.dtype.itemsize * ch
                    d_src = ctx.alloc(B * img.nbytes)
                    d_dst = ctx.alloc(B * img.nbytes)
                    for b in range(B):
                        _lib.check(ctx.lib.mav_memcpy_h2d(ctx.h, d_src.ptr + b * img.nbytes, _lib._ptr(img), img.nbytes))
                    for wname, (m, A, P) in warps.items():
                        y, x = np.mgrid[0:H, 0:W].astype(np.float32)
                        flow = (np.stack([x, y], axis=-1) - m).astype(np.float32)
                        ops = dict(map=np.stack([m] * B), mx=np.stack([m[..., 0]] * B), my=np.stack([m[..., 1]] * B), flow=np.stack([flow] * B),
                                   A=np.stack([A] * B), P=np.stack([P] * B))
                        d = {k: ctx.alloc(v.nbytes).upload(np.ascontiguousarray(v)) for k, v in ops.items()}
                        routes = {
                            "remap": (lambda: ctx.remap_enqueue(d_src, fmt, d["map"], d_dst, B), 8),
                            "remap_planes": (lambda: ctx.remap_enqueue(d_src, fmt, d["mx"], d_dst, B, d["my"]), 8),
                            "warp_flow": (lambda: ctx.warp_flow_enqueue(d_src, fmt, d["flow"], d_dst, B), 8),
                            "warp_affine": (lambda: ctx.warp_affine_enqueue(d_src, fmt, d["A"], d_dst, B, inverse_map=True), 0),
                            "warp_perspective": (lambda: ctx.warp_perspective_enqueue(d_src, fmt, d["P"], d_dst, B, inverse_map=True), 0),
                        }
                        if B == 1 and args.host_reps > 0:
                            host_ms[(fname, wname)] = host_standin(img, m, args.host_reps)
                        hs = host_ms.get((fname, wname))
                        for rname, (enqueue, map_bytes) in routes.items():
                            ms = timed(ctx, args.reps, enqueue)
                            model = (2 * px + map_bytes) * n0 * B
                            emit(dict(common, route=rname, format=fname, warp=wname, ms=round(ms, 4), model_mb=round(model / 1e6, 1),
                                      model_gbps_lower_bound=round(model / (ms * 1e-3) / 1e9, 1), host_standin_ms_per_image=None if hs is None else round(hs, 1),
                                      speedup_vs_standin=None if hs is None else round(hs * B / ms, 1)))
                        if fname == "F32C2":
                            d_mag, d_rec = ctx.alloc(B * n0 * 4), ctx.alloc(16 * B)
                            ms = timed(ctx, args.reps, lambda: ctx.warp_method_enqueue(d_src, d["P"], warp.WARP_PERSPECTIVE, d_rec, B, d_dst, d_mag))
                            model = (8 + 8 + 4) * n0 * B
                            emit(dict(common, route="warp_method", format=fname, warp=wname, ms=round(ms, 4), model_mb=round(model / 1e6, 1),
                                      model_gbps_lower_bound=round(model / (ms * 1e-3) / 1e9, 1), host_standin_ms_per_image=None if hs is None else round(hs, 1),
                                      speedup_vs_standin=None if hs is None else round(hs * B / ms, 1)))
                            d_mag.free(); d_rec.free()
                        for b in d.values():
                            b.free()
                    d_src.free(); d_dst.free()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
