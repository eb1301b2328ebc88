"""Cost of the shapes family on the device (include/mavflow_shapes.h), next to the only route there was before it: bring the frame to
the host, draw there, send it back.

    python tools/shapes_probe.py [--reps 50] [--rounds 5] [--host-reps 2] [--out FILE]

Everything resident, at 1280x720 and 1920x1080:
  foe_draw_lines   FocusOfExpansion.draw's workload: 2 000 lines of thickness 2 in two colours into one frame, the ORDERED form (plane
                   cleared, pass A, pass B) and the DIRECT form of the same table
  blob_boxes       256 boxes x batch 64, thickness 2, one colour: mav_shapes_from_blobs_dev + mav_draw_shapes_dev (DIRECT, n_dev)
  mosaic           the 2 x 3 debug frame of one image (five 3-channel tiles, one gray)
  add_saturate     cv2.add of two frames
IN ALTERNATION, --rounds times in this process: a block of the device form (HIP-event time, mav_timer_start / stop around ONE enqueue,
median of --reps after 3 warm-up enqueues), then a block of the PCIe round trip of the frame(s) the workload draws into (mav_memcpy_d2h +
mav_memcpy_h2d with nothing in between, wall clock, median of --reps; of the 64 frames: --reps / 10).  Each figure is the median of
its round medians; the round medians themselves are in `*_rounds`.  A device draw slower than that round trip would be a defect.
host_route_ms: the round trip plus the host drawing by tests/shapes_ref.py's scalar restatement, --host-reps runs behind the rounds
(no cv2 exists here to time instead; for the blob boxes ONE image of the 64 is drawn on the host and the field's name says so).
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

from mavflow import _lib, shapes  # noqa: E402

SIZES = ((1280, 720), (1920, 1080))


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


def roundtrip(ctx, buf, host, reps, draw=None):
    """the frame(s) down, `draw` on the host, up again: wall-clock ms, median"""
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        _lib.check(ctx.lib.mav_memcpy_d2h(ctx.h, _lib._ptr(host), buf.ptr, host.nbytes))
        if draw is not None:
            draw(host)
        _lib.check(ctx.lib.mav_memcpy_h2d(ctx.h, buf.ptr, _lib._ptr(host), host.nbytes))
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def alternate(rounds, blocks):
    """blocks: name -> a function returning one block's median.  Round after round, each block in turn -> name -> (median of the round
    medians, the round medians)"""
    per = {k: [] for k in blocks}
    for _ in range(rounds):
        for k, f in blocks.items():
            per[k].append(f())
    return {k: (float(np.median(v)), [round(x, 5) for x in v]) for k, v in per.items()}


def foe_lines(W, H, n=2000, seed=5):
    rng = np.random.RandomState(seed)
    p = rng.randint(0, [W, H], (n, 2))
    q = p + rng.randint(-60, 61, (n, 2))
    col = rng.randint(0, 2, n)
    return shapes.table([shapes.shape(shapes.LINE, p[i, 0], p[i, 1], q[i, 0], q[i, 1], 2, (0, 255, 0) if col[i] else (0, 0, 255)) for i in range(n)])


def blob_tables(W, H, B, n=256, seed=6):
    rng = np.random.RandomState(seed)
    counts = np.zeros(B, _lib.CC_COUNTS_DTYPE)
    counts["n_blobs"] = counts["n_components"] = n
    tab = np.zeros((B, n), _lib.BLOB_DTYPE)
    tab["x"], tab["y"] = rng.randint(0, W - 80, (B, n)), rng.randint(0, H - 60, (B, n))
    tab["w"], tab["h"] = rng.randint(4, 80, (B, n)), rng.randint(4, 60, (B, n))
    return counts, tab


def main():
    import shapes_ref as R
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines_out = []

    def emit(**kw):
        s = json.dumps(kw)
        print(s, flush=True)
        lines_out.append(s)

    for W, H in SIZES:
        n = W * H
        with _lib.Context(W, H, 64) as ctx:
            frame = np.random.RandomState(1).randint(0, 255, (1, H, W, 3)).astype(np.uint8)
            img = ctx.alloc(frame.nbytes).upload(frame)
            # FoE.draw's lines
            tab = foe_lines(W, H)
            dtab = ctx.alloc(tab.nbytes).upload(tab)
            plane = ctx.alloc(shapes.scratch_bytes(W, H, 1))
            host_frame = frame.copy()
            r = alternate(a.rounds, dict(
                ordered=lambda: timed(ctx, a.reps, lambda: ctx.draw_shapes_enqueue(img, dtab, len(tab), 3, 1, scratch_ptr=plane)),
                direct=lambda: timed(ctx, a.reps, lambda: ctx.draw_shapes_enqueue(img, dtab, len(tab), 3, 1)),
                pcie=lambda: roundtrip(ctx, img, host_frame, a.reps)))
            host = roundtrip(ctx, img, frame.copy(), a.host_reps, lambda h: R.draw_shapes(h, tab.view(R.SHAPE_DTYPE)))
            emit(what="foe_draw_lines", W=W, H=H, records=len(tab), ordered_ms=r["ordered"][0], direct_ms=r["direct"][0], pcie_roundtrip_ms=r["pcie"][0],
                 ordered_rounds=r["ordered"][1], direct_rounds=r["direct"][1], pcie_rounds=r["pcie"][1], host_route_ms=host, plane_mb=4 * n / 1e6)
            for b in (dtab, plane):
                b.free()
            # add
            other = ctx.alloc(frame.nbytes).upload(frame[:, ::-1].copy())
            dst = ctx.alloc(frame.nbytes)
            r = alternate(a.rounds, dict(add=lambda: timed(ctx, a.reps, lambda: ctx.add_saturate_enqueue(img, other, dst, 3, 1)),
                                         pcie=lambda: roundtrip(ctx, dst, host_frame, a.reps)))
            emit(what="add_saturate", W=W, H=H, ms=r["add"][0], pcie_roundtrip_ms=r["pcie"][0], ms_rounds=r["add"][1], pcie_rounds=r["pcie"][1],
                 model_mb=9 * n / 1e6)
            # mosaic: five pictures and a gray plane
            gray = ctx.alloc(n).upload(frame[..., 0].copy())
            out = ctx.alloc(18 * n)
            big = np.empty((2 * H, 3 * W, 3), np.uint8)
            r = alternate(a.rounds, dict(
                mosaic=lambda: timed(ctx, a.reps, lambda: ctx.mosaic_enqueue([img, other, dst, img, other, gray], [3, 3, 3, 3, 3, 1], 2, 3, out, 1)),
                pcie=lambda: roundtrip(ctx, out, big, a.reps)))
            emit(what="mosaic", W=W, H=H, ms=r["mosaic"][0], pcie_roundtrip_ms_of_the_mosaic=r["pcie"][0], ms_rounds=r["mosaic"][1],
                 pcie_rounds=r["pcie"][1], model_mb=(16 + 18) * n / 1e6)
            for b in (other, dst, gray, out, img):
                b.free()
            # blob boxes, batch 64
            B = 64
            counts, blobs = blob_tables(W, H, B)
            frames = np.random.RandomState(2).randint(0, 255, (B, H, W, 3)).astype(np.uint8)
            imgs = ctx.alloc(frames.nbytes).upload(frames)
            dc, db = ctx.alloc(counts.nbytes).upload(counts), ctx.alloc(blobs.nbytes).upload(blobs)
            ds, dn = ctx.alloc(32 * B * 256), ctx.alloc(4)

            def boxes():
                ctx.shapes_from_blobs_enqueue(db, dc, B, 256, ds, dn, 2, (0, 0, 255))
                ctx.draw_shapes_enqueue(imgs, ds, B * 256, 3, B, n_ptr=dn)
            r = alternate(a.rounds, dict(boxes=lambda: timed(ctx, a.reps, boxes), pcie=lambda: roundtrip(ctx, imgs, frames, max(3, a.reps // 10))))
            one = R.shapes_from_blobs([[(int(q["x"]), int(q["y"]), int(q["w"]), int(q["h"])) for q in blobs[0]]], [256], 256, 2, (0, 0, 255))
            t0 = time.perf_counter()
            R.draw_shapes(frames[:1], one)
            host_one = (time.perf_counter() - t0) * 1e3
            emit(what="blob_boxes", W=W, H=H, batch=B, boxes_per_image=256, ms=r["boxes"][0], pcie_roundtrip_ms=r["pcie"][0], ms_rounds=r["boxes"][1],
                 pcie_rounds=r["pcie"][1], host_draw_ms_of_one_image=host_one)
            for b in (imgs, dc, db, ds, dn):
                b.free()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines_out) + "\n")


if __name__ == "__main__":
    main()
