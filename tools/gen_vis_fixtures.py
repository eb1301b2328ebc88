#!/usr/bin/env python3
"""Generate tests/golden/vis.npz by running the REFERENCE's own Farneback.draw_hsv and Farneback.draw_flow on seeded fields.

Run in the build container only (needs /root/reference):   PYTHONDONTWRITEBYTECODE=1 python tools/gen_vis_fixtures.py [seed]
The reference is imported in place; nothing of it is copied.  cv2 is not installed here: a placeholder module stands in for the import
statement (SURVEY.md section 8c recipe) whose cvtColor returns its input -- so draw_hsv returns the HSV image the reference composed --
and whose polylines and circle record their arguments -- so draw_flow yields the reference-made `lines` array and circle centres.
Only data is written: the fields, the HSV images, the lines and the centres (at step 1, where the centres repeat the lines' first
points, their count, radius and thickness)."""
import os
import sys
import types

sys.dont_write_bytecode = True
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference/src"
OUT = os.path.join(ROOT, "tests", "golden", "vis.npz")
SIZES = ((66, 33), (131, 67))                    # (W, H)
HUE_MARGIN = 5e-4                                # no hue of a fixture field lies this close to a whole number (tests assert it too)


def _placeholder(calls):
    cv2 = types.ModuleType("cv2")
    cv2.VideoCapture = object
    cv2.VideoWriter = object
    cv2.COLOR_HSV2BGR = 54
    cv2.cvtColor = lambda img, code: img
    cv2.polylines = lambda img, pts, closed, colour: calls["lines"].append(np.array(pts))
    cv2.circle = lambda img, centre, radius, colour, thickness: calls["centres"].append((int(centre[0]), int(centre[1]), int(radius), int(thickness)))
    sys.modules["cv2"] = cv2
    sys.path.insert(0, REF)


def field(rng, W, H):
    """A float32 field whose vectors run across every border and have negative components, some shorter than draw_flow's threshold"""
    ang = rng.uniform(-np.pi, np.pi, (H, W))
    mag = rng.uniform(0.0, 1.0, (H, W)) ** 2 * max(W, H) * 0.8
    mag[rng.random((H, W)) < 0.25] *= 0.02                                   # a quarter of the points stay below 1
    f = np.stack([mag * np.cos(ang), mag * np.sin(ang)], -1)
    return f.astype(np.float16).astype(np.float32)                          # float32 values that two bytes hold: the file stores them as float16


def hue_margin(flow):
    h = (np.arctan2(flow[..., 1], flow[..., 0]) + np.float32(np.pi)) * np.float32(180 / np.pi / 2)
    return float(np.min(np.abs(h - np.rint(h))))


def main():
    seed = int(sys.argv[1]) if len(sys.argv) > 1 else 2026
    calls = dict(lines=[], centres=[])
    _placeholder(calls)
    import farneback as ref
    rng = np.random.default_rng(seed)
    out = dict(seed=np.int64(seed))
    for W, H in SIZES:
        flow = field(rng, W, H)
        while hue_margin(flow) < HUE_MARGIN:                                  # (a pixel in the band: draw the field again)
            flow = field(rng, W, H)
        key = f"{W}x{H}"
        assert np.array_equal(flow.astype(np.float16).astype(np.float32), flow)
        out[f"flow_{key}"] = flow.astype(np.float16)                          # tests/vis_cases.load_fixture widens it again: no bit is lost
        hsv = ref.Farneback.draw_hsv(None, flow)
        assert (hsv[..., 1] == 255).all()
        out[f"hsv_{key}"] = hsv
        for step in (8, 1):
            calls["lines"].clear(); calls["centres"].clear()
            ref.Farneback.draw_flow(None, np.zeros((H, W, 3), np.uint8), flow, step)
            assert len(calls["lines"]) == 1
            lines = calls["lines"][0]
            assert lines.dtype == np.int32 and np.array_equal(lines.astype(np.int16), lines)
            out[f"lines_{key}_step{step}"] = lines.astype(np.int16)           # the reference's int32 values, stored in two bytes each
            centres = np.array(calls["centres"], np.int32).reshape(-1, 4)
            if step == 8:                                                     # (x, y, radius, thickness) of every circle
                out[f"centres_{key}_step{step}"] = centres
            else:                                                             # the dense grid: the centres repeat lines[:, 0]; keep the count
                assert np.array_equal(centres[:, :2], out[f"lines_{key}_step{step}"][:, 0])
                out[f"circles_{key}_step{step}"] = np.array([len(centres), *np.unique(centres[:, 2]), *np.unique(centres[:, 3])], np.int32)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
