#!/usr/bin/env python3
"""Generate tests/golden/validation.npz by running the REFERENCE's own Dataset.validate_sky_segment (src/datasets/dataset.py:173-175),
im_helpers.calculate_tpr_fpr and get_simple_bounding_box (src/im_helpers.py:55-84,244-252), Detector.derotate (src/detector.py:70-117)
and the lines of its loop that use them (src/processor.py:343-347, 360) on seeded inputs.

Run where the reference tree is present:   python tools/gen_golden_validation.py [path to the reference's src directory]
The reference is imported in place; nothing of it is copied, only the arrays it computes are stored.  cv2 / airsim / flow_vis / imutils /
torch are not installed here: placeholder modules stand in for them (the recipe of tools/gen_golden_truth.py).  The reference's methods
are called on plain namespace objects that carry the attributes they read.  Bytecode writing is disabled so a read-only reference tree is
left untouched.

Every depth field has the maximum 100.0, whose threshold is 80.0 by numpy 1.x's and by numpy 2's casting rule alike, so the stored
results do not depend on the numpy that ran this (tests/test_validation_ref_cpu.py has a field on which the two rules part)."""
import sys

sys.dont_write_bytecode = True
import os
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(ROOT), "reference", "src")
OUT = os.path.join(ROOT, "tests", "golden", "validation.npz")


def _placeholders():
    import matplotlib
    matplotlib.use("Agg")
    cv2 = types.ModuleType("cv2")
    cv2.TERM_CRITERIA_EPS, cv2.TERM_CRITERIA_COUNT, cv2.COLORMAP_JET, cv2.COLOR_GRAY2RGB = 2, 1, 2, 8
    cv2.VideoCapture = cv2.VideoWriter = object
    airsim, at = types.ModuleType("airsim"), types.ModuleType("airsim.types")
    at.Vector3r = object
    airsim.types = at
    for name, mod in (("cv2", cv2), ("airsim", airsim), ("airsim.types", at), ("flow_vis", types.ModuleType("flow_vis")),
                      ("imutils", types.ModuleType("imutils")), ("torch", types.ModuleType("torch"))):
        sys.modules.setdefault(name, mod)
    import numpy.lib
    if not hasattr(numpy.lib, "angle"):
        numpy.lib.angle = np.angle
    sys.path.insert(0, REF)


def scene(seed, W, H, recipe):
    """seg (H, W) uint8, gt flow (H, W, 2) float32, sky (H, W) bool, depth (H, W) float32 with maximum 100.0"""
    rng = np.random.default_rng(seed)
    seg = rng.integers(0, 20, (H, W)).astype(np.uint8)                     # background below every threshold in use
    if recipe != "no mav":
        h, w = max(1, H // 5), max(1, W // 6)
        y0, x0 = int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1))
        seg[y0:y0 + h, x0:x0 + w] = rng.choice(np.array([128, 200, 255], np.uint8), (h, w))
        seg[rng.integers(0, H), rng.integers(0, W)] = 90                   # above 0.1 * max, below 127: in the box, not in the MAV
    if recipe == "all mav":
        seg[:] = 255
    gt = rng.normal(0, 3, (H, W, 2)).astype(np.float32)
    depth = rng.uniform(1, 99, (H, W)).astype(np.float32)
    far = rng.random((H, W)) < 0.3
    depth[far] = rng.uniform(81, 99, int(far.sum())).astype(np.float32)
    depth[rng.integers(0, H), rng.integers(0, W)] = 100.0
    sky = (depth > 80) ^ (rng.random((H, W)) < 0.1)                        # a prediction that is mostly right
    return seg, gt, sky, depth


def main():
    _placeholders()
    import detector as ref_detector
    import im_helpers as ref_im
    from datasets.dataset import Dataset as RefDataset

    out = {}
    # (name, W, H, frame index, recipe)
    cases = [("g97", 97, 71, 3, "scene"), ("g13", 13, 7, 1, "scene"), ("frame0", 31, 17, 0, "scene"), ("nomav", 16, 9, 2, "no mav"),
             ("allmav", 23, 11, 1, "all mav"), ("one", 1, 1, 1, "all mav"), ("g65", 65, 2, 5, "scene")]
    for k, (name, W, H, index, recipe) in enumerate(cases):
        seg, gt, sky, depth = scene(700 + k, W, H, recipe)
        rng = np.random.default_rng(800 + k)
        dt, ang = 1 / 30.0 + 0.001 * k, rng.normal(0, 0.01, 3)
        ds = types.SimpleNamespace(capture_size=(W, H), get_delta_time=lambda i, dt=dt: dt, get_angular_difference=lambda a, b, ang=ang: ang)
        det = types.SimpleNamespace(dataset=ds, x_coords=np.tile(np.arange(W), (H, 1)), y_coords=np.tile(np.arange(H), (W, 1)).T)   # detector.py:39-40
        derot = ref_detector.Detector.derotate(det, index - 1, index, gt)
        with np.errstate(all="ignore"):
            avg = np.average(derot[seg > 127], axis=0)                                            # processor.py:344
            sky_tpr, sky_fpr = RefDataset.validate_sky_segment(None, sky, depth)                  # processor.py:317
        box = ref_im.get_simple_bounding_box(seg)                                                 # processor.py:346
        size = np.sum(seg > 127)                                                                  # processor.py:360
        assert np.max(depth) == 100.0 and (index < 1) == (derot.dtype == np.float32)
        out.update({f"{name}_seg": seg, f"{name}_gt": gt, f"{name}_sky": sky, f"{name}_depth": depth, f"{name}_index": np.int64(index),
                    f"{name}_omega": ang / dt, f"{name}_dt": np.float64(dt), f"{name}_derotated": derot, f"{name}_avg": np.asarray(avg),
                    f"{name}_sky_rates": np.array([sky_tpr, sky_fpr], np.float64), f"{name}_size": np.int64(size),
                    f"{name}_box": np.array([*box.get_topleft(), *box.get_bottomright()], np.float64),
                    f"{name}_center": np.array(box.get_center(), np.float64)})
    out["cases"] = np.array([c[0] for c in cases])
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
