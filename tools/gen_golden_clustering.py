#!/usr/bin/env python3
"""Generate tests/golden/clustering.npz by running the REFERENCE's own Detector.clustering lines (src/detector.py:396-428) behind a
placeholder cv2.kmeans that returns given labels and centres.

Run where the reference tree is present:   python tools/gen_golden_clustering.py [path to the reference's src directory]
The reference is imported in place; nothing of it is copied, only the arrays it computes are stored.  cv2 / imutils / flow_vis / airsim
are not installed here: placeholder modules stand in for them (the recipe of tools/gen_golden_global_motion.py), with
cv2.cvtColor(GRAY2RGB) as channel replication -- what it is.  Bytecode writing is disabled so a read-only reference tree is left untouched.
"""
import sys

sys.dont_write_bytecode = True
import os

os.environ["PYTHONDONTWRITEBYTECODE"] = "1"
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(ROOT), "reference", "src")
OUT = os.path.join(ROOT, "tests", "golden", "clustering.npz")

ANSWER = {}          # what the placeholder cv2.kmeans returns, and what it was called with


def _kmeans(Z, K, best_labels, criteria, attempts, flags):
    ANSWER["call"] = dict(shape=Z.shape, dtype=Z.dtype, K=K, best_labels=best_labels, criteria=criteria, attempts=attempts, flags=flags)
    return 0.0, ANSWER["labels"], ANSWER["centers"]


def _placeholders():
    import matplotlib
    matplotlib.use("Agg")
    cv2 = types.ModuleType("cv2")
    cv2.TERM_CRITERIA_EPS, cv2.TERM_CRITERIA_COUNT, cv2.TERM_CRITERIA_MAX_ITER, cv2.COLORMAP_JET, cv2.COLOR_GRAY2RGB = 2, 1, 1, 2, 8
    cv2.KMEANS_RANDOM_CENTERS = 0
    cv2.VideoCapture = cv2.VideoWriter = object
    cv2.cvtColor = lambda img, code: np.repeat(np.asarray(img)[..., None], 3, axis=2)
    cv2.kmeans = _kmeans
    flow_vis = types.ModuleType("flow_vis")
    flow_vis.flow_to_color = lambda flow, convert_to_bgr=False: np.zeros(flow.shape[:2] + (3,), np.uint8)
    for name, mod in (("cv2", cv2), ("imutils", types.ModuleType("imutils")), ("flow_vis", flow_vis), ("airsim", types.ModuleType("airsim"))):
        sys.modules.setdefault(name, mod)
    sys.path.insert(0, REF)


def main():
    _placeholders()
    import detector as ref_det

    rng = np.random.default_rng(7)
    K = 8
    edge = np.zeros((K, 3), np.float32)
    edge[0] = (255.0, 10.0, 9.999)                     # the maximum 255: center * 255 / 255 lands on the value itself
    edge[1] = (224.999, 225.0, 225.001)                # either side of the mask's threshold
    edge[2] = (225.0, 0.0, 0.999)
    edge[3] = (224.999, 254.999, 1.0)
    edge[4] = (100.0, 99.999, 100.001)
    edge[5] = (0.001, 254.0, 253.999)
    edge[6] = (17.0, 16.999, 17.001)
    edge[7] = (128.0, 127.999, 0.0)
    # (name, image shape, centres)
    cases = [("plain", (6, 9), rng.uniform(0, 40, (K, 3)).astype(np.float32)),
             ("zero", (4, 6), np.zeros((K, 3), np.float32)),
             ("edge", (8, 9), edge),
             ("bright", (5, 12), (rng.integers(0, 256, (K, 3)) / 4).astype(np.float32))]
    out = {}
    for name, shape, centers in cases:
        n = shape[0] * shape[1] // 3
        labels = rng.integers(0, K, (n, 1)).astype(np.int32)
        labels[:K, 0] = np.arange(K)                   # every cluster is painted
        img = rng.uniform(0, 5, shape).astype(np.float32)
        ANSWER.update(labels=labels, centers=centers)
        res, empty = ref_det.Detector.clustering(None, img, True)
        call = ANSWER["call"]
        assert call["shape"] == (n, 3) and call["dtype"] == np.float32 and call["K"] == 8 and call["attempts"] == 10 and call["flags"] == 0
        assert call["best_labels"] is None and tuple(call["criteria"]) == (3, 10, 1.0)
        assert empty.shape == (0,) and res.dtype == np.uint8 and res.shape == shape
        rgb, mask = ref_det.Detector.clustering(None, img, False)
        assert rgb.dtype == np.uint8 and rgb.shape == shape + (3,) and mask.dtype == bool and mask.shape == shape
        out.update({f"{name}_labels": labels, f"{name}_centers": centers, f"{name}_shape": np.array(shape, np.int64), f"{name}_res": res,
                    f"{name}_rgb": rgb, f"{name}_mask": mask})
    out["cases"] = np.array([c[0] for c in cases])
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
