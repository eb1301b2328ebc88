#!/usr/bin/env python3
"""Generate tests/golden/global_motion.npz by running the REFERENCE's own Detector.flow_vec_subtract (src/detector.py:153-202) and its
pair arithmetic (:126-128) on seeded inputs.

Run where the reference tree is present:   python tools/gen_golden_global_motion.py [path to the reference's src directory]
The reference is imported in place; nothing of it is copied, only the arrays it computes are stored.  cv2 / imutils / flow_vis / airsim
are not installed here: placeholder modules stand in for them (the recipe of tools/gen_golden.py), with cv2.cvtColor(GRAY2RGB) as channel
replication -- what it is -- and a dummy flow_vis.flow_to_color, whose images are not stored.  Detector.analyze_pyramid (cv2.resize
inside) is replaced by a recorder, so the image the reference hands to it is stored too (one of its three equal channels).  Bytecode writing is disabled so a read-only
reference tree is left untouched.
"""
import sys

sys.dont_write_bytecode = True
import os
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(ROOT), "reference", "src")
OUT = os.path.join(ROOT, "tests", "golden", "global_motion.npz")


def _placeholders():
    import matplotlib
    matplotlib.use("Agg")
    cv2 = types.ModuleType("cv2")
    cv2.TERM_CRITERIA_EPS, cv2.TERM_CRITERIA_COUNT, cv2.COLORMAP_JET, cv2.COLOR_GRAY2RGB = 2, 1, 2, 8
    cv2.VideoCapture = cv2.VideoWriter = object
    cv2.cvtColor = lambda img, code: np.repeat(np.asarray(img)[..., None], 3, axis=2)
    flow_vis = types.ModuleType("flow_vis")
    flow_vis.flow_to_color = lambda flow, convert_to_bgr=False: np.zeros(flow.shape[:2] + (3,), np.uint8)
    for name, mod in (("cv2", cv2), ("imutils", types.ModuleType("imutils")), ("flow_vis", flow_vis), ("airsim", types.ModuleType("airsim"))):
        sys.modules.setdefault(name, mod)
    sys.path.insert(0, REF)


class _Dataset:
    """Only what Detector.__init__ and flow_vec_subtract read."""
    ground_truth: list = []

    def __init__(self, W, H):
        self.capture_size = (W, H)


def main():
    _placeholders()
    import detector as ref_det
    import utils as ref_utils

    seen = []

    def recorder(self, img):
        seen.append(np.array(img))
        return (0, ref_utils.Rectangle((0, 0), (0, 0)), np.zeros(0), 0)

    ref_det.Detector.analyze_pyramid = recorder
    A = ref_det.Detector.Algorithm
    out = {}
    # (name, W, H, algorithm, matrix, flow recipe)
    Hm = np.array([[1.013, -0.021, 2.75], [0.017, 0.991, -1.5], [3e-5, -2e-5, 1.0]])
    aff = np.array([[0.98, 0.03, -4.25], [-0.025, 1.02, 3.125]])
    # random: a dense field; a number: a 16x16 block of that scale in a zero field (the stored arrays stay compressible)
    cases = [("h97", 97, 71, A.HOMOGRAPHY, Hm, "random"), ("a64", 64, 64, A.AFFINE, aff, "random"),
             ("z64", 64, 64, A.HOMOGRAPHY, np.eye(3), "zero"),
             ("t64", 64, 64, A.AFFINE, np.array([[1.0, 0.0, 2.5], [0.0, 1.0, -1.25]]), "zero"),
             ("big97", 97, 71, A.AFFINE, np.array([[1.0, 0.0, 0.5], [0.0, 1.0, 0.25]]), "1e4"),
             ("tiny64", 64, 64, A.HOMOGRAPHY, np.eye(3), "1e-30")]
    for k, (name, W, H, alg, M, recipe) in enumerate(cases):
        rng = np.random.default_rng(100 + k)
        np.random.seed(200 + k)
        det = ref_det.Detector(_Dataset(W, H), alg)
        if recipe == "random":
            flow = rng.normal(0, 3, (H, W, 2)).astype(np.float32)
        elif recipe == "zero":
            flow = np.zeros((H, W, 2), np.float32)
        else:
            flow = np.zeros((H, W, 2), np.float32)
            flow[H - 20:H - 4, W - 19:W - 3] = (rng.normal(0, 1, (16, 16, 2)) * float(recipe)).astype(np.float32)
        if alg == A.HOMOGRAPHY:
            det.homography = M
        else:
            det.aff = M
        seen.clear()
        with np.errstate(all="ignore"):
            det.flow_vec_subtract(np.zeros((H, W, 3), np.uint8), flow)
        # the reference's lines :126-128, as they stand
        coords_new = det.coords.astype(np.float64) + flow[det.sample_y, det.sample_x]
        out.update({f"{name}_flow": flow, f"{name}_M": np.asarray(M, np.float64), f"{name}_warped": det.flow_uv_warped,
                    f"{name}_mag": det.flow_uv_warped_mag, f"{name}_flow_max": np.array(det.flow_max, np.int64),
                    f"{name}_image": seen[0][..., 0]})
        if recipe != "zero":                     # (zero flow: coords_new is coords)
            out.update({f"{name}_coords": np.asarray(det.coords, np.int64), f"{name}_coords_new": coords_new})
        assert det.flow_uv_warped.dtype == np.float32 and det.flow_uv_warped_mag.dtype == np.float32 and seen[0].dtype == np.uint8
        assert np.array_equal(det.cluster_vis, seen[0]) and coords_new.dtype == np.float64
        assert seen[0].ndim == 3 and np.array_equal(seen[0][..., 0], seen[0][..., 1]) and np.array_equal(seen[0][..., 0], seen[0][..., 2])
    out["cases"] = np.array([c[0] for c in cases])
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
