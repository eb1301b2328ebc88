#!/usr/bin/env python3
"""Generate tests/golden/truth.npz by running the REFERENCE's own calculate_flow (src/airsim_optical_flow.py:87-107) and
Processor.analyze_radial_error (src/processor.py:267-275) on seeded inputs, with numpy.histogram2d over the reference's bins
(src/plot_radial_error.py:38-39) of what the latter saves.

Run where the reference tree is present:   python tools/gen_golden_truth.py [path to the reference's src directory]
The reference is imported in place; nothing of it is copied, only the arrays it computes are stored.  cv2 / airsim / flow_vis / imutils /
torch are not installed here: placeholder modules stand in for them (the recipe of tools/gen_golden_global_motion.py), airsim.types with
a three-field Vector3r.  numpy.save is replaced by a recorder while analyze_radial_error runs, so the two arrays the reference hands to
it are stored as they are.  Bytecode writing is disabled so a read-only reference tree is left untouched.
"""
import sys

sys.dont_write_bytecode = True
import os
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(ROOT), "reference", "src")
OUT = os.path.join(ROOT, "tests", "golden", "truth.npz")


class Vector3r:
    def __init__(self, x_val=0.0, y_val=0.0, z_val=0.0):
        self.x_val, self.y_val, self.z_val = x_val, y_val, z_val


def _placeholders():
    import matplotlib
    matplotlib.use("Agg")
    cv2 = types.ModuleType("cv2")
    cv2.TERM_CRITERIA_EPS, cv2.TERM_CRITERIA_COUNT, cv2.COLORMAP_JET, cv2.COLOR_GRAY2RGB = 2, 1, 2, 8
    cv2.VideoCapture = cv2.VideoWriter = object
    airsim, at = types.ModuleType("airsim"), types.ModuleType("airsim.types")
    at.Vector3r = Vector3r
    airsim.types = at
    for name, mod in (("cv2", cv2), ("airsim", airsim), ("airsim.types", at), ("flow_vis", types.ModuleType("flow_vis")),
                      ("imutils", types.ModuleType("imutils")), ("torch", types.ModuleType("torch"))):
        sys.modules.setdefault(name, mod)
    import numpy.lib
    if not hasattr(numpy.lib, "angle"):          # processor.py:1 imports a name numpy 2 no longer keeps there (and never uses it)
        numpy.lib.angle = np.angle
    sys.path.insert(0, REF)


def rotation(angles):
    """R = Rz Ry Rx of three angles (radians)"""
    cx, cy, cz = np.cos(angles)
    sx, sy, sz = np.sin(angles)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def view_proj(seed, W, H, angle=0.02, shift=30.0):
    """a reversed-z perspective projection (near plane 10) times a small rotation and a translation"""
    r = np.random.default_rng(seed)
    P = np.array([[1.0, 0, 0, 0], [0, W / H, 0, 0], [0, 0, 0, 10.0], [0, 0, 1.0, 0]])
    V = np.eye(4)
    V[:3, :3] = rotation(r.normal(0, angle, 3))
    V[:3, 3] = r.normal(0, shift, 3)
    return P @ V


def pixel_grid(W, H):
    """write_flow's coords (airsim_optical_flow.py:114-116)"""
    x_coords = np.tile(np.arange(W), (H, 1))
    y_coords = np.tile(np.arange(H), (W, 1)).T
    return np.stack((x_coords, y_coords)).swapaxes(0, 2)


def hist_fields(seed, W, H, mag_edges, err_edges):
    """flow, ground truth and sky whose (magnitude, error) pairs aim at the inside of bins; a tenth out of range on either axis"""
    rng = np.random.default_rng(seed)
    bm, be = rng.integers(0, len(mag_edges) - 1, (H, W)), rng.integers(0, len(err_edges) - 1, (H, W))
    tm = mag_edges[bm] + (mag_edges[1] - mag_edges[0]) * rng.uniform(0.2, 0.8, (H, W))
    te = err_edges[be] + (err_edges[1] - err_edges[0]) * rng.uniform(0.2, 0.8, (H, W))
    tm[rng.random((H, W)) < 0.1] += 10.5
    te[rng.random((H, W)) < 0.1] += 45
    ga, gm = rng.uniform(-np.pi, np.pi, (H, W)), rng.uniform(0.5, 6, (H, W))
    gt = np.stack((gm * np.cos(ga), gm * np.sin(ga)), -1).astype(np.float32)
    fa = ga + np.deg2rad(te)
    flow = np.stack((tm * np.cos(fa), tm * np.sin(fa)), -1).astype(np.float32)
    return flow, gt, rng.random((H, W)) < 0.15


def main():
    _placeholders()
    import airsim_optical_flow as ref_of
    import processor as ref_proc

    out = {}
    # ---- the reprojection: (name, W, H, depth_scale, recipe) ------------------------------------------------------------------------------
    cases = [("p97", 97, 71, 100.0, "scene"), ("p13", 13, 7, 1.0, "scene"), ("one", 1, 1, 100.0, "scene"), ("p5", 5, 3, 100.0, "scene"),
             ("ident", 16, 9, 1.0, "identity"), ("zero", 31, 17, 100.0, "zero depth"), ("allmav", 31, 17, 100.0, "all mav"),
             ("wcross", 32, 20, 1.0, "w crosses zero")]
    for k, (name, W, H, scale, recipe) in enumerate(cases):
        rng = np.random.default_rng(300 + k)
        v1, v2 = view_proj(400 + 2 * k, W, H), view_proj(401 + 2 * k, W, H)
        raw = rng.uniform(1, 200, (H, W)).astype(np.float32)                       # the .pfm's metres (image layout)
        seg = ((rng.random((H, W)) < 0.2) * rng.integers(1, 256, (H, W))).astype(np.uint8)
        disp = np.array([12.5, -3.25, 7.0]) * (k + 1) / 4
        if recipe == "identity":
            v1, v2 = np.eye(4), np.eye(4)
        elif recipe == "zero depth":
            raw[:] = 0
        elif recipe == "all mav":
            seg[:] = 255
        elif recipe == "w crosses zero":
            # inverse = identity: the ray starts at (sx, sy, 1) and runs along -z, so the world point is (sx, sy, 1 - depth); the previous
            # view's w is that z: zero where the depth is exactly 1 (infinities, and NaN on the column with sx = 0), negative behind it
            v2 = np.eye(4)
            v1 = np.array([[1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, 1.0, 0], [0, 0, 1.0, 0]])
            raw = rng.choice(np.array([0.25, 0.5, 1.0, 1.0, 1.5, 3.0], np.float32), (H, W))
            raw[:, W // 2] = 1.0                                                   # sx = 0 on that column: 0 * inf
            seg[:] = 0
            seg[::4, ::3] = 7
            disp = np.array([0.0, 0.5, 0.0])
        depth = raw.T * 100 if scale == 100.0 else raw.T.copy()                   # write_flow's float32 `.T * 100` (:135)
        assert depth.dtype == np.float32
        with np.errstate(all="ignore"):
            res = ref_of.calculate_flow(v1, v2, (W, H), pixel_grid(W, H), depth, Vector3r(*disp), seg.T)
        assert res.shape == (W, H, 2) and res.dtype == np.float64
        out.update({f"{name}_depth": raw, f"{name}_seg": seg, f"{name}_scale": np.float32(scale), f"{name}_vp1": v1, f"{name}_vp2": v2,
                    f"{name}_inv": np.linalg.inv(v2), f"{name}_disp": disp, f"{name}_result": res})
    w = out["wcross_result"]
    assert np.isinf(w).any() and np.isnan(w).any() and np.isfinite(w).any()
    out["cases"] = np.array([c[0] for c in cases])

    # ---- the radial error: what analyze_radial_error saves, and histogram2d of it --------------------------------------------------------
    mag_edges, err_edges = np.linspace(0, 10, 160), np.linspace(-20, 20, 160)      # plot_radial_error.py:38
    saved = []
    hist_cases = [("h53", 53, 37), ("h97", 97, 71)]
    for k, (name, W, H) in enumerate(hist_cases):
        flow, gt, sky = hist_fields(500 + k, W, H, mag_edges, err_edges)
        me = types.SimpleNamespace(flow_uv=flow, gt_flow_uv=gt, sky_mask=sky, frame_index=k)
        saved.clear()
        keep, np.save = np.save, lambda path, arr: saved.append(np.array(arr))
        try:
            ref_proc.Processor.analyze_radial_error(me)
        finally:
            np.save = keep
        (pair,) = saved
        assert pair.dtype == np.float32 and pair.shape[0] == 2
        counts, _, _ = np.histogram2d(pair[0], pair[1], bins=(mag_edges, err_edges))
        assert np.array_equal(counts, counts.astype(np.int64))
        out.update({f"{name}_flow": flow, f"{name}_gt": gt, f"{name}_sky": sky, f"{name}_saved": pair, f"{name}_counts": counts.astype(np.int64)})
    out["hist_cases"] = np.array([c[0] for c in hist_cases])
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
