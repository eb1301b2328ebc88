"""The Python shims of the robust essential-matrix fit: mavflow.essential.findEssentialMat (cv2's signature and shapes, None on failure),
Detector.get_transformation_matrix for ESSENTIAL with .essential_rng set -- from Lucas-Kanade tracks, a host float32 field, a float64
field and the flow seam's device handle -- and refused as before while it is None; Detector.get_rotation; and the chain flow_essential
-> epipolar_residual(F) -> components(mask), which finds one blob whose box is the patch that moves on its own."""
import numpy as np
import pytest

import essential_cases as T
import essential_ref as R
import fundamental_cases as FC
import fundamental_ref as FR

pytestmark = pytest.mark.gpu
W, H = 131, 67


def test_findEssentialMat_has_cv2s_shapes(mav):
    from mavflow import essential as K
    src, dst, good, _ = T.scene(200, 21, outliers=0.3, noise=0.1, motion=T.STRONG)
    a32, b32 = src.astype(np.float32), dst.astype(np.float32)
    E, mask = K.findEssentialMat(a32, b32, T.K_CAM, rng=4)                     # a camera matrix in the third position
    assert E.shape == (3, 3) and E.dtype == np.float64 and mask.shape == (200, 1) and mask.dtype == np.uint8
    want = R.find_one(a32.astype(np.float64), b32.astype(np.float64), T.subsets_for(4, 200, 1000, 1)[0], 1.0, 0.999, T.CAM)
    assert want["record"]["ok"] == 1 and E.tobytes() == want["E"].tobytes() and np.array_equal(mask[:, 0], want["inliers"])
    assert mask[good].mean() > 0.95 and mask[~good].mean() < 0.1
    # cv2's second overload with its (n, 1, 2) layout: focal, pp, method, prob, threshold, maxIters
    E2, mask2 = K.findEssentialMat(src.reshape(-1, 1, 2), dst.reshape(-1, 1, 2), T.LITERAL[0], (0., 0.), K.RANSAC, 0.999, 1.0, 300, rng=4)
    want2 = R.find_one(src, dst, T.subsets_for(4, 200, 300, 1)[0], 1.0, 0.999, T.LITERAL)
    assert E2.shape == (3, 3) and mask2.shape == (200, 1) and E2.tobytes() == want2["E"].tobytes() and np.array_equal(mask2[:, 0], want2["inliers"])
    pts = T.BY_NAME["no_valid"].src[0]                                        # pairs that determine no matrix
    En, maskn = K.findEssentialMat(pts, pts, rng=4)
    assert En is None and maskn.shape == (len(pts), 1) and not maskn.any()
    E4, mask4 = K.findEssentialMat(src[:4], dst[:4], rng=4)
    assert E4 is None and mask4.shape == (4, 1) and not mask4.any()
    with pytest.raises(NotImplementedError):
        K.findEssentialMat(src, dst, method=K.LMEDS)


class _DS:
    capture_size = (W, H)
    ground_truth: list = []


class _Tracks:
    """a Lucas-Kanade tracker that returns given tracks"""

    def __init__(self, old, new):
        self.old, self.new = old, new

    def get_features(self, frame):
        return self.old, self.new, None


def _detector(alg):
    from mavflow.detector import Detector
    np.random.seed(5)
    det = Detector(_DS(), alg)
    _, coords, _ = FC.flow_case(W, H, 1, n=300)
    det.coords = coords
    det.sample_x, det.sample_y = det.coords[:, 0], det.coords[:, 1]
    return det


def test_detector_essential(mav):
    from mavflow import _lib, pipeline
    from mavflow.detector import Detector
    flow = FC.flow_case(W, H, 1)[0][0]
    det = _detector(None)                                                    # the reference's default algorithm
    assert det.algorithm == Detector.Algorithm.ESSENTIAL and det.essential_rng is None
    with pytest.raises(NotImplementedError, match="RANSAC"):
        det.get_transformation_matrix(None, flow)                            # essential_rng is None: what it raised before
    det.essential_rng = 17
    det.get_transformation_matrix(None, flow)
    cam = (float(det.focal_length), float(det.focal_length), 0.0, 0.0)       # the reference's literal arguments
    src, dst = FR.flow_pairs(flow[None], det.coords)
    sub = T.subsets_for(17, 300, 1000, 1)[0]
    want = R.find_one(src[0], dst[0], sub, 1.0, 0.999, cam)
    assert want["record"]["ok"] == 1 and want["record"]["inliers"] > 200
    assert det.essential.shape == (3, 3) and det.essential.dtype == np.float64 and det.essential.tobytes() == want["E"].tobytes()
    assert det.essential_inliers.shape == (300, 1) and det.essential_inliers.dtype == np.uint8
    assert np.array_equal(det.essential_inliers[:, 0], want["inliers"]) and det.essential_F.tobytes() == want["F"].tobytes()
    host_E = det.essential.copy()
    # get_rotation: two Euler triples in degrees and a (3, 1) vector
    e1, e2, t = det.get_rotation(flow)
    assert e1.shape == (3,) and e2.shape == (3,) and t.shape == (3, 1) and np.isfinite(np.concatenate([e1, e2, t[:, 0]])).all()
    assert abs(np.sqrt((t * t).sum()) - 1.0) < 1e-12
    # epipolar_residual works from .essential_F
    res, mask = det.epipolar_residual(flow, 1.0)
    wante = FR.epipolar_residual(flow[None], want["F"][None], 1.0)
    assert res.tobytes() == wante["residual"][0].tobytes() and mask.tobytes() == wante["mask"][0].tobytes()
    # the seam's device handle: the field is read where it is, the same bytes
    with _lib.Context(W, H, 1) as ctx:
        buf = ctx.alloc(flow.nbytes).upload(flow)
        try:
            det.essential = None
            handle = pipeline.DeviceArray(ctx, buf.ptr, (H, W, 2), np.float32)
            det.get_transformation_matrix(None, handle)
            assert det.essential.tobytes() == host_E.tobytes()
            res2, mask2 = det.epipolar_residual(handle, 1.0)
            assert res2.tobytes() == res.tobytes() and mask2.tobytes() == mask.tobytes()
        finally:
            buf.free()
    # a float64 field keeps its precision: the reference's own pair arithmetic, then find_essential
    f64 = flow.astype(np.float64) + 1e-9
    det.get_transformation_matrix(None, f64)
    new = det.coords.astype(np.float64) + f64[det.sample_y, det.sample_x]
    want64 = R.find_one(det.coords.astype(np.float64), new, sub, 1.0, 0.999, cam)
    assert det.essential.tobytes() == want64["E"].tobytes() and det.essential.tobytes() != host_E.tobytes()
    # Lucas-Kanade tracks, when there are any, are the pairs
    old, new = T.scene(120, 33, outliers=0.2, noise=0.1, motion=T.STRONG)[:2]
    det.use_sparse_of, det.lucas_kanade = True, _Tracks(old.astype(np.float32), new.astype(np.float32))
    det.get_transformation_matrix(np.zeros((H, W, 3), np.uint8), flow)
    wantlk = R.find_one(old.astype(np.float32).astype(np.float64), new.astype(np.float32).astype(np.float64), T.subsets_for(17, 120, 1000, 1)[0],
                        1.0, 0.999, cam)
    assert wantlk["record"]["ok"] == 1 and det.essential.tobytes() == wantlk["E"].tobytes() and det.essential_inliers.shape == (120, 1)
    det.use_sparse_of = False
    # pairs that determine no matrix raise
    det.coords = np.column_stack([np.ones(60, np.int64), np.ones(60, np.int64)])
    det.sample_x = det.sample_y = np.ones(60, np.int64)
    with pytest.raises(RuntimeError):
        det.get_transformation_matrix(None, np.zeros((H, W, 2), np.float32))


def test_fit_residual_mask_blobs(mav):
    from mavflow import _lib
    flow, coords, sub, cam = T.flow_case(W, H, 3)
    _, at = FC.dense_scene(W, H, 3)
    with _lib.Context(W, H, 3) as ctx:
        fit = ctx.flow_essential(flow, coords, threshold=0.5, subsets=sub, camera=cam)
        assert np.all(fit["ok"] == 1)
        epi = ctx.epipolar_residual(flow, fit["F"], 1.0)
        assert np.all(epi["movers"] == FC.PATCH * FC.PATCH) and np.all(epi["not_finite"] == 0)
        cc = ctx.components(epi["mask"])
        for b in range(3):
            assert cc["n_blobs"][b] == 1, (b, cc["n_blobs"])
            blob = cc["blobs"][b][0]
            ys, xs = np.nonzero(epi["mask"][b])
            assert (ys.min(), ys.max(), xs.min(), xs.max()) == (at[0], at[0] + FC.PATCH - 1, at[1], at[1] + FC.PATCH - 1)
            assert int(blob["area"]) == FC.PATCH * FC.PATCH
            assert (int(blob["x"]), int(blob["y"]), int(blob["w"]), int(blob["h"])) == (at[1], at[0], FC.PATCH, FC.PATCH)     # the blob's box is the patch
            r, c = epi["flow_max"][b]
            assert at[0] <= r < at[0] + FC.PATCH and at[1] <= c < at[1] + FC.PATCH
