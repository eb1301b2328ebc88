"""The Python shims of the robust fundamental-matrix fit: mavflow.fundamental.findFundamentalMat (cv2's signature, shapes, argument repair
and scaling, None on failure), Detector.get_transformation_matrix for FUNDAMENTAL with .fundamental_rng set -- from a host float32 field, a
float64 field and the flow seam's device handle -- and refused as before while it is None; and the chain fit -> epipolar_residual ->
components(mask), which finds one blob whose box is the patch that moves on its own."""
import numpy as np
import pytest

import fundamental_cases as T
import fundamental_ref as R

pytestmark = pytest.mark.gpu
W, H = 131, 67


def _scaled(f):
    return f / f[2, 2] if abs(f[2, 2]) > np.finfo(np.float64).eps else f


def test_findFundamentalMat_has_cv2s_shapes(mav):
    from mavflow import fundamental as K
    src, dst, good, Ft = T.scene(200, 21, outliers=0.3, noise=0.1)
    a32, b32 = src.astype(np.float32), dst.astype(np.float32)
    Fm, mask = K.findFundamentalMat(a32, b32, rng=4)
    assert Fm.shape == (3, 3) and Fm.dtype == np.float64 and mask.shape == (200, 1) and mask.dtype == np.uint8
    want = R.find_one(a32.astype(np.float64), b32.astype(np.float64), T.subsets_for(4, 200, 1000, 1)[0])
    assert want["record"]["ok"] == 1 and Fm.tobytes() == _scaled(want["F"]).tobytes() and np.array_equal(mask[:, 0], want["inliers"])
    assert Fm[2, 2] == 1.0 and mask[good].mean() > 0.95 and mask[~good].mean() < 0.1
    F3, mask3 = K.findFundamentalMat(src.reshape(-1, 1, 2), dst.reshape(-1, 1, 2), K.FM_RANSAC, 3., 0.99, 1000, rng=4)      # cv2's (n, 1, 2) layout
    assert F3.shape == (3, 3) and mask3.shape == (200, 1)
    # the repair: a threshold <= 0 is 3, a confidence of 1 is 0.99
    Fr, maskr = K.findFundamentalMat(src, dst, K.FM_RANSAC, 0.0, 1.0, rng=4)
    assert Fr.tobytes() == F3.tobytes() and np.array_equal(maskr, mask3)
    Fs, masks = K.findFundamentalMat(src, dst, K.FM_RANSAC, 0.999, 1.0, 300, rng=4)                # the reference's literal arguments
    wants = R.find_one(src, dst, T.subsets_for(4, 200, 300, 1)[0], threshold=0.999, confidence=0.99)
    assert Fs.tobytes() == _scaled(wants["F"]).tobytes() and np.array_equal(masks[:, 0], wants["inliers"])
    pts = T.BY_NAME["no_valid"].src[0]                                        # pairs that determine no matrix
    Fn, maskn = K.findFundamentalMat(pts, pts, rng=4)
    assert Fn is None and maskn.shape == (len(pts), 1) and not maskn.any()
    with pytest.raises(NotImplementedError):
        K.findFundamentalMat(src, dst, method=K.FM_LMEDS)


class _DS:
    capture_size = (W, H)
    ground_truth: list = []


def _detector(alg):
    from mavflow.detector import Detector
    np.random.seed(5)
    det = Detector(_DS(), alg)
    _, coords, _ = T.flow_case(W, H, 1, n=300)
    det.coords = coords
    det.sample_x, det.sample_y = det.coords[:, 0], det.coords[:, 1]
    return det


def test_detector_fundamental(mav):
    from mavflow import _lib, pipeline
    from mavflow.detector import Detector
    flow = T.flow_case(W, H, 1)[0][0]
    det = _detector(Detector.Algorithm.FUNDAMENTAL)
    with pytest.raises(NotImplementedError, match="RANSAC"):
        det.get_transformation_matrix(None, flow)                            # fundamental_rng is None: what it raised before
    ess = _detector(Detector.Algorithm.ESSENTIAL)
    ess.fundamental_rng = ess.affine_rng = 3
    with pytest.raises(NotImplementedError, match="RANSAC"):
        ess.get_transformation_matrix(None, flow)                            # ESSENTIAL raises in every case
    det.fundamental_rng = 17
    det.get_transformation_matrix(None, flow)
    src, dst = R.flow_pairs(flow[None], det.coords)
    sub = T.subsets_for(17, 300, 1000, 1)[0]
    want = R.find_one(src[0], dst[0], sub, threshold=0.999, confidence=0.99)       # the reference's swapped arguments, repaired as cv2 does
    assert want["record"]["ok"] == 1 and want["record"]["inliers"] > 200
    assert det.fundamental.shape == (3, 3) and det.fundamental.dtype == np.float64 and det.fundamental.tobytes() == _scaled(want["F"]).tobytes()
    assert det.fundamental_inliers.shape == (300, 1) and det.fundamental_inliers.dtype == np.uint8
    assert np.array_equal(det.fundamental_inliers[:, 0], want["inliers"])
    host_F = det.fundamental.copy()
    res, mask = det.epipolar_residual(flow, 1.0)
    wante = R.epipolar_residual(flow[None], host_F[None], 1.0)
    assert res.tobytes() == wante["residual"][0].tobytes() and mask.tobytes() == wante["mask"][0].tobytes()
    # the seam's device handle: the field is read where it is, the same bytes
    with _lib.Context(W, H, 1) as ctx:
        buf = ctx.alloc(flow.nbytes).upload(flow)
        try:
            det.fundamental = None
            handle = pipeline.DeviceArray(ctx, buf.ptr, (H, W, 2), np.float32)
            det.get_transformation_matrix(None, handle)
            assert det.fundamental.tobytes() == host_F.tobytes()
            res2, mask2 = det.epipolar_residual(handle, 1.0)
            assert res2.tobytes() == res.tobytes() and mask2.tobytes() == mask.tobytes()
        finally:
            buf.free()
    # a float64 field keeps its precision: the reference's own pair arithmetic, then find_fundamental
    f64 = flow.astype(np.float64) + 1e-9
    det.get_transformation_matrix(None, f64)
    new = det.coords.astype(np.float64) + f64[det.sample_y, det.sample_x]
    want64 = R.find_one(det.coords.astype(np.float64), new, sub, threshold=0.999, confidence=0.99)
    assert det.fundamental.tobytes() == _scaled(want64["F"]).tobytes() and det.fundamental.tobytes() != host_F.tobytes()
    # pairs that determine no matrix raise
    det.coords = np.column_stack([np.arange(60), np.arange(60)])
    det.sample_x = det.sample_y = np.arange(60)
    with pytest.raises(RuntimeError):
        det.get_transformation_matrix(None, np.zeros((H, W, 2), np.float32))


def test_fit_residual_mask_blobs(mav):
    from mavflow import _lib
    flow, coords, sub = T.flow_case(W, H, 3)
    _, at = T.dense_scene(W, H, 3)
    with _lib.Context(W, H, 3) as ctx:
        fit = ctx.flow_fundamental(flow, coords, threshold=0.5, subsets=sub)
        assert np.all(fit["ok"] == 1)
        epi = ctx.epipolar_residual(flow, fit["F"], 1.0)
        assert np.all(epi["movers"] == T.PATCH * T.PATCH) and np.all(epi["not_finite"] == 0)
        cc = ctx.components(epi["mask"])
        for b in range(3):
            assert cc["n_blobs"][b] == 1, (b, cc["n_blobs"])
            blob = cc["blobs"][b][0]
            ys, xs = np.nonzero(epi["mask"][b])
            assert (ys.min(), ys.max(), xs.min(), xs.max()) == (at[0], at[0] + T.PATCH - 1, at[1], at[1] + T.PATCH - 1)
            assert int(blob["area"]) == T.PATCH * T.PATCH
            assert (int(blob["x"]), int(blob["y"]), int(blob["w"]), int(blob["h"])) == (at[1], at[0], T.PATCH, T.PATCH)     # the blob's box is the patch
            r, c = epi["flow_max"][b]
            assert at[0] <= r < at[0] + T.PATCH and at[1] <= c < at[1] + T.PATCH
