"""The Python shims of the robust affine fit: mavflow.affine.estimateAffine2D (cv2's signature and shapes, None on failure),
Detector.get_transformation_matrix for AFFINE with .affine_rng set -- from a host float32 field, a float64 field and the flow seam's device
handle -- and refused as before while it is None; and the chain flow_affine_enqueue -> mav_global_motion_dev / mav_warp_method_dev on the
M block where it is, which equals the same steps staged through the host."""
import ctypes as C

import numpy as np
import pytest

import affine_cases as T
import affine_ref as R

pytestmark = pytest.mark.gpu
W, H = 131, 67


def test_estimateAffine2D_has_cv2s_shapes(mav):
    from mavflow import affine as K
    src, dst, good = T.scene(200, 21, outliers=0.3, noise=0.3)
    M, inl = K.estimateAffine2D(src.astype(np.float32), dst.astype(np.float32), rng=4)
    assert M.shape == (2, 3) and M.dtype == np.float64 and inl.shape == (200, 1) and inl.dtype == np.uint8
    want = R.estimate_one(src.astype(np.float32).astype(np.float64), dst.astype(np.float32).astype(np.float64), T.triples_for(4, 200, 2000, 1)[0])
    assert M.tobytes() == want["M"].tobytes() and np.array_equal(inl[:, 0], want["inliers"]) and want["record"]["refined"] == 1
    sel = inl[:, 0].astype(bool)                                             # the refined M is the least-squares fit of the returned inliers
    a32, b32 = src.astype(np.float32).astype(np.float64), dst.astype(np.float32).astype(np.float64)
    ls = np.linalg.lstsq(np.column_stack([a32[sel], np.ones(sel.sum())]), b32[sel], rcond=None)[0].T
    assert np.abs(M - ls).max() <= 1e-9 * np.abs(ls).max() and inl[good].mean() > 0.95 and inl[~good].mean() < 0.1
    M3, inl3 = K.estimateAffine2D(src.reshape(-1, 1, 2), dst.reshape(-1, 1, 2), method=K.RANSAC, ransacReprojThreshold=3, maxIters=2000, confidence=0.99,
                                  refineIters=10, rng=4)                  # cv2's (n, 1, 2) layout, float64 as given
    assert M3.shape == (2, 3) and inl3.shape == (200, 1)
    M0, inl0 = K.estimateAffine2D(src, dst, refineIters=0, rng=4)
    assert np.array_equal(inl0, inl3) and M0.tobytes() != M3.tobytes()      # the mask is the minimal model's either way
    line = np.column_stack([np.arange(50.0), 3.0 * np.arange(50.0)])
    Mn, inln = K.estimateAffine2D(line, line + 1.0, rng=4)
    assert Mn is None and inln.shape == (50, 1) and not inln.any()
    with pytest.raises(NotImplementedError):
        K.estimateAffine2D(src, dst, method=K.LMEDS)


class _DS:
    capture_size = (W, H)
    ground_truth: list = []


def test_detector_affine(mav):
    from mavflow import _lib, affine as K, pipeline
    from mavflow.detector import Detector
    flow = T.flow_case(W, H, 1)[0][0]
    np.random.seed(5)
    det = Detector(_DS(), Detector.Algorithm.AFFINE)
    det.coords = np.column_stack([np.random.default_rng(1).integers(0, W, 300), np.random.default_rng(2).integers(0, H, 300)])
    det.sample_x, det.sample_y = det.coords[:, 0], det.coords[:, 1]
    with pytest.raises(NotImplementedError, match="AFFINE: cv2.estimateAffine2D"):
        det.get_transformation_matrix(None, flow)                            # affine_rng is None: what it raised before
    for alg in (Detector.Algorithm.FUNDAMENTAL, Detector.Algorithm.ESSENTIAL):
        other = Detector(_DS(), alg)
        other.affine_rng = 3
        with pytest.raises(NotImplementedError):
            other.get_transformation_matrix(None, flow)
    det.affine_rng = 17
    det.get_transformation_matrix(None, flow)
    src, dst = R.flow_pairs(flow[None], det.coords)
    want = R.estimate_one(src[0], dst[0], T.triples_for(17, 300, 2000, 1)[0])
    assert want["record"]["ok"] == 1 and want["record"]["inliers"] > 200
    assert det.aff.shape == (2, 3) and det.aff.dtype == np.float64 and det.aff.tobytes() == want["M"].tobytes()
    assert det.aff_inliers.shape == (300, 1) and det.aff_inliers.dtype == np.uint8 and np.array_equal(det.aff_inliers[:, 0], want["inliers"])
    host_aff = det.aff.copy()
    # the seam's device handle: the field is read where it is, the same bytes
    with _lib.Context(W, H, 1) as ctx:
        buf = ctx.alloc(flow.nbytes).upload(flow)
        try:
            det.aff = None
            det.get_transformation_matrix(None, pipeline.DeviceArray(ctx, buf.ptr, (H, W, 2), np.float32))
            assert det.aff.tobytes() == host_aff.tobytes()
        finally:
            buf.free()
    # a float64 field keeps its precision: the reference's own pair arithmetic, then estimate_affine
    f64 = flow.astype(np.float64) + 1e-9
    det.get_transformation_matrix(None, f64)
    new = det.coords.astype(np.float64) + f64[det.sample_y, det.sample_x]
    want64 = R.estimate_one(det.coords.astype(np.float64), new, T.triples_for(17, 300, 2000, 1)[0])
    assert det.aff.tobytes() == want64["M"].tobytes() and det.aff.tobytes() != host_aff.tobytes()
    # a Generator advances; pairs that determine no map raise
    det.affine_rng = np.random.default_rng(17)
    det.get_transformation_matrix(None, flow)
    assert det.aff.tobytes() == host_aff.tobytes()
    det.get_transformation_matrix(None, flow)                                # ... with the generator's next draw
    g = np.random.default_rng(17)
    g.random(3 * 2000)
    u = g.random(3 * 2000)
    second = K.sample_triples(type("S", (), {"random": staticmethod(lambda k: u)})(), 300, 2000)[0]
    assert det.aff.tobytes() == R.estimate_one(src[0], dst[0], second)["M"].tobytes()
    det.coords = np.column_stack([np.arange(60), np.arange(60)])
    det.sample_x = det.sample_y = np.arange(60)
    with pytest.raises(RuntimeError):
        det.get_transformation_matrix(None, flow)
    # flow_vec_subtract reads the fitted .aff
    det.aff = host_aff
    out = det.flow_vec_subtract(np.zeros((H, W, 3), np.uint8), flow)
    assert out[0].shape == (H, W, 3)


def test_fitted_affine_feeds_global_motion_and_the_warp_without_a_host_round_trip(mav):
    from mavflow import _lib, warp as K
    from mavflow._lib import MOTION_DTYPE, check
    import warp_ref
    flow, coords, tri = T.flow_case(W, H, 1, n=200, max_iters=300)
    vp = lambda b: C.c_void_p(int(b.ptr))
    with _lib.Context(W, H, 1) as ctx:
        staged = ctx.flow_affine(flow, coords, triples=tri)
        assert int(staged["ok"][0]) == 1
        gm = ctx.global_motion(flow, staged["M"])
        wm = ctx.warp_method(flow[0], staged["M"][0])
        need = ctx.estimate_affine_workspace_bytes(200, 1, 300)
        bufs = [ctx.alloc(flow.nbytes).upload(flow), ctx.alloc(tri.nbytes).upload(tri), ctx.alloc(48), ctx.alloc(200), ctx.alloc(32), ctx.alloc(need),
                ctx.alloc(MOTION_DTYPE.itemsize), ctx.alloc(W * H), ctx.alloc(16)]
        try:
            df, dt, dM, di, dr, dw, dres, dgray, drec = bufs
            ctx.flow_affine_enqueue(df, coords, 1, dt, dM, di, dr, dw, need, max_iters=300)
            check(ctx.lib.mav_global_motion_dev(ctx.h, vp(df), vp(dM), 1, 1.5, 0, None, None, vp(dgray), vp(dres)))
            ctx.warp_method_enqueue(df, dM, K.WARP_AFFINE, drec)
            assert dM.download(np.float64, (1, 2, 3)).tobytes() == staged["M"].tobytes()
            assert di.download(np.uint8, (1, 200)).tobytes() == staged["inliers"].tobytes()
            assert dr.download(R.RECORD_DTYPE, (1,)).tobytes() == staged["records"].tobytes()
            assert dres.download(MOTION_DTYPE, (1,)).tobytes() == gm["results"].tobytes()
            assert dgray.download(np.uint8, (1, H, W)).tobytes() == gm["gray"].tobytes()
            assert drec.download(warp_ref.RECORD_DTYPE, (1,)).tobytes() == wm["records"].tobytes()
            # estimate_affine_enqueue on the pairs the flow form gathered equals it
            src, dst = R.flow_pairs(flow, coords)
            ds, dd = ctx.alloc(src.nbytes).upload(src), ctx.alloc(dst.nbytes).upload(dst)
            bufs += [ds, dd]
            ctx.estimate_affine_enqueue(ds, dd, 200, 1, dt, dM, di, dr, dw, need, max_iters=300)
            assert dM.download(np.float64, (1, 2, 3)).tobytes() == staged["M"].tobytes()
        finally:
            for b in bufs:
                b.free()
