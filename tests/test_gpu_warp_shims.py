"""The Python shims of the image warps: mavflow.warp.remap / warpAffine / warpPerspective (cv2's signatures) and Farneback.warp_flow equal
the Context calls; Detector.warp_method at 752 x 480 and at 66 x 33 equals the restatement composed with get_flow_vis / to_rgb, from a
host array and from a device handle; the chain mav_flow_homography_dev -> warp_perspective_enqueue equals the same two steps through the
host; every unsupported argument raises what the module says."""
import numpy as np
import pytest

import warp_cases as T
import warp_ref as R

pytestmark = pytest.mark.gpu
W, H = 66, 33


def test_cv2_signatures_equal_the_context_calls(mav):
    from mavflow import _lib, warp as K
    bgr = T.images(R.U8C3, W, H)[1]
    f32 = T.images(R.F32C2, W, H, nan=False)[1]
    gray = T.images(R.U8C1, W, H)[1]
    m = T.smooth_map(W, H)
    A = np.array(T.affine_matrices(W, H)[4].M)
    P = np.array(T.perspective_matrices(W, H)[-2].M)
    with _lib.Context(W, H, 1) as ctx:
        for img in (bgr, f32, gray, f32[..., 0].copy()):
            a = K.remap(img, m, None, K.INTER_LINEAR)
            assert a.tobytes() == ctx.remap(img, m).tobytes() == R.remap(img, m).tobytes() and a.shape == img.shape and a.dtype == img.dtype
            b = K.remap(img, m[..., 0].copy(), m[..., 1].copy(), K.INTER_LINEAR, borderMode=K.BORDER_CONSTANT, borderValue=0)
            assert b.tobytes() == a.tobytes() == ctx.remap(img, m[..., 0], m[..., 1]).tobytes()
            for flags, inv in ((K.INTER_LINEAR, False), (K.INTER_LINEAR | K.WARP_INVERSE_MAP, True)):
                c = K.warpAffine(img, A, (W, H), flags=flags)
                assert c.tobytes() == ctx.warp_affine(img, A, inverse_map=inv).tobytes() == R.warp_affine(img, A, 16 if inv else 0).tobytes()
                d = K.warpPerspective(img, P, (W, H), flags=flags)
                assert d.tobytes() == ctx.warp_perspective(img, P, inverse_map=inv).tobytes() == R.warp_perspective(img, P, 16 if inv else 0).tobytes()
        dst = np.zeros_like(bgr)
        assert K.warpAffine(bgr, A, (W, H), dst) is dst and dst.tobytes() == ctx.warp_affine(bgr, A).tobytes()
        with pytest.raises(TypeError):
            K.remap(f32.astype(np.float64), m, None, K.INTER_LINEAR)
        with pytest.raises(TypeError):
            ctx.warp_affine(np.zeros((H, W, 2), np.uint8), A)
        with pytest.raises(ValueError):
            ctx.warp_affine(bgr, [[1, 2, 0], [2, 4, 1]])                    # singular
        with pytest.raises(ValueError):
            ctx.remap(np.zeros((H + 1, W), np.uint8), m)


class _Cap:
    def __init__(self, frame):
        self.frame = frame

    def read(self):
        return True, self.frame


def test_farneback_warp_flow(mav):
    from mavflow.farneback import Farneback
    bgr = T.images(R.U8C3, W, H)[1]
    flow = T.flow_fields(W, H)[-1][1]
    fb = Farneback(_Cap(bgr))
    keep = flow.copy()
    res = fb.warp_flow(bgr, flow)
    assert res.shape == bgr.shape and res.dtype == np.uint8 and res.tobytes() == R.warp_flow(bgr, flow).tobytes() == fb.ctx.warp_flow(bgr, flow).tobytes()
    assert np.array_equal(flow, keep)                                       # not negated in place
    # it is cv2.remap of the reference's map
    from mavflow import warp as K
    assert res.tobytes() == K.remap(bgr, R.flow_map(flow), None, K.INTER_LINEAR).tobytes()
    # a frame of another size than the capture's
    small = T.images(R.U8C3, 37, 23)[2]
    f2 = T.flow_fields(37, 23)[-1][1]
    assert fb.warp_flow(small, f2).tobytes() == R.warp_flow(small, f2).tobytes()


class _DS:
    capture_size = (752, 480)
    ground_truth: list = []


def _field(w, h, seed):
    f = np.random.default_rng(seed).normal(0, 3, (h, w, 2)).astype(np.float32)
    f[:h // 3, :w // 3] = 0
    f[h - 2, w - 3] = (90.0, -120.0)
    return f


@pytest.mark.parametrize("size", [(752, 480), (66, 33)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("algorithm", ["HOMOGRAPHY", "AFFINE"])
def test_detector_warp_method(mav, size, algorithm):
    from mavflow import _lib, im_helpers, pipeline
    from mavflow.detector import Detector
    w, h = size
    np.random.seed(5)
    det = Detector(_DS(), getattr(Detector.Algorithm, algorithm))
    det.homography = np.array([[1.01, 0.004, -1.25], [-0.006, 0.99, 0.8], [1e-5, -2e-5, 1.0]])
    det.aff = np.array([[1.01, 0.02, -1.5], [-0.015, 0.99, 0.75]])
    flow = _field(w, h, 9)
    kind, M = (R.PERSPECTIVE, det.homography) if algorithm == "HOMOGRAPHY" else (R.AFFINE, det.aff)
    diff, mag, rec = R.warp_method(flow, M, kind)
    want = im_helpers.get_flow_vis(diff), im_helpers.to_rgb(mag)
    keep = flow.copy()
    got = det.warp_method(flow)
    assert np.array_equal(flow, keep)
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes() and got[1].shape == (h, w, 3)
    assert det.flow_diff_mag.tobytes() == mag.tobytes() and det.flow_diff.tobytes() == diff.tobytes()
    assert det.flow_diff_max == (int(rec["row"]), int(rec["col"])) == tuple(int(v) for v in np.unravel_index(mag.argmax(), mag.shape))
    with _lib.Context(w, h, 1) as ctx:
        buf = ctx.alloc(flow.nbytes).upload(flow)
        try:
            again = det.warp_method(pipeline.DeviceArray(ctx, buf.ptr, (h, w, 2), np.float32))
            assert again[0].tobytes() == want[0].tobytes() and again[1].tobytes() == want[1].tobytes()
            assert det.flow_diff_mag.tobytes() == mag.tobytes()
        finally:
            buf.free()
    if size == (66, 33):
        # a float64 field: the reference's arithmetic on the host around a float32 warp
        f64 = flow.astype(np.float64) + 1e-12
        a = det.warp_method(f64)
        assert det.flow_diff_mag.dtype == np.float64 and a[0].shape == (h, w, 3)
        stable = (R.warp_perspective if kind == R.PERSPECTIVE else R.warp_affine)(f64.astype(np.float32), M, 0)
        d = np.where(stable == 0, 0.0, f64 - stable)
        assert np.array_equal(det.flow_diff, d)


def test_fitted_homography_feeds_the_warp_without_a_host_round_trip(mav):
    import ctypes as C
    from mavflow import _lib, warp as K
    from mavflow._lib import check
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    Ht = np.array([[1.02, 0.01, -0.7], [-0.015, 0.985, 0.4], [2e-4, -1e-4, 1.0]])
    den = Ht[2, 0] * x + Ht[2, 1] * y + Ht[2, 2]
    flow = np.stack([(Ht[0, 0] * x + Ht[0, 1] * y + Ht[0, 2]) / den - x, (Ht[1, 0] * x + Ht[1, 1] * y + Ht[1, 2]) / den - y], axis=-1).astype(np.float32)
    rng = np.random.default_rng(3)
    coords = np.column_stack([rng.integers(0, W, 200), rng.integers(0, H, 200)])
    img = T.images(R.U8C3, W, H)[1]
    with _lib.Context(W, H, 1) as ctx:
        Hm, ok = ctx.flow_homography(flow[None], coords)
        assert int(ok[0]) == 1
        through_host = ctx.warp_perspective(img, Hm[0])
        assert through_host.tobytes() == R.warp_perspective(img, Hm[0], 0).tobytes()
        bufs = [ctx.alloc(flow.nbytes).upload(flow), ctx.alloc(72), ctx.alloc(4), ctx.alloc(img.nbytes).upload(img), ctx.alloc(img.nbytes)]
        try:
            df, dH, dok, dsrc, ddst = bufs
            c32 = ctx._coords(coords)
            check(ctx.lib.mav_flow_homography_dev(ctx.h, C.c_void_p(df.ptr), c32.ctypes.data_as(C.c_void_p), c32.shape[0], 1, C.c_void_p(dH.ptr), C.c_void_p(dok.ptr)))
            ctx.warp_perspective_enqueue(dsrc, K.WARP_U8C3, dH, ddst)
            assert ddst.download(np.uint8, img.shape).tobytes() == through_host.tobytes()
            assert dH.download(np.float64, (3, 3)).tobytes() == Hm[0].tobytes()
            # and the flow field itself, registered: the other enqueue twins on the same blocks
            dflow_out = ctx.alloc(flow.nbytes)
            bufs.append(dflow_out)
            ctx.warp_perspective_enqueue(df, K.WARP_F32C2, dH, dflow_out, inverse_map=True)
            assert dflow_out.download(np.float32, flow.shape).tobytes() == R.warp_perspective(flow, Hm[0], R.INVERSE_MAP).tobytes()
            ctx.warp_flow_enqueue(dsrc, K.WARP_U8C3, df, ddst)
            assert ddst.download(np.uint8, img.shape).tobytes() == R.warp_flow(img, flow).tobytes()
            dA = ctx.alloc(48).upload(np.ascontiguousarray(Hm[0][:2]))
            bufs.append(dA)
            ctx.warp_affine_enqueue(dsrc, K.WARP_U8C3, dA, ddst)
            assert ddst.download(np.uint8, img.shape).tobytes() == R.warp_affine(img, Hm[0][:2], 0).tobytes()
            ctx.remap_enqueue(dsrc, K.WARP_U8C3, df, ddst)
            assert ddst.download(np.uint8, img.shape).tobytes() == R.remap(img, flow).tobytes()
            drec = ctx.alloc(16)
            bufs.append(drec)
            ctx.warp_method_enqueue(df, dH, K.WARP_PERSPECTIVE, drec)
            assert drec.download(R.RECORD_DTYPE, (1,)).tobytes() == R.warp_method(flow, Hm[0], R.PERSPECTIVE)[2].tobytes()
        finally:
            for b in bufs:
                b.free()
