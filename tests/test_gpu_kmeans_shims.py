"""The Python shims of the clustering step on the device: mavflow.clustering.kmeans (cv2.kmeans' signature and return shapes; the same rng
seed gives the same result), Detector.clustering on a host array and on the mag / gray handle of a global-motion call (the same bytes),
and Detector.use_clustering (True: cluster_vis is clustering's image; False: flow_vec_subtract's four returns are what they were)."""
import numpy as np
import pytest

import cluster_cases as T
import global_motion_ref as GR
import kmeans_ref as R

pytestmark = pytest.mark.gpu
W, H = 66, 45                           # 990 triples; the Detector's sample border needs H > 40


def test_cv2_signature_shapes_and_seed(mav):
    from mavflow import clustering as K
    x = T.inputs("frame_66x33")["samples"][0]
    crit = (K.TERM_CRITERIA_EPS + K.TERM_CRITERIA_MAX_ITER, 10, 1.0)
    comp, labels, centers = K.kmeans(x, 8, None, crit, 10, K.KMEANS_RANDOM_CENTERS, rng=5)
    assert isinstance(comp, float) and labels.shape == (726, 1) and labels.dtype == np.int32 and centers.shape == (8, 3) and centers.dtype == np.float32
    again = K.kmeans(x, 8, None, crit, 10, K.KMEANS_RANDOM_CENTERS, rng=5)
    assert again[0] == comp and np.array_equal(again[1], labels) and again[2].tobytes() == centers.tobytes()
    # it is the restatement's result for the centres the seed draws
    ref = R.kmeans(x, K.random_centers(x, 8, 10, rng=5), 10, 1.0)
    assert np.array_equal(labels[:, 0], ref["labels"]) and centers.tobytes() == ref["centers"].tobytes()
    assert abs(comp - ref["compactness"]) <= 1e-12 * ref["compactness"]
    # criteria without the EPS bit: eps 0; without the MAX_ITER bit: 100 iterations
    init = K.random_centers(x, 4, 2, rng=6)
    no_eps = K.kmeans(x, 4, None, (K.TERM_CRITERIA_MAX_ITER, 7, 50.0), 2, 0, rng=6)
    want = R.kmeans(x, init, 7, 0.0)
    assert np.array_equal(no_eps[1][:, 0], want["labels"]) and no_eps[2].tobytes() == want["centers"].tobytes()
    no_count = K.kmeans(x, 4, None, (K.TERM_CRITERIA_EPS, 3, 1e-3), 2, 0, rng=6)
    want = R.kmeans(x, init, 100, 1e-3)
    assert max(q["iterations"] for q in want["attempts"]) > 2                 # more than criteria's count of 3 would allow
    assert np.array_equal(no_count[1][:, 0], want["labels"]) and no_count[2].tobytes() == want["centers"].tobytes()
    one_d = K.kmeans(np.arange(40, dtype=np.float32), 3, None, crit, 2, 0, rng=1)
    assert one_d[1].shape == (40, 1) and one_d[2].shape == (3, 1)


class _DS:
    capture_size = (W, H)
    ground_truth: list = []


def _detector(seed=4):
    from mavflow.detector import Detector
    np.random.seed(seed)
    det = Detector(_DS(), Detector.Algorithm.AFFINE)
    det.aff = np.array([[1.01, 0.02, -1.5], [-0.015, 0.99, 0.75]])
    return det


def _flow():
    return np.random.default_rng(12).normal(0, 3, (H, W, 2)).astype(np.float32)


def test_detector_clustering_host_array_and_handle(mav):
    from mavflow import _lib, clustering as K, pipeline
    flow = _flow()
    det = _detector()
    with _lib.Context(W, H, 1) as ctx:
        buf = ctx.alloc(flow.nbytes).upload(flow)
        try:
            det.flow_vec_subtract(None, pipeline.DeviceArray(ctx, buf.ptr, (H, W, 2), np.float32))
            mag, gray = np.array(det.flow_uv_warped_mag), np.ascontiguousarray(det.cluster_vis[..., 0])
            assert det.mag_handle is not None and det.mag_handle.shape == (H, W) and det.gray_handle.dtype == np.uint8
            for host, handle in ((mag, det.mag_handle), (gray, det.gray_handle)):
                for raw in (True, False):
                    det.cluster_rng = 21
                    a = det.clustering(host, raw)
                    det.cluster_rng = 21
                    b = det.clustering(handle, raw)
                    assert a[0].dtype == np.uint8 and a[0].shape == ((H, W) if raw else (H, W, 3))
                    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[1].shape == b[1].shape
                    assert a[1].shape == ((0,) if raw else (H, W)) and (raw or a[1].dtype == bool)
            # uint8 samples: every sum is exact, so the image is the restatement's for the centres the seed draws
            z = gray.reshape(-1, 3)
            ref = R.kmeans(z, K.random_centers(z, 8, 10, rng=21), 10, 1.0)
            det.cluster_rng = 21
            rgb, mask = det.clustering(det.gray_handle)
            want = R.paint_image(ref["labels"], ref["centers"], (H, W))
            assert np.array_equal(rgb, want[0]) and np.array_equal(mask, want[1])
            # the default generator is np.random, the one the reference's other draws use
            det.cluster_rng = None
            np.random.seed(8)
            first = det.clustering(mag, True)[0]
            np.random.seed(8)
            assert np.array_equal(first, det.clustering(mag, True)[0])
            with pytest.raises(ValueError):
                det.clustering(mag[:-1, :-1])                       # 44 x 65 values are no triples
        finally:
            det._free_dev_buffers()
            buf.free()


@pytest.mark.parametrize("device_flow", [False, True])
def test_use_clustering_switch(mav, device_flow, monkeypatch):
    from mavflow import _lib, pipeline
    from mavflow.detector import Detector
    flow = _flow()
    with _lib.Context(W, H, 1) as ctx:
        buf = ctx.alloc(flow.nbytes).upload(flow)
        dets = []
        try:
            give = (lambda: pipeline.DeviceArray(ctx, buf.ptr, (H, W, 2), np.float32)) if device_flow else (lambda: flow)
            off = _detector()
            dets.append(off)
            assert off.use_clustering is False
            with monkeypatch.context() as m:                      # off: clustering is never entered
                m.setattr(Detector, "clustering", lambda *a, **k: (_ for _ in ()).throw(AssertionError("clustering was called")))
                base = off.flow_vec_subtract(None, give())
            sub = GR.subtract(flow, off.aff)
            assert np.array_equal(base[1], np.repeat(sub["gray"][..., None], 3, axis=2)) and np.array_equal(base[2], base[1])
            assert off.cluster_vis is base[1]
            on = _detector()
            dets.append(on)
            on.use_clustering, on.cluster_rng = True, 33
            got = on.flow_vec_subtract(None, give())
            assert got[0].tobytes() == base[0].tobytes() and got[2].tobytes() == base[2].tobytes() and got[3].tobytes() == base[3].tobytes()
            on.cluster_rng = 33
            want = on.clustering(np.array(on.flow_uv_warped_mag))[0]
            assert got[1].shape == (H, W, 3) and got[1].tobytes() == want.tobytes() and on.cluster_vis is got[1]
            assert got[1].tobytes() != base[1].tobytes()
            assert on.opt_window[0] == off.opt_window[0] and on.flow_max == off.flow_max
            # and switched off again the detector returns what the untouched one does
            on.use_clustering = False
            back = on.flow_vec_subtract(None, give())
            assert all(a.tobytes() == b.tobytes() for a, b in zip(back, base))
        finally:
            for d in dets:
                d._free_dev_buffers()
            buf.free()
