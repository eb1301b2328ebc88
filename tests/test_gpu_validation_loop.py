"""Processor(validation="device"): the three FoE loops take drone_size_pixels, the box centre behind center_phi, sky_tpr / sky_fpr and
drone_flow_pixels from one Context.gt_stats call per batch and fill the FrameResults and JSON files validation="host" fills, field for
field -- with a host ground-truth flow, with device handles of it, and with the pixel list capped below the drone's size (the fallback).
The dataset is small (96x80, N = 6); its MAV patch moves, its sky and depth change per frame, its validate_sky_segment is the
reference's rule (src/datasets/dataset.py:173-175) and it declares no image constant."""
import logging

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
W, H, N = 96, 80, 6
BATCH = 3


def _dataset_class():
    from mavflow import im_helpers, pipeline
    from mavflow.processor import SyntheticDataset

    class Moving(SyntheticDataset):
        def __init__(self, results_path):
            super().__init__(W, H, N, use_farneback=False, dangle=(0.004, -0.002, 0.001), results_path=results_path)
            self.constant_segmentation = False
            self.constant_sky_segmentation = False
            self.calls = dict(validate=0)
            self._gt_dev = None

        def get_flow_uv(self, i):                               # the .flo seam: a host array, whatever get_gt_of hands out
            return self._pair(i)[2].astype(np.float32)

        def get_segmentation(self, i):
            seg = np.zeros((H, W, 3), np.uint8)
            seg[5 + 7 * i:5 + 7 * i + 12, 10 + 9 * i:10 + 9 * i + 17] = 255
            seg[H - 1 - i, 3] = 60                              # inside the box (above 0.1 * max), not a drone pixel
            return seg

        def get_depth(self, i):
            rng = np.random.default_rng(900 + i)
            d = rng.uniform(1, 99, (H, W)).astype(np.float32)
            d[i, 2 * i] = 100.0                                 # the maximum: 80.0 is the threshold by either numpy's casting
            return d

        def get_sky_segmentation(self, i):
            rng = np.random.default_rng(950 + i)
            return (self.get_depth(i) > 80) ^ (rng.random((H, W)) < 0.1)

        def validate_sky_segment(self, sky_mask, depth_buffer):
            self.calls["validate"] += 1
            sky_mask_gt = depth_buffer > 0.80 * np.max(depth_buffer)
            return im_helpers.calculate_tpr_fpr(sky_mask_gt * 255, sky_mask)

        def put_gt_on(self, ctx):
            """every frame's ground-truth flow in one block of ctx; get_gt_of then hands out device handles into it"""
            host = np.stack([SyntheticDataset.get_gt_of(self, i) for i in range(N)])
            self._gt_dev = (ctx, ctx.alloc(host.nbytes).upload(host), host[0].nbytes)

        def get_gt_of(self, i):
            if self._gt_dev is None:
                return super().get_gt_of(i)
            ctx, block, step = self._gt_dev
            return pipeline.DeviceArray(ctx, block.ptr + i * step, (H, W, 2), np.float32)

        def release(self):
            if self._gt_dev is not None:
                if self._gt_dev[0].alive:
                    self._gt_dev[1].free()
                self._gt_dev = None
            super().release()

    return Moving


def _run(loop, out_dir, validation, gt="host", max_pixels=None, spy=None):
    from mavflow import pipeline
    from mavflow.processor import Processor
    from mavflow.run_config import RunConfig
    ds = _dataset_class()(str(out_dir))
    np.random.seed(29)
    p = Processor(RunConfig(logging.getLogger("t"), ds, "", False, False, False, True, False, False, "FLOW_FOE_CLUSTERING"), validation=validation)
    try:
        if max_pixels is not None:
            p.validation_max_pixels = max_pixels
        if gt == "device":
            lanes = pipeline.auto_lanes(W, H, BATCH) if loop == "run_detection_batched" else 1
            ds.put_gt_on(p._own_ctxs(BATCH if loop == "run_detection_batched" else 1, lanes)[0])
        if spy is not None:
            spy(p)
        res = p.run_detection_batched(batch=BATCH) if loop == "run_detection_batched" else getattr(p, loop)()
        texts = [(out_dir / f"image_{i:05d}.json").read_text() for i in range(N - 1)]
        return res, texts, dict(ds.calls)
    finally:
        ds.release()
        p.release()


@pytest.mark.parametrize("loop", ["run_detection", "run_detection_staged", "run_detection_batched"])
def test_device_validation_fills_the_host_validations_results(mav, tmp_path, loop):
    base, base_texts, base_calls = _run(loop, tmp_path / "host", "host")
    assert sorted(base) == list(range(N - 1)) and base_calls["validate"] == N - 1
    for i in range(N - 1):                                       # the scene exercises every field: no NaN anywhere, a drone in every frame
        r = base[i]
        assert r.drone_size_pixels == 12 * 17 and all(np.isfinite(v) for v in (r.sky_tpr, r.sky_fpr, r.center_phi, *r.drone_flow_pixels))
        assert 0 < r.sky_tpr < 1 and 0 < r.sky_fpr < 1
    from mavflow import _lib
    seen = {}
    real = _lib.Context.gt_stats

    def counted(self, seg, *a, **k):
        seen["calls"].append(np.asarray(seg).shape[0])
        return real(self, seg, *a, **k)

    def spy(p):
        """count the gt_stats calls and make the host tail's functions fail if the device mode reaches them"""
        seen["calls"] = []
        p._segmentation = p._gt_center = None                    # not called in this mode

    try:
        _lib.Context.gt_stats = counted
        for what, kw in (("host gt", {}), ("device gt", dict(gt="device"))):
            res, texts, calls = _run(loop, tmp_path / what.replace(" ", "_"), "device", spy=spy, **kw)
            assert calls["validate"] == 0, what                  # dataset.validate_sky_segment is not called
            want = [BATCH, N - 1 - BATCH] if loop == "run_detection_batched" else [1] * (N - 1)
            assert seen["calls"] == want, (what, seen["calls"])  # ONE call per batch
            for i in range(N - 1):
                assert vars(res[i]) == vars(base[i]), (loop, what, i, vars(res[i]), vars(base[i]))
                assert type(res[i].drone_size_pixels) is type(base[i].drone_size_pixels)
                assert texts[i] == base_texts[i], (loop, what, i)
    finally:
        _lib.Context.gt_stats = real
    # the list capped below the drone's size: those frames take the host path for their pixels, same results
    res, texts, _ = _run(loop, tmp_path / "capped", "device", max_pixels=4)
    for i in range(N - 1):
        assert vars(res[i]) == vars(base[i]) and texts[i] == base_texts[i], (loop, "capped", i)
    res, texts, _ = _run(loop, tmp_path / "capped_dev", "device", gt="device", max_pixels=4)
    for i in range(N - 1):
        assert vars(res[i]) == vars(base[i]) and texts[i] == base_texts[i], (loop, "capped, device gt", i)
