"""Processor.run_detection_batched for the global-motion branch (algorithm HOMOGRAPHY) against the one-frame loop run_detection():
same windows, IoUs, final detector state and decoded PNG files.  No tolerance appears in this file."""
import logging
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, N = 160, 120, 6


def _processor(ds, **kw):
    from mavflow.detector import Detector
    from mavflow.processor import Processor
    from mavflow.run_config import RunConfig
    cfg = RunConfig(logging.getLogger("t"), ds, "", False, False, False, True, False, False, "FLOW_FOE_CLUSTERING")
    return Processor(cfg, algorithm=Detector.Algorithm.HOMOGRAPHY, **kw)


def _run(tmp, name, use_farneback, optimize, encoder, batch, dataset=None):
    """One processor through one loop form -> (processor, dataset, directory of its files); batch None: run_detection()."""
    from mavflow.processor import SyntheticDataset
    np.random.seed(17)
    ds = dataset or SyntheticDataset(W=W, H=H, N=N, use_farneback=use_farneback)
    out = str(tmp / name)
    p = _processor(ds, processed_path=out, png_encoder=encoder)
    p.detector.use_optimization = optimize
    got = p.run_detection() if batch is None else p.run_detection_batched(batch)
    assert got == {}
    return p, ds, out


def _rect(r):
    return (r.get_left(), r.get_top(), r.get_right(), r.get_bottom())


# the one-frame loop of each (use_farneback, optimize) is run once and shared (host encoder: its files are the reference's form)
_ONE = {}


@pytest.fixture(scope="module")
def one_frame(tmp_path_factory):
    def get(use_farneback, optimize):
        key = (use_farneback, optimize)
        if key not in _ONE:
            from mavflow import frame_source
            p, ds, out = _run(tmp_path_factory.mktemp("one"), "one", use_farneback, optimize, "host", None)
            try:
                det = p.detector
                _ONE[key] = dict(windows={i: _rect(r) for i, r in p.detection_windows.items()}, iou=dict(p.detection_iou),
                                 homography=det.homography.copy(), confidence=det.confidence.copy(), flow_max=tuple(det.flow_max), det_iou=det.iou,
                                 frame_index=p.frame_index, coords=det.coords.copy(),
                                 png={i: frame_source.imread(os.path.join(out, f"image_{i:05d}.png")) for i in range(N - 1)})
            finally:
                p.release()
        return _ONE[key]
    yield get
    _ONE.clear()


@pytest.mark.parametrize("encoder", ["host", "device"])
@pytest.mark.parametrize("optimize", [False, True], ids=["plain", "optimized"])
@pytest.mark.parametrize("use_farneback", [False, True], ids=["host_flow", "frames"])
@pytest.mark.parametrize("batch", [2, 8])
def test_batched_loop_equals_the_one_frame_loop(tmp_path, one_frame, batch, use_farneback, optimize, encoder):
    from mavflow import frame_source
    ref = one_frame(use_farneback, optimize)
    assert sorted(ref["windows"]) == list(range(N - 1)) and ref["frame_index"] == N - 1
    p, ds, out = _run(tmp_path, "batched", use_farneback, optimize, encoder, batch)
    try:
        det = p.detector
        assert np.array_equal(det.coords, ref["coords"])                 # same seed, same draws
        assert {i: _rect(r) for i, r in p.detection_windows.items()} == ref["windows"]
        assert p.detection_iou == ref["iou"] and p.frame_index == N - 1
        assert det.homography.tobytes() == ref["homography"].tobytes() and det.homography.shape == (3, 3)
        assert det.confidence.tobytes() == ref["confidence"].tobytes() and det.confidence.shape == ref["confidence"].shape
        assert tuple(det.flow_max) == ref["flow_max"] and det.iou == ref["det_iou"]
        assert sorted(os.listdir(out)) == [f"image_{i:05d}.png" for i in range(N - 1)]
        for i in range(N - 1):
            png = frame_source.imread(os.path.join(out, f"image_{i:05d}.png"))
            assert png.shape == (H, W, 3) and np.array_equal(png[..., 0], png[..., 1]) and np.array_equal(png[..., 1], png[..., 2]), i
            assert np.array_equal(png, ref["png"][i]), i
        assert ds._frame_cursor == N - 1                                 # one get_frame() per index
    finally:
        p.release()


def test_failing_frame_ends_the_loop_as_the_one_frame_loop_ends(tmp_path):
    from mavflow.processor import SyntheticDataset

    class Frame3Collapses(SyntheticDataset):
        """Frame 3's flow sends every pixel -- so every sampled pair -- to the point (7, 9)."""

        def get_flow_uv(self, i):
            if i != 3:
                return super().get_flow_uv(i)
            yy, xx = np.mgrid[0:H, 0:W]
            return np.stack([7.0 - xx, 9.0 - yy], axis=-1).astype(np.float32)

    state = {}
    for name, batch in (("one", None), ("b2", 2), ("b8", 8)):
        np.random.seed(17)
        ds = Frame3Collapses(W=W, H=H, N=N, use_farneback=False)
        out = str(tmp_path / name)
        p = _processor(ds, processed_path=out)
        try:
            with pytest.raises(RuntimeError, match="frame 3"):
                p.run_detection() if batch is None else p.run_detection_batched(batch)
            assert p.frame_index == 3
            p._flush_images()                                            # (the one-frame loop leaves its queued files to release())
            assert sorted(p.detection_windows) == [0, 1, 2] == sorted(p.detection_iou)
            assert sorted(os.listdir(out)) == [f"image_{i:05d}.png" for i in range(3)]
            state[name] = ({i: _rect(r) for i, r in p.detection_windows.items()}, dict(p.detection_iou), p.detector.homography.tobytes(),
                           tuple(p.detector.flow_max))
        finally:
            p.release()
    assert state["b2"] == state["one"] and state["b8"] == state["one"]


def test_other_forms_still_refuse_the_branch():
    from mavflow.processor import SyntheticDataset
    np.random.seed(17)
    ds = SyntheticDataset(W=W, H=H, N=N, use_farneback=False)
    p = _processor(ds)
    try:
        with pytest.raises(NotImplementedError, match="run_detection"):
            p.run_detection_staged()
        with pytest.raises(NotImplementedError, match=r"run_detection_batched\(batch\)"):
            p.run_detection_batched()                                    # no batch: the call keeps refusing the algorithm
        p.detector.use_sparse_of = True
        with pytest.raises(NotImplementedError, match=r"run_detection\(\)"):
            p.run_detection_batched(2)
        p.detector.use_sparse_of = False
        p.debug_mode = True
        with pytest.raises(NotImplementedError, match="debug"):
            p.run_detection_batched(2)
        p.debug_mode = False
        assert p.detection_windows == {} and p.frame_index == 0
        # a field that is not float32 is refused by name: the one-frame loop serves it

        class F64(SyntheticDataset):
            def get_flow_uv(self, i):
                return np.asarray(super().get_flow_uv(i), np.float64)

        p64 = _processor(F64(W=W, H=H, N=N, use_farneback=False))
        try:
            with pytest.raises(ValueError, match=r"run_detection\(\)"):
                p64.run_detection_batched(2)
        finally:
            p64.release()
        assert p.run_detection_batched(4) == {} and sorted(p.detection_windows) == list(range(N - 1))     # no processed_path: no files, no get_frame
        assert ds._frame_cursor == 0
    finally:
        p.release()
