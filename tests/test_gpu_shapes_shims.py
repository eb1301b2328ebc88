"""The reference's drawing calls on the device against their numpy compositions: FocusOfExpansion.draw, Detector.draw, Detector.predict,
cv2's line / rectangle / circle signatures, and one debug frame of Processor(debug_path=...) on the synthetic dataset.  The shapes
themselves are tests/shapes_ref.py's; every comparison is byte for byte."""
import logging
import os
from types import SimpleNamespace

import numpy as np
import pytest

import shapes_cases as sc
import shapes_ref as R

pytestmark = pytest.mark.gpu

W, H = sc.FRAMES[0]


def frame_of(seed, channels=3):
    return np.random.RandomState(seed).randint(0, 200, (H, W, channels)).astype(np.uint8)


def drawn(img, records):
    """tests/shapes_ref.py on one (H, W[, C]) image"""
    a = img.reshape(1, H, W, -1)
    return R.draw_shapes(a, R.table(records)).reshape(img.shape)


def test_cv2_signatures_draw_what_the_restatement_draws(mav):
    from mavflow import shapes
    img = frame_of(1)
    want = drawn(img, [R.shape(R.LINE, 0, 5, 60, 120, 9, 5, (0, 0, 255))])
    got = img.copy()
    assert shapes.line(got, (5, 60), (120, 9), (0, 0, 255), 5) is got and np.array_equal(got, want)
    want = drawn(want, [R.shape(R.RECT, 0, 20, 10, 70, 50, 2, (0, 0, 255)), R.shape(R.RECT, 0, 90, 40, 80, 30, R.FILLED, (7, 8, 9))])
    shapes.rectangle(got, (20, 10), (70, 50), (0, 0, 255), 2)
    shapes.rectangle(got, (90, 40), (80, 30), (7, 8, 9), -1)
    assert np.array_equal(got, want)
    want = drawn(want, [R.shape(R.CIRCLE, 0, 100, 20, 20, 0, R.FILLED, (0, 42, 255))])
    shapes.circle(got, (100, 20), 20, [0, 42, 255], -1)
    assert np.array_equal(got, want)
    gray = frame_of(2, 1)[..., 0]
    want = drawn(gray, [R.shape(R.LINE, 0, -5, 3, 140, 66, 3, (200,))])
    assert np.array_equal(shapes.line(gray.copy(), (-5, 3), (140, 66), 200, 3), want)
    a, b = frame_of(3), frame_of(4)
    assert np.array_equal(shapes.add(a, b), np.minimum(a.astype(np.int32) + b, 255))


def tracked_lines(n=400, seed=8):
    """lines as get_FOE_sparse leaves them: ((int32, int32), (uint16, uint16)), zero-length ones and one through the FoE among them"""
    rng = np.random.RandomState(seed)
    p = rng.randint(0, [W, H], (n, 2)).astype(np.int32)
    q = np.clip(p + rng.randint(-20, 21, (n, 2)), 0, 65535).astype(np.uint16)
    q[::50] = p[::50]
    lines = [((p[i, 0], p[i, 1]), (q[i, 0], q[i, 1])) for i in range(n)]
    lines.append(((np.int32(60), np.int32(30)), (np.uint16(70), np.uint16(30))))
    return lines


def test_focus_of_expansion_draw_equals_its_numpy_composition(mav):
    from mavflow import im_helpers
    from mavflow.focus_of_expansion import FocusOfExpansion
    np.random.seed(2)
    foe_obj = FocusOfExpansion(SimpleNamespace(total_num_corners=30, old_frame=np.zeros((H, W, 3), np.uint8)))
    foe_obj.lines = tracked_lines()
    foe_obj.mask = np.zeros((H, W, 3), np.uint8)
    frame, FoE = frame_of(5), (60.7, 30.2)
    colours = FocusOfExpansion.line_colours(foe_obj.lines, FoE, foe_obj.radial_threshold)
    assert {tuple(c) for c in colours} == {(0, 255, 0), (0, 0, 255)}
    want_frame = drawn(frame, [R.shape(R.CIRCLE, 0, 60, 30, 20, 0, R.FILLED, (0, 42, 255))])
    recs = [R.shape(R.LINE, 0, int(l[0][0]), int(l[0][1]), int(l[1][0]), int(l[1][1]), 2, c) for l, c in zip(foe_obj.lines, colours)]
    want_mask = drawn(np.zeros((H, W, 3), np.uint8), recs)
    rev_mask = drawn(np.zeros((H, W, 3), np.uint8), recs[::-1])
    assert (want_mask != rev_mask).any(axis=-1).sum() > 100                               # the lines' order decides pixels here
    got_frame = frame.copy()
    out = foe_obj.draw(got_frame, FoE)
    assert np.array_equal(got_frame, want_frame), "the disc is drawn into the frame in place"
    assert np.array_equal(foe_obj.mask, want_mask), int((foe_obj.mask != want_mask).any(axis=-1).sum())
    assert np.array_equal(out, np.minimum(want_frame.astype(np.int32) + want_mask, 255))
    assert foe_obj.time == 1 and np.array_equal(foe_obj.old_gray, im_helpers._ctx(W, H).bgr2gray(want_frame)[0])
    untouched = frame.copy()
    assert foe_obj.draw(untouched, (np.nan, 3.0)) is untouched and np.array_equal(untouched, frame) and foe_obj.time == 1


def test_detector_draw_and_predict_equal_their_numpy_compositions(mav):
    from mavflow.detector import Detector
    from mavflow.utils import Rectangle
    det = object.__new__(Detector)
    boxes = [Rectangle.from_points((24, 20), (48, 44)), Rectangle.from_points((100, 50), (140, 80)), Rectangle.from_points((-5, -5), (6, 9))]
    det.dataset = SimpleNamespace(ground_truth=boxes)
    frame = frame_of(6)
    recs = [R.shape(R.RECT, 0, *b.get_topleft_int(), *b.get_bottomright_int(), 2, (0, 0, 255)) for b in boxes]
    got = frame.copy()
    assert det.draw(got) is None and np.array_equal(got, drawn(frame, recs))
    flow = np.random.RandomState(7).randn(H, W, 2).astype(np.float32) * 2 + np.float32([9.5, -6.25])
    seg = np.zeros((H, W), bool)
    seg[20:44, 24:48] = True
    avg = np.average(flow[seg], 0)
    c = boxes[0].get_center_int()
    end = (int(c[0] + avg[0]), int(c[1] + avg[1]))
    got = frame.copy()
    det.predict(seg, flow, got)
    assert det.prediction == end and end != c
    assert np.array_equal(got, drawn(frame, [R.shape(R.LINE, 0, c[0], c[1], end[0], end[1], 5, (0, 0, 255))]))
    det.dataset = SimpleNamespace(ground_truth=[])
    got = frame.copy()
    det.draw(got)
    assert np.array_equal(got, frame)


def _processor(ds, **kw):
    from mavflow.detector import Detector
    from mavflow.processor import Processor
    from mavflow.run_config import RunConfig
    cfg = RunConfig(logging.getLogger("t"), ds, "", False, False, False, True, False, False, "FLOW_FOE_CLUSTERING")
    return Processor(cfg, algorithm=Detector.Algorithm.HOMOGRAPHY, **kw)


def test_debug_path_writes_the_reference_debug_frame(mav, tmp_path):
    """image_%05d.png at 3W x 2H against the composition of processor.py:295-299 from the Detector's own two calls (whose pictures
    come back to the host one by one) and get_flow_vis"""
    from mavflow import frame_source, im_helpers
    from mavflow.frame_result import FrameResult
    from mavflow.processor import SyntheticDataset
    w, h, n = 160, 120, 3
    np.random.seed(17)
    p = _processor(SyntheticDataset(W=w, H=h, N=n, use_farneback=False), debug_path=str(tmp_path / "dbg"))
    np.random.seed(17)
    ds = SyntheticDataset(W=w, H=h, N=n, use_farneback=False)
    q = _processor(ds)
    try:
        assert np.array_equal(p.detector.coords, q.detector.coords)
        res = p.run_detection()
        assert sorted(res) == list(range(n - 1)) and all(isinstance(r, FrameResult) for r in res.values())
        for i in range(n - 1):
            frame = ds.get_frame().copy()
            flow = ds.get_flow_uv(i)
            ds.get_annotation(i)
            q.detector.get_transformation_matrix(frame, flow)
            warped_vis, cluster_vis, _, global_vis = q.detector.flow_vec_subtract(frame, flow)
            a = frame.reshape(1, h, w, 3)
            recs = [R.shape(R.RECT, 0, *g.get_topleft_int(), *g.get_bottomright_int(), 2, (0, 0, 255)) for g in ds.ground_truth]
            assert recs
            top = np.hstack((R.draw_shapes(a, R.table(recs))[0], global_vis.astype(np.uint8), warped_vis))
            bottom = np.hstack((im_helpers.get_flow_vis(flow), global_vis.astype(np.uint8), cluster_vis))
            want = np.vstack((top, bottom))
            got = frame_source.imread(os.path.join(str(tmp_path / "dbg"), f"image_{i:05d}.png"))
            assert got is not None and got.shape == (2 * h, 3 * w, 3)
            for r in range(2):
                for c in range(3):
                    tile = (slice(r * h, (r + 1) * h), slice(c * w, (c + 1) * w))
                    assert np.array_equal(got[tile], want[tile]), (i, "tile", r, c, int((got[tile] != want[tile]).any(axis=-1).sum()))
            assert (want[:h, :w] != frame).any()                                          # the rectangle is in the picture
    finally:
        p.release()
        q.release()
