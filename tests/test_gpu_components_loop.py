"""Connected components behind the detection calls, at 160x120 and 6 frames: components_last after detect / process_batch, the frame
step's cc fields (on: the step without them plus a separate call; zeroed: today's bytes), and Processor(blobs=...) through the three
loops.  Everything is compared for equality; the reference for blobs is tests/components_ref.py."""
import filecmp
import logging
import os

import numpy as np
import pytest

import components_ref as R
from mavflow import synth

pytestmark = pytest.mark.gpu
W, H, N = 160, 120, 7                      # N - 1 = 6 frames
CC = dict(connectivity=8, min_area=2, max_blobs=64)


def _same_cc(a, b, what):
    assert np.array_equal(a["n_components"], b["n_components"]) and np.array_equal(a["n_blobs"], b["n_blobs"]), what
    assert len(a["blobs"]) == len(b["blobs"]), what
    for k, (x, y) in enumerate(zip(a["blobs"], b["blobs"])):
        assert x.tobytes() == y.tobytes(), (what, k)
    if "labels" in a:
        assert np.array_equal(a["labels"], b["labels"]), what


def test_components_last_equals_components_of_the_downloaded_masks(mav):
    from mavflow import _lib
    B = 3
    prev, nxt = synth.make_batch(W, H, B, distinct=B)
    samples = np.stack([synth.foe_samples(W, H, b) for b in range(B)])
    with _lib.Context(W, H, B) as ctx, _lib.Context(W, H, B) as other:
        out = ctx.process_batch(prev, nxt, samples)
        for which, key in (("fixed", "mask_fixed"), ("dynamic", "mask_dyn")):
            for conn in (4, 8):
                got = ctx.components_last(B, which, connectivity=conn, labels=True)
                _same_cc(got, other.components(out[key], connectivity=conn, labels=True), ("process_batch", which, conn))
                labels, counts, _ = R.components_batch(out[key], conn, 1, 256)
                assert np.array_equal(got["labels"], labels) and np.array_equal(got["n_components"], counts["n_components"])
        det = ctx.detect(out["flow"], samples)
        _same_cc(ctx.components_last(B, "fixed", **CC), other.components(det["mask_fixed"], **CC), "detect")
        with pytest.raises(_lib.MavflowError):             # MAV_ERR_STATE: another batch; another host call in between
            ctx.components_last(B - 1)
        ctx.bbox(np.zeros((H, W), np.uint8))
        with pytest.raises(_lib.MavflowError):
            ctx.components_last(B)


def test_frame_step_with_cc_equals_the_step_without_plus_a_components_call(mav):
    from mavflow import _lib
    from mavflow.pipeline import DetectPipeline
    B = 3
    prev, nxt = synth.make_batch(W, H, B, distinct=B)
    samples = np.stack([synth.foe_samples(W, H, b) for b in range(B)])
    gt = [np.full((H, W), 255 * (b % 2), np.uint8) for b in range(B)]
    runs = {}
    for worker in (True, False):                           # the posted form and mav_frame_step_dev
        with _lib.Context(W, H, B) as ctx:
            pipe = DetectPipeline(ctx, B, worker=worker)
            t = pipe.submit(samples, prev=list(prev), nxt=list(nxt), gt=gt)
            plain = pipe.collect(t)
            assert "blobs" not in plain and "cc_counts" not in plain
            raw_plain = bytes(pipe.slots[t].h_out)            # the slot's whole result block as the step's one copy left it
            assert len(raw_plain) == B * 96
            pipe.set_params(cc_params=CC)
            on = pipe.collect(pipe.submit(samples, prev=list(prev), nxt=list(nxt), gt=gt))
            masks = np.stack([np.array(m) for m in on["mask_fixed"]])
            for key in ("results", "counts_fixed", "counts_dyn"):
                assert on[key].tobytes() == plain[key].tobytes(), key
            assert np.array_equal(masks, np.stack([np.array(m) for m in plain["mask_fixed"]]))
            sep = ctx.components(masks, **CC)
            assert np.array_equal(on["cc_counts"]["n_blobs"], sep["n_blobs"]) and np.array_equal(on["cc_counts"]["n_components"], sep["n_components"])
            for k in range(B):
                assert on["blobs"][k].tobytes() == sep["blobs"][k].tobytes(), k
                _, counts, tab = R.components(masks[k], **CC)
                assert on["blobs"][k].tobytes() == tab[:min(counts[1], CC["max_blobs"])].tobytes(), k
            runs[worker] = [b.tobytes() for b in on["blobs"]]
            pipe.set_params(cc_params=None)                # a zeroed cc: the block and its bytes are today's
            t = pipe.submit(samples, prev=list(prev), nxt=list(nxt), gt=gt)
            off = pipe.collect(t)
            assert "blobs" not in off and bytes(pipe.slots[t].h_out) == raw_plain
            # bad parameters are refused before the blocks are touched
            with pytest.raises(ValueError):
                pipe.set_params(cc_params=dict(connectivity=5))
            pipe.close()
    assert runs[True] == runs[False]


def _processor(ds, **kw):
    from mavflow.processor import Processor
    from mavflow.run_config import RunConfig
    return Processor(RunConfig(logging.getLogger("t"), ds, "", False, False, False, True, False, False, "FLOW_FOE_CLUSTERING"), **kw)


def _run(tmp_path, name, loop, blobs, images=False):
    from mavflow.processor import SyntheticDataset
    out_dir = tmp_path / name
    ds = SyntheticDataset(W, H, N, use_farneback=True, dangle=(0.004, -0.002, 0.001), results_path=str(out_dir))
    np.random.seed(31)
    kw = dict(blobs=blobs) if blobs is not None else {}
    p = _processor(ds, images_path=str(out_dir / "img") if images else None, **kw)
    masks = {}
    if loop == "run_detection_staged":
        store = p._store
        p._store = lambda i, r: (masks.__setitem__(i, np.array(p.estimate_fixed)), store(i, r))[1]
    res = p.run_detection_batched(4) if loop == "run_detection_batched" else getattr(p, loop)()
    out = dict(res=res, blobs=dict(p.detection_blobs), boxes=dict(p.detection_boxes), dir=out_dir, masks=masks)
    p.release()
    return out


def _same_dirs(a, b):
    cmp = filecmp.dircmp(a, b)
    assert not cmp.left_only and not cmp.right_only, (cmp.left_only, cmp.right_only)
    for f in cmp.common_files:
        assert filecmp.cmp(os.path.join(a, f), os.path.join(b, f), shallow=False), f
    for d in cmp.common_dirs:
        _same_dirs(os.path.join(a, d), os.path.join(b, d))


def test_processor_blobs_through_the_three_loops(mav, tmp_path):
    staged = _run(tmp_path, "staged", "run_detection_staged", CC)
    one = _run(tmp_path, "one", "run_detection", CC, images=True)
    batched = _run(tmp_path, "batched", "run_detection_batched", CC)
    without = _run(tmp_path, "without", "run_detection", None, images=True)
    assert without["blobs"] == {} and sorted(one["blobs"]) == list(range(N - 1)) == sorted(staged["masks"])

    def plain(blobs):
        return {i: [(r.topleft, r.size, a, c) for r, a, c in v] for i, v in blobs.items()}

    assert plain(one["blobs"]) == plain(batched["blobs"]) == plain(staged["blobs"])
    for i in range(N - 1):
        _, counts, tab = R.components(staged["masks"][i], **CC)
        tab = tab[:min(counts[1], CC["max_blobs"])]
        want = [((int(t["x"]), int(t["y"])), (int(t["w"]) - 1, int(t["h"]) - 1), int(t["area"]),
                 (int(t["sum_x"]) / int(t["area"]), int(t["sum_y"]) / int(t["area"]))) for t in tab]
        assert plain(one["blobs"])[i] == want, i
    # the hull of a frame's blobs (no filter) is the frame's detection box
    full = _run(tmp_path, "full", "run_detection", dict(min_area=1, max_blobs=4096))
    for i in range(N - 1):
        rects = [r for r, _, _ in full["blobs"][i]]
        box = full["boxes"][i]
        if not rects:
            assert (box.topleft, box.size) == ((-1, -1), (0, 0)), i
            continue
        x0, y0 = min(r.topleft[0] for r in rects), min(r.topleft[1] for r in rects)
        x1, y1 = max(r.get_right() for r in rects), max(r.get_bottom() for r in rects)
        assert (box.topleft, box.size) == ((x0, y0), (x1 - x0, y1 - y0)), i
    # results, JSON files and images do not know about blobs
    for i in range(N - 1):
        assert vars(one["res"][i]) == vars(without["res"][i]) == vars(staged["res"][i]) == vars(batched["res"][i]), i
    _same_dirs(str(one["dir"]), str(without["dir"]))


def test_global_motion_branch_refuses_blobs(mav):
    from mavflow.detector import Detector
    from mavflow.processor import Processor, SyntheticDataset
    from mavflow.run_config import RunConfig
    ds = SyntheticDataset(W, H, 3, use_farneback=True)
    p = Processor(RunConfig(logging.getLogger("t"), ds, "", False, False, False, True, False, False, "FLOW_FOE_CLUSTERING"),
                  algorithm=Detector.Algorithm.HOMOGRAPHY, blobs={})
    with pytest.raises(NotImplementedError):
        p.run_detection()
    with pytest.raises(NotImplementedError):
        p.run_detection_batched(2)
    p.release()


def test_get_bounding_boxes(mav):
    from mavflow import im_helpers
    img = np.zeros((H, W), np.uint8)
    assert im_helpers.get_bounding_boxes(img) == []
    img[10:20, 30:50] = 200
    img[60:61, 5:6] = 255
    img[100:110, 100:140] = 20                              # below 0.1 * max: not set, as in get_simple_bounding_box
    boxes = im_helpers.get_bounding_boxes(img)
    assert [(b.topleft, b.size) for b in boxes] == [((30, 10), (19, 9)), ((5, 60), (0, 0))]
    assert [(b.topleft, b.size) for b in im_helpers.get_bounding_boxes(img, min_area=2)] == [((30, 10), (19, 9))]
    hull = im_helpers.get_simple_bounding_box(img)
    assert hull.topleft == (5, 10) and hull.get_bottomright() == (49, 60)
    assert min(b.topleft[0] for b in boxes) == 5 and max(b.get_right() for b in boxes) == 49
