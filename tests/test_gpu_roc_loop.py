"""The threshold sweep behind the detection loops, at 160x120 and 6 frames: the armed frame step (on: the step's other bytes are
today's and the tables are a separate sweep's; disarmed: today's bytes), a step whose block is too small, and Processor(roc=...)
through the three loops -- equal counts, the (15 degrees, 1.0 px) cell reproducing every frame's tpr_fixed / fpr_fixed exactly."""
import ctypes as C
import filecmp
import logging
import os

import numpy as np
import pytest

from mavflow import synth

pytestmark = pytest.mark.gpu
W, H, N = 160, 120, 7                      # N - 1 = 6 frames
ROC = dict(angles=[2.0, 5.0, 10.0, 15.0, 20.0, 45.0, 90.0], mags=[0.25, 0.5, 1.0, 2.0])
I15, J1 = ROC["angles"].index(15.0), ROC["mags"].index(1.0)


def test_armed_frame_step(mav):
    from mavflow import _lib
    from mavflow.pipeline import DetectPipeline
    B = 3
    prev, nxt = synth.make_batch(W, H, B, distinct=B)
    samples = np.stack([synth.foe_samples(W, H, b) for b in range(B)])
    gt = [np.where(np.arange(W)[None, :] + np.arange(H)[:, None] * (b + 1) < 150, 255 * (b % 2), 128 + b).astype(np.uint8) for b in range(B)]
    runs = {}
    for worker in (True, False):                           # the posted form and mav_frame_step_dev
        with _lib.Context(W, H, B) as ctx:
            pipe = DetectPipeline(ctx, B, worker=worker, keep_flow=True)
            t = pipe.submit(samples, prev=list(prev), nxt=list(nxt), gt=gt)
            plain = pipe.collect(t)
            assert "roc" not in plain
            raw_plain = bytes(pipe.slots[t].h_out)
            assert len(raw_plain) == B * 96
            pipe.set_params(roc=ROC)
            t = pipe.submit(samples, prev=list(prev), nxt=list(nxt), gt=gt)
            on = pipe.collect(t)
            assert bytes(pipe.slots[t].h_out)[:B * 96] == raw_plain           # records and counts: today's bytes
            assert on["roc"].shape == (B, len(ROC["angles"]), len(ROC["mags"]), 4) and on["roc"].dtype == np.int64
            assert np.array_equal(on["roc"][:, I15, J1], on["counts_fixed"])   # the reference's operating point
            flow = np.stack([np.array(f) for f in on["flow"]])
            sep = ctx.roc_sweep(flow, on["results"]["foe"], np.stack(gt), ROC["angles"], ROC["mags"])["counts"]
            assert np.array_equal(on["roc"], sep)
            runs[worker] = on["roc"].tobytes()
            no_gt = pipe.collect(pipe.submit(samples, prev=list(prev), nxt=list(nxt)))      # no ground truth: no counts, no sweep
            assert "roc" not in no_gt and no_gt["counts_fixed"] is None
            # with components in front of the tables
            pipe.set_params(cc_params=dict(max_blobs=16))
            both = pipe.collect(pipe.submit(samples, prev=list(prev), nxt=list(nxt), gt=gt))
            assert np.array_equal(both["roc"], sep) and "blobs" in both
            pipe.set_params(cc_params=None, roc=None)          # disarmed: the block and its bytes are today's
            t = pipe.submit(samples, prev=list(prev), nxt=list(nxt), gt=gt)
            off = pipe.collect(t)
            assert "roc" not in off and bytes(pipe.slots[t].h_out) == raw_plain
            # armed behind the binding's back (the raw call: the pipeline cannot see it and does not re-arm): its blocks do not hold
            # the tables, the step is refused and its markers still fire
            p, _a, _m = _lib.roc_params(ROC["angles"], ROC["mags"])
            _lib.check(ctx.lib.mav_roc_arm(ctx.h, C.byref(p), B * 96))
            with pytest.raises(ValueError, match="out_bytes"):
                pipe.collect(pipe.submit(samples, prev=list(prev), nxt=list(nxt), gt=gt))
            _lib.check(ctx.lib.mav_roc_arm(ctx.h, None, 0))
            t = pipe.submit(samples, prev=list(prev), nxt=list(nxt), gt=gt)
            assert pipe.collect(t)["results"].tobytes() == plain["results"].tobytes() and bytes(pipe.slots[t].h_out) == raw_plain
            with pytest.raises(ValueError):
                pipe.set_params(roc=dict(angles=[3.0, 1.0], mags=[1.0]))
            pipe.close()
    assert runs[True] == runs[False]


def test_pipelines_that_share_a_context(mav):
    """The armed state is the context's; it follows the pipeline that submits.  Pipelines of different batches (different table
    offsets), an unarmed one in between, and closing one of them while another goes on."""
    from mavflow import _lib
    from mavflow.pipeline import DetectPipeline
    B = 4
    prev, nxt = synth.make_batch(W, H, B, distinct=B)
    samples = np.stack([synth.foe_samples(W, H, b) for b in range(B)])
    gt = [np.where(np.arange(W)[None, :] + np.arange(H)[:, None] * (b + 1) < 150, 255 * (b % 2), 128 + b).astype(np.uint8) for b in range(B)]
    other = dict(angles=[1.0, 15.0, 30.0], mags=[1.0, 3.0])
    for worker in (True, False):
        with _lib.Context(W, H, B) as ctx:
            def run(pipe, n):
                return pipe.collect(pipe.submit(samples[:n], prev=list(prev[:n]), nxt=list(nxt[:n]), gt=gt[:n]))

            first = DetectPipeline(ctx, 1, worker=worker)                   # the stale pipeline of the hand-over
            first.set_params(roc=ROC)
            want1 = run(first, 1)
            big = DetectPipeline(ctx, B, worker=worker)
            big.set_params(roc=ROC)
            want = run(big, B)
            assert np.array_equal(want["roc"][0], want1["roc"][0]) and np.array_equal(want["roc"][:, I15, J1], want["counts_fixed"])
            one = DetectPipeline(ctx, 1, worker=worker)                     # another batch: another offset of the tables
            one.set_params(roc=other)
            plain = DetectPipeline(ctx, B, worker=worker)                   # no sweep at all
            got_one = run(one, 1)
            assert got_one["roc"].shape == (1, 3, 2, 4) and np.array_equal(got_one["roc"][0, 1, 0], got_one["counts_fixed"][0])
            again = run(big, B)                                             # the batch-4 pipeline after the batch-1 one armed the context
            for key in ("results", "counts_fixed", "counts_dyn", "roc"):
                assert again[key].tobytes() == want[key].tobytes(), key
            off = run(plain, B)
            assert "roc" not in off and off["results"].tobytes() == want["results"].tobytes()
            assert off["counts_fixed"].tobytes() == want["counts_fixed"].tobytes()
            t1, t2 = (p.submit(samples[:n], prev=list(prev[:n]), nxt=list(nxt[:n]), gt=gt[:n]) for p, n in ((big, B), (one, 1)))   # both in flight
            assert big.collect(t1)["roc"].tobytes() == want["roc"].tobytes() and one.collect(t2)["roc"].tobytes() == got_one["roc"].tobytes()
            assert run(big, B)["roc"].tobytes() == want["roc"].tobytes()
            one.close()                                                     # closing a pipeline whose arming the context does not carry ...
            assert ctx.roc_state == big._roc_want()
            assert run(first, 1)["roc"].tobytes() == want1["roc"].tobytes()
            first.close()                                                   # ... and one whose arming it does carry, while `big` goes on
            assert ctx.roc_state is None
            assert run(big, B)["roc"].tobytes() == want["roc"].tobytes()
            plain.close()
            assert run(big, B)["roc"].tobytes() == want["roc"].tobytes()
            big.close()
            assert ctx.roc_state is None


def _processor(ds, **kw):
    from mavflow.processor import Processor
    from mavflow.run_config import RunConfig
    return Processor(RunConfig(logging.getLogger("t"), ds, "", False, False, False, True, False, False, "FLOW_FOE_CLUSTERING"), **kw)


def _run(tmp_path, name, loop, roc, images=False):
    from mavflow.processor import SyntheticDataset
    out_dir = tmp_path / name
    ds = SyntheticDataset(W, H, N, use_farneback=True, dangle=(0.004, -0.002, 0.001), results_path=str(out_dir))
    np.random.seed(31)
    kw = dict(roc=roc) if roc is not None else {}
    p = _processor(ds, images_path=str(out_dir / "img") if images else None, **kw)
    res = p.run_detection_batched(4) if loop == "run_detection_batched" else getattr(p, loop)()
    out = dict(res=res, roc=dict(p.roc_counts), rates=p.roc_rates() if roc is not None else None, dir=out_dir)
    p.release()
    return out


def _same_dirs(a, b):
    cmp = filecmp.dircmp(a, b)
    assert not cmp.left_only and not cmp.right_only, (cmp.left_only, cmp.right_only)
    for f in cmp.common_files:
        assert filecmp.cmp(os.path.join(a, f), os.path.join(b, f), shallow=False), f
    for d in cmp.common_dirs:
        _same_dirs(os.path.join(a, d), os.path.join(b, d))


def test_processor_roc_through_the_three_loops(mav, tmp_path):
    staged = _run(tmp_path, "staged", "run_detection_staged", ROC)
    one = _run(tmp_path, "one", "run_detection", ROC, images=True)
    batched = _run(tmp_path, "batched", "run_detection_batched", ROC)
    without = _run(tmp_path, "without", "run_detection", None, images=True)
    assert without["roc"] == {} and sorted(one["roc"]) == sorted(batched["roc"]) == sorted(staged["roc"]) == list(range(N - 1))
    ka, km = len(ROC["angles"]), len(ROC["mags"])
    for i in range(N - 1):                                  # frame 0, the float32 pair, included
        c = one["roc"][i]
        assert c.shape == (ka, km, 4) and c.dtype == np.int64
        assert np.array_equal(c, batched["roc"][i]) and np.array_equal(c, staged["roc"][i]), i
        pos, neg, tp, fp = (int(v) for v in c[I15, J1])
        r = one["res"][i]
        with np.errstate(all="ignore"):
            want = (np.float64(tp) / np.float64(pos), np.float64(fp) / np.float64(neg))
        assert np.array_equal(np.array([r.tpr_fixed, r.fpr_fixed], np.float64), np.array(want), equal_nan=True), i
        # monotone in both thresholds
        assert np.all(np.diff(c[..., 2], axis=0) <= 0) and np.all(np.diff(c[..., 2], axis=1) <= 0)
        assert np.all(np.diff(c[..., 3], axis=0) <= 0) and np.all(np.diff(c[..., 3], axis=1) <= 0)
    assert any(one["roc"][i][..., 2:].any() for i in range(N - 1))
    # results, JSON files and images do not know about the sweep
    for i in range(N - 1):
        assert vars(one["res"][i]) == vars(without["res"][i]) == vars(staged["res"][i]) == vars(batched["res"][i]), i
    _same_dirs(str(one["dir"]), str(without["dir"]))
    # roc_rates(): the numpy division of the counts
    rates = one["rates"]
    c = np.stack([one["roc"][i] for i in range(N - 1)]).astype(np.float64)
    with np.errstate(all="ignore"):
        assert np.array_equal(rates["tpr"], c[..., 2] / c[..., 0], equal_nan=True) and np.array_equal(rates["fpr"], c[..., 3] / c[..., 1], equal_nan=True)
        assert np.array_equal(rates["tpr_pooled"], c[..., 2].sum(0) / c[..., 0].sum(0), equal_nan=True)
        assert np.array_equal(rates["fpr_pooled"], c[..., 3].sum(0) / c[..., 1].sum(0), equal_nan=True)
    assert rates["tpr"].shape == (N - 1, ka, km) and rates["tpr_pooled"].shape == (ka, km)
    assert rates["angles"].tolist() == ROC["angles"] and rates["mags"].tolist() == ROC["mags"]
    for k in ("tpr", "fpr", "tpr_pooled", "fpr_pooled"):
        assert np.array_equal(rates[k], batched["rates"][k], equal_nan=True) and np.array_equal(rates[k], staged["rates"][k], equal_nan=True), k


def test_global_motion_branch_refuses_roc(mav):
    from mavflow.detector import Detector
    from mavflow.processor import Processor, SyntheticDataset
    from mavflow.run_config import RunConfig
    ds = SyntheticDataset(W, H, 3, use_farneback=True)
    p = Processor(RunConfig(logging.getLogger("t"), ds, "", False, False, False, True, False, False, "FLOW_FOE_CLUSTERING"),
                  algorithm=Detector.Algorithm.HOMOGRAPHY, roc=ROC)
    with pytest.raises(NotImplementedError):
        p.run_detection()
    with pytest.raises(NotImplementedError):
        p.run_detection_batched(2)
    p.release()
