"""Which bytes the kernels read: the layer above them (mavflow/pipeline.py: FlowStage, LanedFlowStage, DetectPipeline, and the
worker thread behind mav_frame_step_post / _wait / mav_worker_drain) pinned against the synchronous path.

The kernels are pinned elsewhere; here the reference is the plain call -- ctx.farneback for a flow, ctx.detect / process_batch for
records, both masks and counts -- run on PRIVATE COPIES of the inputs in a context of its own.  Every comparison is bit for bit.

A  caller buffers: flow_of / flow_next have read their frames when they return (a capture that decodes into one buffer refills it at
   once); DetectPipeline.submit is zero-copy and reads its arrays until collect returns, after which the same objects may be refilled;
   sky_shared / gt_shared are keyed by object identity.
B  failed steps: a failure is reported once per channel (its ticket, one drain), a failed step leaves nothing enqueued behind the
   host buffers it is given back, and the pipeline recovers and closes.  Every failure here is a host-side argument refusal."""
import ctypes as C
import logging

import numpy as np
import pytest

from mavflow import synth

pytestmark = pytest.mark.gpu
SHAPES = [(256, 192), (320, 240), (333, 217)]


def _frames(W, H, n, seed, color):
    """n distinct seeded frames: gray (H, W) or BGR (H, W, 3) whose three channels differ."""
    seq = synth.make_sequence(W, H, n, seed=seed, k=0.006)
    if color == "gray":
        return [np.ascontiguousarray(f) for f in seq]
    return [np.ascontiguousarray(np.stack([f, np.roll(f, 5, axis=1), 255 - np.roll(f, 3, axis=0)], axis=2)) for f in seq]


class _Ref:
    """The synchronous path on private copies, in a context of its own."""

    def __init__(self, W, H, B=1):
        from mavflow import _lib
        self.ctx = _lib.Context(W, H, B)

    def gray(self, f):
        return f.copy() if f.ndim == 2 else self.ctx.bgr2gray(f.copy())[0].copy()

    def flow(self, a, b):
        return self.ctx.farneback(self.gray(a)[None], self.gray(b)[None])[0].copy()

    def detect(self, flows, smp, sky=None, gt=None):
        """records, masks and (with gt: one image per pair) the counts of both masks for a (B, H, W, 2) flow."""
        flows = np.array(flows, np.float32)
        d = self.ctx.detect(flows, np.asarray(smp).copy(), sky=None if sky is None else np.array(sky))
        out = dict(results=d["results"].copy(), mask_fixed=d["mask_fixed"].copy(), mask_dyn=d["mask_dyn"].copy())
        if gt is not None:
            for m, key in (("mask_fixed", "counts_fixed"), ("mask_dyn", "counts_dyn")):
                out[key] = np.stack([self.ctx.tpr_fpr_counts(np.array(gt[k]), out[m][k:k + 1].view(np.uint8), 255)[0]
                                     for k in range(len(flows))])
        return out

    def close(self):
        self.ctx.close()


def _processor(ds):
    from mavflow.processor import Processor
    from mavflow.run_config import RunConfig
    return Processor(RunConfig(logging.getLogger("t"), ds, "", False, False, False, True, False, False, "FLOW_FOE_CLUSTERING"))


def _same(got, ref, tag):
    assert got["results"].tobytes() == ref["results"].tobytes(), tag
    for k in range(len(ref["results"])):
        assert np.array_equal(got["mask_fixed"][k], ref["mask_fixed"][k]), (tag, k)
        assert np.array_equal(got["mask_dyn"][k], ref["mask_dyn"][k]), (tag, k)
    for key in ("counts_fixed", "counts_dyn"):
        if key in ref:
            assert np.array_equal(got[key], ref[key]), (tag, key)


# ---- A. caller buffers -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("color", ["gray", "bgr"])
@pytest.mark.parametrize("W,H", SHAPES)
def test_flow_of_has_read_its_frames_when_it_returns(mav, W, H, color):
    """A1: one pair of persistent buffers, refilled with other frames right after every flow_of, before anybody reads the handle.
    The handle still holds the flow of the pair handed in -- read on the spot, settled by the next flow_of, or taken into the fused
    step of a DetectPipeline (records and masks == ctx.detect of the reference flow), with the step posted or enqueued in place."""
    from mavflow import _lib
    from mavflow.pipeline import DetectPipeline, FlowStage
    fr = _frames(W, H, 8, seed=W, color=color)
    junk = _frames(W, H, 2, seed=W + 99, color=color)
    smp = synth.foe_samples(W, H, 3)
    ref = _Ref(W, H)
    flow = {(a, b): ref.flow(fr[a], fr[b]) for a, b in ((0, 1), (1, 2), (2, 3), (3, 4), (4, 5), (6, 7))}
    with _lib.Context(W, H, 1) as ctx:
        stage = FlowStage(ctx)
        bp, bn = np.empty_like(fr[0]), np.empty_like(fr[0])

        def flow_of(a, b):
            np.copyto(bp, fr[a]); np.copyto(bn, fr[b])
            h = stage.flow_of(bp, bn)
            assert h._deferred is not None
            np.copyto(bp, junk[0]); np.copyto(bn, junk[1])           # the capture decodes the next frames into the same buffers
            return h

        h = flow_of(0, 1)
        assert np.asarray(h).tobytes() == flow[0, 1].tobytes(), "read"
        h1 = flow_of(1, 2)
        h2 = flow_of(2, 3)                                           # settles h1 (held): computed now, from what flow_of was given
        assert h1._deferred is None and h2._deferred is not None
        assert np.asarray(h1).tobytes() == flow[1, 2].tobytes(), "settled by the next flow_of"
        det = {ab: ref.detect(flow[ab][None], smp[None]) for ab in ((2, 3), (3, 4), (4, 5))}
        for worker in (True, False):
            # (more fused steps than the stage has snapshot blocks: a block is refilled after the step that gathered it has read it)
            pipe = DetectPipeline(ctx, 1, worker=worker)
            for j in range(FlowStage.SNAP + 2):
                ab = (2, 3) if j == 0 else ((3, 4), (4, 5))[j % 2]
                if j or not worker:
                    h2 = flow_of(*ab)
                out = pipe.collect(pipe.submit(smp, flow=h2))
                _same(out, det[ab], ("fused step", worker, j))
                assert np.asarray(h2).tobytes() == flow[ab].tobytes(), ("the handle of the fused step", worker, j)
            pipe.close()
        # more calls than the stage has snapshot blocks, every handle held and read at the end
        hs = [flow_of(a, b) for a, b in ((4, 5), (6, 7)) * FlowStage.SNAP]
        for k, h in enumerate(hs):
            assert np.asarray(h).tobytes() == flow[(4, 5) if k % 2 == 0 else (6, 7)].tobytes(), k
        stage.close()
    ref.close()


@pytest.mark.parametrize("color", ["gray", "bgr"])
@pytest.mark.parametrize("W,H", SHAPES)
def test_flow_next_has_read_its_frame_when_it_returns(mav, W, H, color):
    """A2: video mode from ONE persistent frame buffer, refilled before every call.  Handles read late, one dropped unread (its frame
    is still the next pair's prev), one taken into a fused step: every flow is the flow of the true frame sequence."""
    from mavflow import _lib
    from mavflow.pipeline import DetectPipeline, FlowStage
    n = 10
    fr = _frames(W, H, n, seed=W + 1, color=color)
    smp = synth.foe_samples(W, H, 4)
    ref = _Ref(W, H)
    flow = [ref.flow(fr[k], fr[k + 1]) for k in range(n - 1)]
    with _lib.Context(W, H, 1) as ctx:
        stage, pipe = FlowStage(ctx), DetectPipeline(ctx, 1)
        buf = np.empty_like(fr[0])
        np.copyto(buf, fr[0])
        assert stage.flow_next(buf) is None
        kept = {}
        for k in range(1, n):
            np.copyto(buf, fr[k])
            h = stage.flow_next(buf)
            if k == 3:
                del h                                                # dropped unread
            elif k == 5:
                out = pipe.collect(pipe.submit(smp, flow=h))
                _same(out, ref.detect(flow[k - 1][None], smp[None]), "fused step")
                kept[k] = h
            else:
                kept[k] = h
        buf[...] = 0
        for k, h in kept.items():
            assert np.asarray(h).tobytes() == flow[k - 1].tobytes(), k
        pipe.close(); stage.close()
    ref.close()


def test_laned_stage_and_the_processor_loop_from_one_capture_buffer(mav):
    """A3: LanedFlowStage over 2 contexts fed from one reused pair of capture buffers: each lane's deferred flow is settled one call
    later on that lane, after the buffers have been refilled twice.  Then the Processor loop with a get_flow_uv doing the same: flows
    and FrameResults equal the run that hands in a fresh array per frame."""
    from mavflow import _lib, pipeline
    from mavflow.processor import SyntheticDataset
    W, H, n = 320, 240, 7
    pairs = [synth.make_pair(W, H, 40 + i)[:2] for i in range(n)]
    ref = _Ref(W, H)
    flow = [ref.flow(p, q) for p, q in pairs]
    ref.close()
    ctxs = [_lib.Context(W, H, 1) for _ in range(2)]
    stage = pipeline.LanedFlowStage(ctxs)
    cap = (np.empty((H, W), np.uint8), np.empty((H, W), np.uint8))
    hs = []
    for p, q in pairs:
        np.copyto(cap[0], p); np.copyto(cap[1], q)
        hs.append(stage.flow_of(*cap))
    cap[0][...] = 0; cap[1][...] = 0
    for i, h in enumerate(hs):
        assert np.asarray(h).tobytes() == flow[i].tobytes(), i
    stage.close()
    for c in ctxs:
        c.close()

    class Capture(SyntheticDataset):
        """get_flow_uv as a capture that decodes every frame into the same two buffers."""

        def get_flow_uv(self, i):
            f0, f1, _ = self._pair(i)
            if self._stage is None:
                self._ctxs = [_lib.Context(W, H, 1) for _ in range(self.lanes)]
                self._stage = pipeline.LanedFlowStage(self._ctxs)
                self._cap = (np.empty_like(f0), np.empty_like(f1))
            np.copyto(self._cap[0], f0); np.copyto(self._cap[1], f1)
            return self._stage.flow_of(*self._cap)

    runs = {}
    for cls in (SyntheticDataset, Capture):
        ds = cls(W, H, 9, use_farneback=True, dangle=(0.002, -0.001, 0.003), lanes=2, seed=6)
        seen = []
        get = ds.get_flow_uv
        ds.get_flow_uv = lambda i, get=get: seen.append(get(i)) or seen[-1]
        np.random.seed(21)
        p = _processor(ds)
        res = p.run_detection()
        runs[cls.__name__] = (res, [np.array(h) for h in seen])
        p.release()
    (a, fa), (b, fb) = runs["SyntheticDataset"], runs["Capture"]
    assert sorted(a) == sorted(b) == list(range(8))
    for i in range(8):
        assert fa[i].tobytes() == fb[i].tobytes(), i
        assert vars(a[i]) == vars(b[i]), i


@pytest.mark.parametrize("worker", [True, False])
def test_submit_arrays_may_be_refilled_once_collect_has_returned(mav, worker):
    """A4: the same frame, flow, sky and gt array objects, refilled after every collect and submitted again, give the reference
    result for their new content.  (Overwriting them BEFORE collect is the caller's bug: not tested, it would assert a race.)"""
    from mavflow import _lib
    from mavflow.pipeline import DetectPipeline
    W, H, B = 333, 217, 3
    smp = np.stack([synth.foe_samples(W, H, b) for b in range(B)])
    ref = _Ref(W, H, B)
    prev, nxt = [np.empty((H, W), np.uint8) for _ in range(B)], [np.empty((H, W), np.uint8) for _ in range(B)]
    flows = [np.empty((H, W, 2), np.float32) for _ in range(B)]
    sky, gt = [np.empty((H, W), bool) for _ in range(B)], [np.empty((H, W), np.uint8) for _ in range(B)]
    rng = np.random.default_rng(11)
    with _lib.Context(W, H, B) as ctx:
        pipe = DetectPipeline(ctx, B, worker=worker)
        for r in range(4):                                           # more rounds than the pipeline has slots
            p0, n0 = synth.make_batch(W, H, B + r, distinct=B + r)
            for k in range(B):
                np.copyto(prev[k], p0[r + k]); np.copyto(nxt[k], n0[r + k])
                np.copyto(flows[k], synth.synthetic_flow(W, H, seed=10 * r + k))
                sky[k][...] = False
                sky[k][:5 + 9 * r + 3 * k] = True
                np.copyto(gt[k], (rng.integers(0, 2, (H, W)) * 255).astype(np.uint8))
            f_ref = ref.ctx.farneback(np.stack(prev), np.stack(nxt)).copy()
            got = pipe.collect(pipe.submit(smp, prev=prev, nxt=nxt, sky=sky, gt=gt))
            _same(got, ref.detect(f_ref, smp, sky=np.stack(sky), gt=[g.copy() for g in gt]), ("frames", r))
            got = pipe.collect(pipe.submit(smp, flow=flows, sky=sky, gt=gt))
            _same(got, ref.detect(np.stack(flows), smp, sky=np.stack(sky), gt=[g.copy() for g in gt]), ("host flow", r))
        pipe.close()
    ref.close()


@pytest.mark.parametrize("worker", [True, False])
def test_shared_images_are_taken_at_first_use_and_keyed_by_identity(mav, worker):
    """A5, the contract of sky_shared / gt_shared: the device copy is taken the first time an object is seen and is a real copy; an
    in-place edit of that object is NOT seen (the run's constant images are uploaded once), a new object is."""
    from mavflow import _lib
    from mavflow.pipeline import DetectPipeline
    W, H = 320, 240
    smp = synth.foe_samples(W, H, 1)
    f = synth.synthetic_flow(W, H, seed=3)
    sky_b = np.zeros((H, W), bool)                                   # bool: cached through a u8 view of the same memory
    sky_b[:40] = True
    sky_u = np.zeros((H, W), np.uint8)                               # contiguous u8: the cache holds the very object
    sky_u[:, :50] = 1
    gt = np.zeros((H, W), np.uint8)
    gt[60:120, 100:180] = 255
    ref = _Ref(W, H)
    with _lib.Context(W, H, 1) as ctx:
        for sky in (sky_b, sky_u):
            pipe = DetectPipeline(ctx, 1, worker=worker)
            first = (sky.copy(), gt.copy())
            expect = ref.detect(f[None], smp[None], sky=first[0][None], gt=[first[1]])
            _same(pipe.collect(pipe.submit(smp, flow=[f], sky_shared=sky, gt_shared=gt)), expect, "first use")
            sky[...] = 0                                             # in place: not seen
            sky[100:] = 1
            gt[...] = 255 - gt
            _same(pipe.collect(pipe.submit(smp, flow=[f], sky_shared=sky, gt_shared=gt)), expect, "edited in place")
            new_sky, new_gt = sky.copy(), gt.copy()                  # new objects: seen
            expect2 = ref.detect(f[None], smp[None], sky=new_sky[None], gt=[new_gt])
            assert expect2["results"].tobytes() != expect["results"].tobytes() or not np.array_equal(expect2["counts_fixed"], expect["counts_fixed"])
            _same(pipe.collect(pipe.submit(smp, flow=[f], sky_shared=new_sky, gt_shared=new_gt)), expect2, "new objects")
            pipe.close()
            gt[...] = 255 - gt
    ref.close()


# ---- B. failed steps -----------------------------------------------------------------------------------------------------------------
def _bad_step(n):
    from mavflow import _lib
    s = _lib.FrameStep()
    s.n = n                                                          # beyond max_batch: refused before anything is enqueued
    return s


def test_a_failure_delivered_by_its_ticket_is_not_reported_again(mav):
    """B1: wait_step(t) raises; after that neither a drain (ctx.sync) nor a plain call reports it again."""
    from mavflow import _lib
    W, H = 64, 48
    prev, nxt = synth.make_batch(W, H, 1, distinct=1)
    with _lib.Context(W, H, 1) as rc:
        ref = rc.farneback(prev, nxt).copy()
    with _lib.Context(W, H, 1) as ctx:
        t = ctx.post_step(_bad_step(5))
        with pytest.raises(ValueError, match="n 5 outside"):
            ctx.wait_step(t)
        ctx.sync()
        assert ctx.farneback(prev, nxt).tobytes() == ref.tobytes()


def test_a_drain_reports_the_earliest_failure_not_yet_delivered(mav):
    """B2: two bad tickets; t1 is delivered by its wait, so the drain reports t2 -- and t2's own wait still tells."""
    from mavflow import _lib
    with _lib.Context(64, 48, 1) as ctx:
        t1, t2 = ctx.post_step(_bad_step(5)), ctx.post_step(_bad_step(7))
        with pytest.raises(ValueError, match="n 5 outside"):
            ctx.wait_step(t1)
        with pytest.raises(ValueError, match="n 7 outside"):
            ctx.drain()
        ctx.sync()                                                   # reported once by a drain: not again
        with pytest.raises(ValueError, match="n 7 outside"):
            ctx.wait_step(t2)
        ctx.sync()


@pytest.mark.parametrize("worker", [True, False])
def test_a_step_refused_inside_the_detection_leaves_the_pipeline_usable(mav, worker):
    """B3 / B4: foe_params.n_pairs = 0 is refused inside the detection, after the step's gathers and Farneback have been enqueued.
    The failure surfaces (at collect; with worker=False at submit), and by then the slot's marker has fired -- recorded behind what
    the step had enqueued -- so its host buffers go back with nothing of the step pending.  With the parameter restored every slot,
    the failed one included, gives the reference result again; close() succeeds and returns every device block."""
    from mavflow import _lib
    from mavflow.pipeline import DetectPipeline, FlowStage
    W, H, B = 640, 480, 4
    prev, nxt = synth.make_batch(W, H, B, distinct=B)
    prev, nxt = list(prev), list(nxt)
    smp = np.stack([synth.foe_samples(W, H, b) for b in range(B)])
    ref = _Ref(W, H, B)
    expect = ref.detect(ref.ctx.farneback(np.stack(prev), np.stack(nxt)).copy(), smp)
    with _lib.Context(W, H, B) as ctx:
        pipe = DetectPipeline(ctx, B, worker=worker, keep_flow=True)
        for _ in pipe.slots:                                         # every slot has its buffers
            _same(pipe.collect(pipe.submit(smp, prev=prev, nxt=nxt)), expect, "before")
        pipe.foe_params.n_pairs = 0
        failed = pipe.slots[pipe._turn]
        with pytest.raises(ValueError, match="n_pairs 0 outside"):
            pipe.collect(pipe.submit(smp, prev=prev, nxt=nxt))
        d = C.c_int(0)
        _lib.check(ctx.lib.mav_marker_query(None, failed.marker, C.byref(d)))
        assert d.value == 1 and failed.keep is None and not failed.busy
        pipe.foe_params.n_pairs = 1000
        for k in range(len(pipe.slots)):
            _same(pipe.collect(pipe.submit(smp, prev=prev, nxt=nxt)), expect, ("after", k))
        # a deferred flow through the same failure: its handle still reads the right flow, the next step recovers
        stage = FlowStage(ctx)
        pipe.foe_params.n_pairs = 0
        h = stage.flow_of(prev[0], nxt[0])
        with pytest.raises(ValueError, match="n_pairs 0 outside"):
            pipe.collect(pipe.submit(smp[0], flow=h))
        assert np.asarray(h).tobytes() == ref.flow(prev[0], nxt[0]).tobytes()
        pipe.foe_params.n_pairs = 1000
        h = stage.flow_of(prev[1], nxt[1])
        _same(pipe.collect(pipe.submit(smp[1], flow=h)), ref.detect(ref.flow(prev[1], nxt[1])[None], smp[1:2]), "deferred, after")
        stage.close()
        bufs = [b for s in pipe.slots for b in (s.frames, s.flow_out, s.mf, s.md, s.par, s.out) if b is not None]
        held = sum(b.nbytes for b in bufs)
        free_open = ctx.mem_info()["dev_free"]
        pipe.close()
        assert all(b.ptr is None for b in bufs) and pipe.slots == []
        freed = ctx.mem_info()["dev_free"] - free_open
        assert freed >= held // 2, (freed, held)                     # (allocation granularity and other tenants of the device)
        ctx.sync()
    ref.close()


def test_a_marker_of_a_closed_context_is_done_without_asking_the_runtime(mav):
    """A handle retired by pipe.close() is read after its context has gone (test_gpu_api_loop.py does so): mav_destroy has drained the
    streams, so the marker behind the handle's copy has fired, but the runtime's event still refers to the destroyed stream and must
    not be waited for or queried -- doing so gave "operation not permitted on an event last recorded in a capturing stream" when the
    heap had reused the stream's memory.  _Marker answers by itself then, and leaves no error behind for the next call."""
    from mavflow import _lib
    from mavflow.pipeline import _Marker
    asked = []
    with _lib.Context(64, 48, 1) as ctx:
        img = np.zeros((48, 64), np.uint8)
        img[5:9, 7:20] = 200
        ctx.bbox(img)
        m = _Marker(ctx)
        assert m.done() in (True, False)                                   # alive: the runtime answers
        m.wait()
        assert m.done() is True
        lib = ctx.lib
    assert not ctx.alive

    class Spy:                                                             # the library behind the marker, counting what is asked of it
        def __getattr__(self, name):
            if name in ("mav_marker_wait", "mav_marker_query"):
                asked.append(name)
            return getattr(lib, name)
    ctx.lib = Spy()
    m.wait()
    assert m.done() is True and asked == []
    ctx.lib = lib
    with _lib.Context(64, 48, 1) as other:                                 # nothing sticky is left for the next launch check
        assert tuple(other.bbox(img)[0]) == (7, 5, 19, 8)
