"""Device-memory behaviour of a context (include/mavflow.h: mav_mem_info): the Farneback workspace belongs to the calls that compute
flow, the reference's stateless helpers (src/im_helpers.py:55-84, 244-252) must not pay for it; the Python helpers keep a bounded
number of contexts."""
import numpy as np
import pytest

from mavflow import synth

pytestmark = pytest.mark.gpu
MB = 1 << 20


def test_a_4k_context_used_for_bbox_only_takes_a_few_megabytes(mav):
    from mavflow import _lib
    W, H = 3840, 2160
    with _lib.Context(64, 48, 1) as warm:                        # the runtime's own first-use allocations (code objects, pools)
        warm.bbox(np.zeros((48, 64), np.uint8))
        free0 = warm.mem_info()["dev_free"]
        img = np.zeros((H, W), np.uint8)
        img[700:720, 1000:1100] = 255
        with _lib.Context(W, H, 1) as ctx:
            assert tuple(ctx.bbox(img)[0]) == (1000, 700, 1099, 719)
            info = ctx.mem_info()
            taken = free0 - info["dev_free"]
            print(f"3840x2160 context after bbox: {taken / MB:.1f} MB of device memory taken, ctx_bytes {info['ctx_bytes'] / MB:.1f} MB, "
                  f"workspace {info['workspace_bytes']}")
            assert info["workspace_bytes"] == 0
            assert taken < 64 * MB and info["ctx_bytes"] < 64 * MB
            # validation counts and the detection tail do not bring it either
            ctx.tpr_fpr_counts(img, (img > 0).astype(np.uint8))
            assert ctx.mem_info()["workspace_bytes"] == 0


def test_the_workspace_comes_with_the_first_flow_call_and_stays(mav):
    from mavflow import _lib
    W, H, B = 640, 480, 2
    prev, nxt = synth.make_batch(W, H, B, distinct=B)
    with _lib.Context(W, H, B) as ctx:
        assert ctx.mem_info()["workspace_bytes"] == 0
        sched = ctx.schedule_info(B)                              # planning needs no workspace
        assert sched["pairs_per_group"] == B
        ctx.set_option("group", 1)                                # ... nor does changing the plan
        assert ctx.mem_info()["workspace_bytes"] == 0
        ctx.set_option("group", 2)
        f1 = ctx.farneback(prev, nxt).copy()
        ws = ctx.mem_info()["workspace_bytes"]
        assert ws > 0
        f2 = ctx.farneback(prev, nxt)
        assert ctx.mem_info()["workspace_bytes"] == ws and np.array_equal(f1, f2)
        # a stage hook that needs the two-pass scratch takes a staging block of its own: no Farneback workspace, and "deep_frac"
        # (settable until the first call that computes flow) stays open
    with _lib.Context(W, H, 1) as ctx:
        a = ctx.stage_blur_resize(prev[0], 1, two_pass=True)
        assert ctx.mem_info()["workspace_bytes"] == 0
        assert np.array_equal(a, ctx.stage_blur_resize(prev[0], 1))
        ctx.set_option("deep_frac", 32)


def test_deep_layer_workspace_arrives_with_the_first_call_of_more_than_one_group(mav):
    """The deep layers' work set is reachable only by calls of more than one group: a context whose calls stay within one group never
    holds it, and mav_mem_info's workspace figure grows by exactly that set when the first such call comes."""
    from mavflow import _lib
    W, H, B = 320, 240, 6
    prev, nxt = synth.make_batch(W, H, B, distinct=2)
    with _lib.Context(W, H, B) as ctx:
        ctx.set_option("group", 2)
        one = ctx.farneback(prev[:2], nxt[:2]).copy()            # one group: no deep set
        ws1 = ctx.mem_info()["workspace_bytes"]
        all6 = ctx.farneback(prev, nxt)                           # three groups: the deep layers run once for the call
        ws2 = ctx.mem_info()["workspace_bytes"]
        assert ws2 > ws1 > 0
        assert np.array_equal(all6[:2], one)
        ctx.farneback(prev, nxt)
        assert ctx.mem_info()["workspace_bytes"] == ws2


def test_helper_context_cache_is_bounded_and_a_held_context_survives_eviction(mav):
    """The helpers' context cache keeps the most recently used frame sizes and only DROPS what falls out -- it never closes a context,
    because a caller may still hold it: pyramid() across its yields, a loop across its frames."""
    from mavflow import im_helpers
    im_helpers._ctx_cache.clear()
    cap = im_helpers._CTX_CACHE_SIZES
    sizes = [(64 + 16 * k, 48 + 12 * k) for k in range(cap + 2)]
    seen = []
    for (W, H) in sizes:
        img = np.zeros((H, W), np.uint8)
        img[5:9, 7:20] = 200
        r = im_helpers.get_simple_bounding_box(img)
        assert r.get_topleft() == (7, 5)
        seen.append(im_helpers._ctx_cache[(W, H)])
    assert list(im_helpers._ctx_cache) == sizes[2:]               # `cap` sizes kept, the two oldest dropped ...
    assert seen[0].h is not None                                  # ... but NOT closed: the handle we hold still works
    img = np.zeros((sizes[0][1], sizes[0][0]), np.uint8)
    img[3, 4] = 9
    assert tuple(seen[0].bbox(img)[0]) == (4, 3, 4, 3)
    im_helpers.get_simple_bounding_box(np.zeros((sizes[3][1], sizes[3][0]), np.uint8))
    assert list(im_helpers._ctx_cache)[-1] == sizes[3]            # a hit moves to the back
    c = im_helpers._ctx(*sizes[4], batch=4)                       # a larger batch replaces the cached context, the old one stays usable
    assert c.max_batch == 4 and seen[4].h is not None and c is not seen[4]
    im_helpers._ctx_cache.clear()


def test_pyramid_generator_survives_helper_calls_on_every_level_size(mav):
    """pyramid() holds its context across yields; calling a helper on each level's own size (more sizes than the cache keeps would
    evict that context) must not break the next level."""
    from mavflow import im_helpers
    im_helpers._ctx_cache.clear()
    keep = im_helpers._CTX_CACHE_SIZES
    im_helpers._CTX_CACHE_SIZES = 2
    try:
        img = (np.add.outer(np.arange(540), np.arange(960)) % 251).astype(np.uint8)
        levels = []
        for lv in im_helpers.pyramid(img, scale=1.5):
            box = im_helpers.get_simple_bounding_box(lv)          # a context of this level's size: evicts the generator's
            assert box.get_topleft()[0] >= 0
            levels.append(lv.shape)
        assert len(levels) >= 6 and levels[0] == (540, 960)
    finally:
        im_helpers._CTX_CACHE_SIZES = keep
        im_helpers._ctx_cache.clear()


def test_two_contexts_in_two_threads_are_independent(mav):
    """include/mavflow.h: a mav_ctx is single-threaded, distinct contexts are independent.  Two host threads, each with a context of its
    own (different frame sizes, hence different streams, workspaces, tables and option sets), run the fused path concurrently; every
    result must equal what the same context gives alone."""
    import threading
    from mavflow import _lib
    jobs = []
    for (W, H, B, levels) in ((640, 480, 3, 1), (1000, 562, 2, 3)):
        prev, nxt = synth.make_batch(W, H, B, distinct=B)
        smp = np.stack([synth.foe_samples(W, H, b) for b in range(B)])
        with _lib.Context(W, H, B, _lib.fb_defaults(levels=levels)) as c:
            ref = c.process_batch(prev, nxt, smp)
        jobs.append((W, H, B, levels, prev, nxt, smp, ref))
    errors = []

    def work(job):
        W, H, B, levels, prev, nxt, smp, ref = job
        try:
            with _lib.Context(W, H, B, _lib.fb_defaults(levels=levels)) as c:
                c.set_option("group", 1 + (W % 2))
                for rep in range(6):
                    out = c.process_batch(prev, nxt, smp)
                    assert np.array_equal(out["flow"], ref["flow"]), (W, rep)
                    assert out["results"].tobytes() == ref["results"].tobytes(), (W, rep)
                    assert np.array_equal(out["mask_fixed"], ref["mask_fixed"]) and np.array_equal(out["mask_dyn"], ref["mask_dyn"])
        except Exception as e:                         # noqa: BLE001 -- reported by the main thread
            errors.append(repr(e))

    threads = [threading.Thread(target=work, args=(j,)) for j in jobs]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors


def _walk(ctx, d):
    """Every call of a context that allocates device memory lazily, once each: [(step, mem_info after it)]."""
    from mavflow import _lib
    prev, nxt, smp, B = d["prev"], d["nxt"], d["samples"], d["prev"].shape[0]
    marks = []

    def step(name, fn):
        out = fn()
        marks.append((name, ctx.mem_info()))
        return out

    def process_batch_dev_without_flow():                       # nobody wants the flow: the context's own flow buffer
        bufs = [ctx.alloc(a.nbytes).upload(a) for a in (prev, nxt, smp)] + [ctx.alloc(B * _lib.RESULT_DTYPE.itemsize)]
        try:
            ctx.process_batch_dev(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, B, bufs[3].ptr)
            ctx.sync()
        finally:
            for b in bufs:                                      # caller-owned memory: not the context's, and not in dev_free afterwards
                b.free()

    def sparse():
        pts = ctx.good_features(prev[0])
        ctx.lk_track(None, nxt[0], pts)

    step("bbox", lambda: ctx.bbox(prev))
    flow = step("farneback, several groups", lambda: ctx.farneback(prev, nxt).copy())
    step("farneback with an initial flow", lambda: ctx.farneback(prev, nxt, initial_flow=flow))
    out = step("process_batch", lambda: ctx.process_batch(prev, nxt, smp))
    step("process_batch_dev without a flow pointer", process_batch_dev_without_flow)
    foe = [(ctx.W / 2.0, ctx.H / 2.0)] * B
    step("render", lambda: ctx.render(flow, foe))
    step("overlay", lambda: ctx.overlay(d["bgr"], out["mask_fixed"], foe, foe))
    step("png_encode", lambda: ctx.png_encode(prev))
    step("analyze_pyramid", lambda: ctx.analyze_pyramid(prev))
    step("optimize_window", lambda: ctx.optimize_window(prev, [(40, 30, 64, 64)] * B))
    step("good_features + lk_track", sparse)
    step("flow_to_color of a float64 field", lambda: ctx.flow_to_color(flow.astype(np.float64)))    # 16 bytes per pixel: grows staging block 0
    return marks


def test_every_lazy_allocation_is_counted_kept_when_warm_and_given_back(mav):
    """The context's device memory from outside, over every call that allocates lazily (_walk): mav_mem_info's ctx_bytes never
    decreases from one call to the next, the host call with the largest staging buffer grows it, a second pass over the same calls
    leaves ctx_bytes and workspace_bytes exactly where the first left them (nothing is reallocated once warm), and close() gives
    everything back: the device's free memory, read from a small context that stays open, is the same after every walk in a fresh
    context -- a buffer mav_destroy forgets would make every walk take more than the one before.
    Measured on one MI355X, six walks in a process that had done nothing else, before and after the ledger went in (the same figures
    from both libraries): dev_free 308 363 132 928 after the first walk's close(), 308 354 744 320 after each of the other five.  The
    HIP runtime keeps 8 MiB more from the second walk on (pools of its own: in a process that other tests have warmed the first two
    readings agree as well), so a walk whose reading is not compared goes first, the next two must agree to the byte -- the parent's
    spread over five repetitions is zero --, and the first may exceed them by that 8 MiB at most."""
    from mavflow import _lib
    W, H, B = 320, 240, 4
    prev, nxt = synth.make_batch(W, H, B, distinct=B)
    d = dict(prev=prev, nxt=nxt, samples=np.stack([synth.foe_samples(W, H, b) for b in range(B)]),
             bgr=np.ascontiguousarray(np.stack([prev, nxt, prev], axis=-1)))
    free_after = []
    with _lib.Context(64, 48, 1) as probe:
        probe.bbox(np.zeros((48, 64), np.uint8))
        for walk in range(3):
            with _lib.Context(W, H, B) as ctx:
                ctx.set_option("group", 2)                       # 4 pairs = 2 groups: the deep layers' set comes too
                last = ctx.mem_info()
                assert last["workspace_bytes"] == 0
                for name, info in _walk(ctx, d):
                    print(f"walk {walk}: ctx_bytes {info['ctx_bytes']:>10} workspace_bytes {info['workspace_bytes']:>10} after {name}")
                    assert info["ctx_bytes"] >= last["ctx_bytes"] and info["workspace_bytes"] >= last["workspace_bytes"], name
                    if name.startswith("flow_to_color"):
                        assert info["ctx_bytes"] > last["ctx_bytes"], name
                    last = info
                assert 0 < last["workspace_bytes"] < last["ctx_bytes"]
                for name, info in _walk(ctx, d):                 # warm: every buffer exists and is large enough
                    assert (info["ctx_bytes"], info["workspace_bytes"]) == (last["ctx_bytes"], last["workspace_bytes"]), name
            free_after.append(probe.mem_info()["dev_free"])
            print(f"walk {walk}: dev_free after close() {free_after[-1]}")
    assert free_after[2] == free_after[1], free_after            # a later walk takes no more than the one before: nothing leaks
    assert free_after[0] - free_after[1] <= 8 * MB, free_after
