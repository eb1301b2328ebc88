"""The flow history on the device (csrc/kernels_history.hip: k_history_put, k_history_trace, k_remap_linear) held to the numpy
restatement tests/history_ref.py byte for byte, NaNs included (both store THE quiet NaN), on every case of tests/history_cases.py: the
stage-level remap, host and device entry points (on the same fields: tests/test_history_cases_cpu.py checks that their cases share
one reference, so equal bytes there are equal bytes between them), several fields per call, reset, two histories on one context, Detector.get_history
from an array and from a device handle, and the "flow" output thresholded without leaving the device."""
import ctypes as C

import numpy as np
import pytest

import history_cases as hc
import history_ref as R

pytestmark = pytest.mark.gpu
GUARD = 64                     # canary bytes kept on both sides of a caller's output


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, got.dtype, want.shape, want.dtype)
    a, b = R.bits(got), R.bits(want)
    if not np.array_equal(a, b):
        bad = np.argwhere(a != b)
        raise AssertionError((what, len(bad), "first differing element", bad[0].tolist(), got[tuple(bad[0])], want[tuple(bad[0])]))


def _run(c, ctx, hist, fields, count):
    """The case's fields through one history, `count` per call: (pushes, H, W, 2) in the case's out form."""
    from mavflow import _lib
    odt = _lib.HISTORY_OUTS[c.out][1]
    outs = []
    if c.entry == "host":
        for i in range(0, len(fields), count):
            chunk = fields[i:i + count]
            outs.append(hist.push(chunk[0], out=c.out)[None] if count == 1 else hist.push(chunk, out=c.out))
        return np.concatenate(outs)
    for i in range(0, len(fields), count):                  # the caller's own buffers, offset by the case's bytes, guarded
        chunk = np.ascontiguousarray(fields[i:i + count])
        n, obytes = len(chunk), len(chunk) * c.n0 * 2 * odt.itemsize
        fbuf, obuf = ctx.alloc(chunk.nbytes + 64), ctx.alloc(obytes + 2 * GUARD + 64)
        try:
            raw = np.full(chunk.nbytes + 64, 0xA5, np.uint8)
            raw[c.flow_off:c.flow_off + chunk.nbytes] = chunk.view(np.uint8).reshape(-1)
            fbuf.upload(raw)
            obuf.upload(np.full(obytes + 2 * GUARD + 64, 0x5A, np.uint8))
            hist.push_enqueue(fbuf.ptr + c.flow_off, obuf.ptr + GUARD + c.out_off, count=n, dtype=chunk.dtype, out=c.out)
            back = obuf.download(np.uint8, (obytes + 2 * GUARD + 64,))
            lo, hi = GUARD + c.out_off, GUARD + c.out_off + obytes
            assert (back[:lo] == 0x5A).all() and (back[hi:] == 0x5A).all(), (c.name, "wrote outside its output")
            outs.append(back[lo:hi].copy().view(odt).reshape(n, c.H, c.W, 2))
        finally:
            fbuf.free()
            obuf.free()
    return np.concatenate(outs)


def _history(ctx, c):
    return ctx.flow_history(c.L, hc.NP[c.ring], c.axes)


@pytest.mark.parametrize("name", [c.name for c in hc.CASES])
def test_push_equals_the_restatement(mav, name):
    """Every case of the table, its fields `count` per call and -- where count > 1 -- the same fields again one by one: both equal the
    restatement's bytes, so they equal each other."""
    from mavflow import _lib
    c = hc.BY_NAME[name]
    want, _ = hc.reference(name)
    fields = hc.fields_of(c)
    with _lib.Context(c.W, c.H, 1) as ctx:
        hist = _history(ctx, c)
        got = _run(c, ctx, hist, fields, c.count)
        _same(got, want, (name, "count", c.count))
        assert hist.pushes == c.n_pushes and hist.index == c.n_pushes % c.L
        assert hist.ring_bytes == c.L * c.n0 * 2 * hc.ELEM[c.ring]
        if c.count > 1:
            hist.reset()
            assert hist.pushes == 0 and hist.index == 0
            _same(_run(c, ctx, hist, fields, 1), want, (name, "one by one after reset"))
        hist.close()


REMAP_CASES = ["planted37x23_f32tof32_reference_reference", "planted37x23_f64tof64_reference_reference", "tiny1x1_L3", "tiny7x1", "tiny1x7_xy",
               "tiny5x3_f64", "tiny6x2_flow"]


@pytest.mark.parametrize("name", REMAP_CASES)
def test_stage_remap_equals_the_restatement(mav, name):
    """mav_stage_remap_linear: the sampled field (NaN and infinity inside) at the positions the planted field sends the pixels to --
    every tap position, tie, non-finite and far-away coordinate of the table -- and at a dense sweep of 1/64 steps across the borders."""
    from mavflow import _lib
    c = hc.BY_NAME[name]
    H, W = c.H, c.W
    src = hc.sampled(W, H, 3).astype(hc.NP[c.ring])
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    p = hc.planted(W, H, "reference")
    with np.errstate(all="ignore"):
        maps = [(xx + p[..., 1], yy + p[..., 0]), (xx, yy)]
        rng = np.random.default_rng(W + H)
        maps.append(((rng.integers(-3 * 64, (W + 3) * 64, (H, W)) / 64.0).astype(np.float32), (rng.integers(-3 * 64, (H + 3) * 64, (H, W)) / 64.0).astype(np.float32)))
        maps.append((rng.normal(W / 2, W, (H, W)).astype(np.float32), rng.normal(H / 2, H, (H, W)).astype(np.float32)))
    with _lib.Context(W, H, 1) as ctx:
        for i, (mx, my) in enumerate(maps):
            _same(ctx.stage_remap_linear(src, mx, my), R.remap_linear_ref(src, mx, my), (name, "map", i))
        clean = np.nan_to_num(src, nan=1.0, posinf=2.0, neginf=-2.0)
        _same(ctx.stage_remap_linear(clean, xx, yy), clean.astype(np.float64), (name, "identity"))


def test_two_histories_on_one_context_do_not_disturb_each_other(mav):
    from mavflow import _lib
    a, b = hc.BY_NAME["planted37x23_f32tof32_reference_reference"], hc.BY_NAME["planted37x23_f64tof64_xy_flow"]
    fa, fb = hc.fields_of(a), hc.fields_of(b)
    with _lib.Context(a.W, a.H, 1) as ctx:
        base = ctx.mem_info()["ctx_bytes"]
        ha, hb = _history(ctx, a), _history(ctx, b)
        assert ctx.mem_info()["ctx_bytes"] - base == ha.ring_bytes + hb.ring_bytes
        ga, gb = [], []
        for i in range(a.n_pushes):                          # interleaved
            ga.append(ha.push(fa[i], out=a.out))
            gb.append(hb.push(fb[i], out=b.out))
        _same(np.stack(ga), hc.reference(a.name)[0], "first history")
        _same(np.stack(gb), hc.reference(b.name)[0], "second history")
        ha.reset()                                           # resetting one leaves the other where it was
        assert (ha.index, ha.pushes, hb.index, hb.pushes) == (0, 0, b.n_pushes % b.L, b.n_pushes)
        _same(ha.push(fa[0]), hc.reference(a.name)[0][0], "after reset")
        ref = R.HistoryRef(b.H, b.W, b.L, np.float64, b.axes)
        for f in fb:
            ref.get_history(f, b.out)
        _same(hb.push(fb[0], out=b.out), ref.get_history(fb[0], b.out), "the other goes on")
        held = ctx.mem_info()["ctx_bytes"]                    # (the host pushes' staging blocks stay with the context)
        rings = ha.ring_bytes + hb.ring_bytes
        hb.close()
        ha.close()
        assert held - ctx.mem_info()["ctx_bytes"] == rings


class _Dataset:
    def __init__(self, W, H):
        self.capture_size = (W, H)
        self.ground_truth = []


def test_detector_get_history_from_an_array_and_from_a_handle(mav):
    """Detector.get_history over 2 L + 1 frames (the reference's name, argument and return): host arrays on one detector, device
    handles of the flow seam's kind on another; history_length / history_index as in the reference."""
    from mavflow import _lib, pipeline
    from mavflow.detector import Detector
    c = hc.Case("detector61x47_L5", 61, 47, L=5, kind="smooth")        # (the detector's constructor samples 20 px inside the frame)
    fields = hc.fields_of(c)
    ref = R.HistoryRef(c.H, c.W, c.L, np.float64)                       # the reference's own float64 ring
    want = [ref.get_history(f) for f in fields]
    assert len(fields) == 2 * c.L + 1
    np.random.seed(3)
    det_a, det_h = Detector(_Dataset(c.W, c.H), Detector.Algorithm.FOE), Detector(_Dataset(c.W, c.H), Detector.Algorithm.FOE)
    assert det_a.history_length == 20 and det_a.history_index == 0 and det_a._history is None      # nothing allocated until called
    det_a.history_length = det_h.history_length = c.L
    with _lib.Context(c.W, c.H, 1) as ctx:
        buf = ctx.alloc(fields[0].nbytes)
        for i, f in enumerate(fields):
            out = det_a.get_history(f)
            _same(out, want[i], ("array", i))
            buf.upload(f)
            handle = pipeline.DeviceArray(ctx, buf.ptr, (c.H, c.W, 2), np.float32)
            _same(det_h.get_history(handle), want[i], ("handle", i))
            assert handle.on_device                                    # read where it is
            assert det_a.history_index == det_h.history_index == (i + 1) % c.L
        assert det_h._history.ctx is ctx
        with pytest.raises(ValueError):                                # a float64 field would round into the float32 ring
            det_a.get_history(fields[0].astype(np.float64))
        det_h._history.close()
        buf.free()
    det_a._history.close()


def test_flow_output_feeds_detect_without_leaving_the_device(mav):
    """out="flow" is the float32 (u, v) layout of the detection stage: mav_detect_dev on the buffer the push wrote equals
    Context.detect on the same array uploaded from the host."""
    from mavflow import _lib, synth
    W, H, L = 64, 48, 4
    with _lib.Context(W, H, 1) as ctx:
        hist = ctx.flow_history(L, np.float32, "xy")
        obuf = ctx.alloc(W * H * 8)
        fbuf = ctx.alloc(W * H * 8)
        for i in range(2 * L):
            fbuf.upload(hc.smooth(W, H, i))
            hist.push_enqueue(fbuf, obuf, out="flow")
        acc = obuf.download(np.float32, (H, W, 2))
        assert np.isfinite(acc).all() and np.abs(acc).max() > 1.0
        samples = synth.foe_samples(W, H, 0).astype(np.uint32)
        fp, tp = _lib.foe_defaults(), _lib.thr_defaults()
        sbuf, rbuf, mf, md = ctx.alloc(samples.nbytes).upload(samples), ctx.alloc(_lib.RESULT_DTYPE.itemsize), ctx.alloc(W * H), ctx.alloc(W * H)
        _lib.check(ctx.lib.mav_detect_dev(ctx.h, obuf.ptr, sbuf.ptr, None, None, None, None, 1, C.byref(fp), C.byref(tp), None, mf.ptr, md.ptr, rbuf.ptr))
        dev = (rbuf.download(_lib.RESULT_DTYPE, (1,)), mf.download(np.uint8, (H, W)), md.download(np.uint8, (H, W)))
        host = ctx.detect(acc, samples)
        assert dev[0].tobytes() == host["results"].tobytes()
        assert np.array_equal(dev[1], host["mask_fixed"][0].view(np.uint8)) and np.array_equal(dev[2], host["mask_dyn"][0].view(np.uint8))
        for b in (obuf, fbuf, sbuf, rbuf, mf, md):
            b.free()
        hist.close()
