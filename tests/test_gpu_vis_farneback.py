"""Farneback(vis="device") against the host mode on the FakeCapture sequence of tests/test_gpu_shims.py (f0, f1, black, black; 320 x 240),
and what the entry points of include/mavflow_vis.h leave alone: every reader of tests/resident_cases.py returns the same code and bytes
before and after each of them (the tables are imported, not edited), a light call of the detect family after them returns a fresh
context's bytes, and they themselves return a fresh context's bytes after a heavier call."""
import numpy as np
import pytest

import resident_cases as rc
import vis_cases as vc
import vis_ref as R

pytestmark = pytest.mark.gpu
W, H, B = rc.W, rc.H, rc.B


class FakeCapture:
    """read() hands out ONE buffer, refilled on every call, as a decoding capture does"""

    def __init__(self, frames):
        self.frames, self.i = frames, 0
        self.buf = np.zeros_like(frames[0])

    def read(self):
        self.buf[...] = self.frames[min(self.i, len(self.frames) - 1)]
        self.i += 1
        return True, self.buf


def _sequence():
    from mavflow import synth
    f0, f1, _ = synth.make_pair(320, 240, 5)
    bgr = lambda g: np.ascontiguousarray(np.stack([g, np.roll(g, 3, 1), g[::-1]], -1))      # three different channels
    black = np.zeros((240, 320, 3), np.uint8)
    return [bgr(f0), bgr(f1), black, black]


def test_device_mode_equals_host_mode(mav):
    from mavflow import vis  # noqa: F401
    from mavflow.farneback import Farneback
    from mavflow.pipeline import DeviceArray
    frames = _sequence()
    host, dev = Farneback(FakeCapture(frames), None), Farneback(FakeCapture(frames), None, vis="device")
    assert host.vis == "host" and dev.vis == "device"
    try:
        for step in range(3):
            cap = dev.capture
            rh, rd = host.process(), dev.process()
            cap.buf[...] = 77                                          # the capture's buffer may be refilled right after process() returns
            assert rd.shape == rh.shape == (240, 320, 3) and rd.dtype == np.uint8
            if step == 2:                                              # black -> black: no flow, the previous result is kept
                assert rd is dev.prev_result and np.array_equal(rd, prev_dev) and np.array_equal(rh, prev_host)
                assert np.asarray(dev.flow).tobytes() == np.asarray(host.flow).tobytes()
                continue
            assert isinstance(dev.flow, DeviceArray) and dev.flow.on_device            # nothing but the picture and the record came back
            hue = R.process_hue_float(np.asarray(host.flow))
            band = vc.in_band(hue)
            share = band.mean()
            diff = (rd != rh).any(axis=-1)
            print(f"frame {step + 1}: band share {share:.2e}, {int(diff.sum())} pixels differ, {int((diff & ~band).sum())} outside the band")
            assert share < 1e-2 and not (diff & ~band).any()
            hsv_d, hsv_h = dev.hsv, host.hsv                           # produced on demand, from the flow where it is
            assert np.array_equal(hsv_d[~band], hsv_h[~band]) and np.array_equal(hsv_d[..., 1:], hsv_h[..., 1:])
            assert np.asarray(dev.flow).tobytes() == np.asarray(host.flow).tobytes()        # the flow itself, bit for bit
            prev_dev, prev_host = rd.copy(), rh.copy()
    finally:
        dev.close()


def test_device_mode_refuses_a_warm_start(mav):
    from mavflow import _lib
    from mavflow.farneback import Farneback

    class Warm(Farneback):
        PARAMS = dict(Farneback.PARAMS, flags=_lib.OPTFLOW_USE_INITIAL_FLOW)

    with pytest.raises(NotImplementedError, match="warm start"):
        Warm(FakeCapture(_sequence()), None, vis="device")
    with pytest.raises(ValueError):
        Farneback(FakeCapture(_sequence()), None, vis="gpu")


# ---- residency ------------------------------------------------------------------------------------------------------------------------------
def _inputs():
    rng = np.random.default_rng(84)
    return dict(flow=np.ascontiguousarray(vc.constructed_fields(W, H)), img=rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8),
                colour=np.array([0, 255, 0], np.uint8))


def _interveners(env, t):
    """name -> (run() -> return code, the code expected); the host forms on host arrays, the _dev forms on the interveners' own device blocks"""
    from mavflow import vis
    lib = vis.load()
    p_, h = rc.p_, env.h
    n = B * H * W
    bgr, hsv, rec = np.zeros((B, H, W, 3), np.uint8), np.zeros((B, H, W, 3), np.uint8), np.zeros(B, vis.RECORD_DTYPE)
    img = t["img"].copy()
    dev = lambda name, src: env.dev("iv_vis_" + name, src)
    col = t["colour"].ctypes.data
    runs = {
        "mav_flow_hsv": lambda: lib.mav_flow_hsv(h, p_(t["flow"]), B, vis.HSV_PROCESS, p_(bgr), p_(hsv), p_(rec)),
        "mav_flow_hsv draw": lambda: lib.mav_flow_hsv(h, p_(t["flow"]), B, vis.HSV_DRAW, p_(bgr), None, p_(rec)),
        "mav_flow_hsv_dev": lambda: lib.mav_flow_hsv_dev(h, dev("flow", t["flow"]), B, vis.HSV_PROCESS, dev("bgr", 3 * n), dev("hsv", 3 * n), dev("rec", 16 * B)),
        "mav_flow_hsv_dev draw, bytes": lambda: lib.mav_flow_hsv_dev(h, dev("flow", t["flow"]), B, vis.HSV_DRAW, dev("bgr1", 3 * n + 16) + 1, None, dev("rec", 16 * B)),
        "mav_cvt_color": lambda: lib.mav_cvt_color(h, p_(t["img"]), vis.COLOR_BGR2HSV, B, p_(hsv)),
        "mav_cvt_color_dev": lambda: lib.mav_cvt_color_dev(h, dev("img", t["img"]), vis.COLOR_HSV2BGR, B, dev("bgr", 3 * n)),
        "mav_draw_flow": lambda: lib.mav_draw_flow(h, p_(img), p_(t["flow"]), B, 4, 1.0, col),
        "mav_draw_flow_dev": lambda: lib.mav_draw_flow_dev(h, dev("img", t["img"]), dev("flow", t["flow"]), B, 8, 0.0, col),
    }
    out = {k: (v, rc.OK) for k, v in runs.items()}
    out["mav_flow_hsv refused(mode)"] = (lambda: lib.mav_flow_hsv(h, p_(t["flow"]), B, 7, p_(bgr), None, p_(rec)), rc.ERR_ARG)
    out["mav_draw_flow_dev refused(step)"] = (lambda: lib.mav_draw_flow_dev(h, dev("img", t["img"]), dev("flow", t["flow"]), B, 0, 1.0, col), rc.ERR_ARG)
    return out


@pytest.mark.parametrize("pname", list(rc.PRODUCERS))
def test_every_reader_returns_the_same_after_the_vis_calls(mav, pname):
    from mavflow import _lib, vis
    P, readers, t = rc.PRODUCERS[pname], rc.readers_of(pname), _inputs()
    fails = []
    with _lib.Context(W, H, B) as ctx:
        env = rc.Env(ctx)
        try:
            P.run(env)
            base = {}
            for name in readers:
                code, _, value = rc.READERS[name][2](env)
                assert code == rc.OK, (pname, name, code)
                base[name] = value
            ivs = _interveners(env, t)
            assert set(vis.EXPORTS) - {"mav_vis_form"} <= set(ivs)
            for iname, (run, want) in ivs.items():
                got = run()
                assert got == want, (pname, iname, got, _lib.load().mav_last_error())
                for name in readers:
                    code, _, value = rc.READERS[name][2](env)
                    if code != rc.OK or value != base[name]:
                        fails.append(f"{pname}, {iname}, {name}: returned {code}" + ("" if value == base[name] else " with other bytes"))
            ctx.sync()
        finally:
            env.close()
    assert not fails, "\n".join(fails)


def _vis_bytes(ctx, t):
    """what the host forms of the family return on this context"""
    out = ctx.flow_hsv(t["flow"], "process", hsv=True)
    drawn = ctx.draw_flow(t["img"].copy(), t["flow"], step=4)
    return b"".join(a.tobytes() for a in (out["bgr"], out["hsv"], out["record"], ctx.flow_hsv(t["flow"], "draw")["bgr"],
                                          ctx.cvt_color(t["img"], 40), ctx.cvt_color(t["img"], 54), drawn))


def test_fresh_context_bytes_after_a_heavier_call_and_for_a_light_call_after(mav):
    from mavflow import _lib, synth, vis  # noqa: F401
    t = _inputs()
    prev, nxt = synth.make_batch(W, H, B, distinct=B)
    samples = np.stack([synth.foe_samples(W, H, b) for b in range(B)])
    with _lib.Context(W, H, B) as fresh:
        want = _vis_bytes(fresh, t)
    with _lib.Context(W, H, B) as fresh:
        light = fresh.bgr2gray(t["img"]).tobytes() + fresh.bbox(t["img"][..., 0]).tobytes()
    with _lib.Context(W, H, B) as ctx:
        base = ctx.process_batch(prev, nxt, samples)                    # the heaviest call: frames -> flow -> FoE -> masks -> boxes
        images = {k: v.copy() for k, v in ctx.render_last(B).items()}
        assert _vis_bytes(ctx, t) == want
        assert ctx.bgr2gray(t["img"]).tobytes() + ctx.bbox(t["img"][..., 0]).tobytes() == light
    with _lib.Context(W, H, B) as ctx:
        ctx.process_batch(prev, nxt, samples)
        env = rc.Env(ctx)
        try:
            for run, code in _interveners(env, t).values():
                assert run() == code
        finally:
            env.close()
        after = ctx.render_last(B)                                       # render_last is unchanged by the family
        assert set(after) == set(images) and all(np.array_equal(after[k], images[k]) for k in images)
        assert base["results"].tobytes() == ctx.process_batch(prev, nxt, samples)["results"].tobytes()


def test_a_light_call_after_each_entry_point_returns_a_fresh_contexts_bytes(mav):
    """after EACH call of the family, host and _dev form and the refused ones, one light call of the detect family (bgr2gray, bbox)"""
    from mavflow import _lib, vis  # noqa: F401
    t = _inputs()
    light = lambda c: c.bgr2gray(t["img"]).tobytes() + c.bbox(t["img"][..., 0]).tobytes()
    with _lib.Context(W, H, B) as fresh:
        want = light(fresh)
    with _lib.Context(W, H, B) as ctx:
        env = rc.Env(ctx)
        try:
            for iname, (run, code) in _interveners(env, t).items():
                assert run() == code, iname
                assert light(ctx) == want, iname
        finally:
            env.close()


def test_the_calls_hold_no_memory_of_the_contexts(mav):
    from mavflow import _lib, vis  # noqa: F401
    t = _inputs()
    with _lib.Context(W, H, B) as ctx:
        env = rc.Env(ctx)
        try:
            ivs = _interveners(env, t)
            for run, want in ivs.values():                                  # once: the staging blocks of every call shape exist from here on
                assert run() == want
            before = ctx.mem_info()
            for run, want in ivs.values():
                assert run() == want
                after = ctx.mem_info()
                assert (after["ctx_bytes"], after["workspace_bytes"]) == (before["ctx_bytes"], before["workspace_bytes"])
            assert before["workspace_bytes"] == 0
        finally:
            env.close()
