"""The Gaussian window (cv2.OPTFLOW_FARNEBACK_GAUSSIAN; mav_set_window) on the device.

Stage: every sweep kernel form, on every layer of the small cases of tests/stage_cases.py, against tests/gauss_window_ref.py BIT FOR
BIT -- the Gaussian path is float32 with a fixed operation order, so unlike the box path (whose CPU original sums in double) it has
no tolerance -- and the box window of the same library untouched.  End to end: Context.farneback against gauss_window_ref.calc through
the strict flow gate of oracle/tolerances.py (the pyramid in front of the sweeps is the box path's and toleranced as there), and the
box flow failing that gate.  Schedules: the box path's bit-identity tests repeated with the Gaussian window.  Interface: mav_set_window
/ mav_get_window, the schedule line, the cv2-signature function.

Reference error (CPU, the four end-to-end inputs): gauss_window_ref.calc moves by mean <= 2e-6, p99.9 <= 3.1e-5, max <= 1.9e-4 px when
R0 / R1 are perturbed by +-3e-5 (the size of the GPU's expansion error) or every operation is widened to float64 -- two orders inside
the gate.  The library against it, measured on an MI355X on those inputs: mean <= 1.4e-6, p99.9 <= 1.3e-5, max <= 8.8e-5 px (the
box flow of the same pairs: mean 0.039 - 0.147 px)."""
import numpy as np
import pytest

import gauss_window_ref as gw
import schedule_cases as sc
from stage_cases import CASES, FORMS, crafted_flow, images, smooth_flow, sweep_form

pytestmark = pytest.mark.gpu

STAGE_CASES = [c for c in CASES if (c.W, c.H) not in ((1920, 1080), (3840, 2160))]
STAGE_IDS = [c.name for c in STAGE_CASES]


def soa(a):
    return np.ascontiguousarray(np.moveaxis(a, -1, 0))


def test_stage_cases_reach_every_testable_form(mav):
    from mavflow import _lib
    assert len(STAGE_CASES) == 11
    reached = set()
    for case in STAGE_CASES:
        with _lib.Context(case.W, case.H, 1, case.fb(), window="gaussian") as ctx:
            reached |= {sweep_form(ctx.layer_dims(k)[0], case.winsize) for k in range(ctx.num_layers())}
    assert reached == FORMS["sweep"], reached


@pytest.mark.parametrize("case", STAGE_CASES, ids=STAGE_IDS)
def test_sweep_bit_for_bit(mav, fb_oracle, case):
    """One Gaussian sweep per layer and flow: the stored flow is gauss_window_ref.sweep(M) bit for bit, M' is UpdateMatrices of that
    flow bit for bit, update = False stores the same flow and no M'; the context switched back to the box window returns what a
    context that never left it returns."""
    from mavflow import _lib
    imgs = images(case)
    with _lib.Context(case.W, case.H, 1, case.fb(), window="gaussian") as ctx, _lib.Context(case.W, case.H, 1, case.fb()) as box:
        assert ctx.window == "gaussian" and box.window == "box"
        for k in range(ctx.num_layers()):
            w, h, sigma, ks = ctx.layer_dims(k)
            R = [fb_oracle.polyexp(fb_oracle.blur_resize(img, w, h, ks, sigma), case.poly_n, case.poly_sigma) for img in imgs]
            R0, R1 = soa(R[0]), soa(R[1])
            form = sweep_form(w, case.winsize)
            for tag, flow in (("smooth", smooth_flow(w, h)), ("crafted", crafted_flow(w, h))):
                M = fb_oracle.update_matrices(R[0], R[1], flow)
                want = gw.sweep(M, case.winsize)
                gflow, gM = ctx.stage_blur_iter(R0, R1, soa(M), k, True)
                bad = int((gflow != want).any(-1).sum())
                assert np.array_equal(gflow, want), (case.name, k, tag, form, bad, float(np.abs(gflow - want).max()))
                assert np.array_equal(gM, ctx.stage_update_matrices(R0, R1, gflow, k)), (case.name, k, tag, form)
                last, none = ctx.stage_blur_iter(R0, R1, soa(M), k, False)
                assert none is None and np.array_equal(last, gflow), (case.name, k, tag, form)
                bflow, bM = box.stage_blur_iter(R0, R1, soa(M), k, True)
                ctx.set_window("box")
                sflow, sM = ctx.stage_blur_iter(R0, R1, soa(M), k, True)
                ctx.set_window("gaussian")
                assert np.array_equal(sflow, bflow) and np.array_equal(sM, bM), (case.name, k, tag, form)


# ---- end to end ---------------------------------------------------------------------------------------------------------------
E2E = [(640, 480, 0, 1, 12), (333, 227, 3, 1, 13), (640, 480, 2, 3, 12), (96, 64, 1, 1, 12)]     # W, H, pair, levels, winsize


@pytest.mark.parametrize("W,H,pair,levels,winsize", E2E, ids=[f"{w}x{h}_p{p}_l{l}_w{ws}" for w, h, p, l, ws in E2E])
def test_farneback_against_the_reference(mav, fb_oracle, W, H, pair, levels, winsize):
    from mavflow import _lib, synth
    from oracle import fb_oracle as fbo, tolerances
    prev, nxt = synth.make_pair(W, H, pair)[:2]
    fb = _lib.fb_defaults(levels=levels)
    fb.winsize = winsize
    exp = gw.calc(fb_oracle, prev, nxt, fbo.Params(fb.pyr_scale, levels, winsize, fb.iterations, fb.poly_n, fb.poly_sigma, 0))
    with _lib.Context(W, H, 1, fb, window="gaussian") as ctx:
        got = ctx.farneback(prev, nxt)[0]
        ctx.set_window("box")
        box = ctx.farneback(prev, nxt)[0]
    e = tolerances.epe(got, exp)
    print(f"\n[gauss e2e] {W}x{H} pair {pair} levels {levels} winsize {winsize}: mean {e.mean():.3g} p99.9 {np.percentile(e, 99.9):.3g} "
          f"max {e.max():.3g} px; box vs gaussian reference: mean {tolerances.epe(box, exp).mean():.3g} px")
    tolerances.check_flow(got, exp, tag=f"gaussian {W}x{H}")                 # strict gate: no twins, no pixel excused
    assert tolerances.flow_gate(tolerances.epe(box, exp)) is not None       # the box window is not mistaken for it


# ---- schedules: the flow of a Gaussian context does not depend on how its launches are cut ------------------------------------
def test_band_major_and_two_streams_are_bit_identical(mav):
    from mavflow import _lib, synth
    W, H = 640, 480
    prev, nxt = synth.make_batch(W, H, 3, distinct=3)
    with _lib.Context(W, H, 3, window="gaussian") as c:
        c.set_option("pairs_in_flight", 1)
        c.set_option("bands", 1)
        ref = c.farneback(prev, nxt)
        for pif in (1, 2):
            c.set_option("pairs_in_flight", pif)
            for bands in (1, 2, 3):
                c.set_option("bands", bands)
                sc.dirty(c, W, H, 3)                   # (every compared call on buffers another picture has just gone through)
                assert np.array_equal(c.farneback(prev, nxt), ref), (pif, bands)
        c.set_option("group", 2)
        sc.dirty(c, W, H, 3)
        assert np.array_equal(c.farneback(prev, nxt), ref)
        c.set_window("box")
        assert not np.array_equal(c.farneback(prev, nxt), ref)


def test_small_batch_sequence_initial_flow_process_batch_and_depth(mav):
    from mavflow import _lib, synth
    W, H, B = 58, 174, 3
    prev, nxt = synth.make_batch(W, H, B, distinct=3)
    with _lib.Context(W, H, B, window="gaussian") as c:
        c.set_option("small_batch", 0)
        ref = c.farneback(prev, nxt)
        c.set_option("small_batch", 1)
        assert np.array_equal(c.farneback(prev, nxt), ref)
        seq = synth.make_sequence(W, H, 3)
        pairwise = np.stack([c.farneback(seq[i], seq[i + 1])[0] for i in range(2)])
        assert np.array_equal(c.farneback_sequence(seq), pairwise)
        assert np.array_equal(c.farneback(prev, nxt, initial_flow=np.zeros((B, H, W, 2), np.float32)), ref)
        smp = np.stack([synth.foe_samples(W, H, b) for b in range(B)])
        assert np.array_equal(c.process_batch(prev, nxt, smp)["flow"], ref)
        assert np.array_equal(c.farneback(prev.astype(np.uint16), nxt.astype(np.uint16)), ref)
        c.set_window("box")
        assert not np.array_equal(c.farneback(prev, nxt), ref)


# ---- interface ----------------------------------------------------------------------------------------------------------------
def test_window_round_trip_and_bad_values(mav):
    from mavflow import _lib
    assert _lib.OPTFLOW_FARNEBACK_GAUSSIAN == 256
    with _lib.Context(64, 48) as c:
        assert c.window == "box" and c.schedule_info(1)["window"] == "box"
        c.set_window("gaussian")
        assert c.window == "gaussian" and c.schedule_info(1)["window"] == "gaussian"
        c.set_window(_lib.WINDOW_BOX)
        assert c.window == "box"
        for bad in (2, -1):
            with pytest.raises(ValueError):
                c.set_window(bad)
        with pytest.raises(ValueError):
            c.set_window("triangle")
        assert c.window == "box"
    fb = _lib.fb_defaults()
    fb.flags = _lib.OPTFLOW_FARNEBACK_GAUSSIAN
    with pytest.raises(ValueError, match="mav_set_window"):
        _lib.Context(64, 48, 1, fb)
    with pytest.raises(ValueError):
        _lib.Context(64, 48, window="triangle")


def test_box_schedule_line_is_untouched(mav):
    """mav_schedule_info of a box context, byte for byte, before and after a Gaussian context existed in the process and after the
    context itself went gaussian and back; a Gaussian context's line is the box line with one field appended."""
    import ctypes as C
    from mavflow import _lib

    def line(c, batch=2):
        buf = C.create_string_buffer(8192)
        _lib.check(c.lib.mav_schedule_info(c.h, batch, buf, len(buf)))
        return buf.value

    with _lib.Context(640, 480, 2) as c:
        before = line(c)
        assert b"window" not in before and b"gauss" not in before
        with _lib.Context(640, 480, 2, window="gaussian") as g:
            assert line(g) == before[:-1] + b', "window": "gaussian"}'
        assert line(c) == before
        c.set_window("gaussian")
        assert line(c) == before[:-1] + b', "window": "gaussian"}'
        c.set_window("box")
        assert line(c) == before


def test_cv2_signature_function(mav):
    from mavflow import _lib, synth
    from mavflow.farneback import calcOpticalFlowFarneback
    W, H = 96, 64
    prev, nxt = synth.make_pair(W, H, 1)[:2]
    args = (0.4, 1, 12, 10, 8, 1.2)
    fb = _lib.fb_defaults()
    init = (synth.true_flow(W, H) * 0.5).astype(np.float32)
    with _lib.Context(W, H, window="gaussian") as g, _lib.Context(W, H) as b:
        gauss, box = g.farneback(prev, nxt)[0], b.farneback(prev, nxt)[0]
        gauss_init = g.farneback(prev, nxt, initial_flow=init)[0]
        box_init = b.farneback(prev, nxt, initial_flow=init)[0]
    assert (fb.pyr_scale, fb.levels, fb.winsize, fb.iterations, fb.poly_n, fb.poly_sigma) == args
    assert not np.array_equal(gauss, box) and not np.array_equal(gauss_init, gauss)
    assert np.array_equal(calcOpticalFlowFarneback(prev, nxt, None, *args, 256), gauss)
    assert np.array_equal(calcOpticalFlowFarneback(prev, nxt, None, *args, 0), box)
    assert np.array_equal(calcOpticalFlowFarneback(prev, nxt, init.copy(), *args, 260), gauss_init)
    assert np.array_equal(calcOpticalFlowFarneback(prev, nxt, init.copy(), *args, 4), box_init)
    with pytest.raises(ValueError):
        calcOpticalFlowFarneback(prev, nxt, None, *args, 8)


def test_farneback_shim_honours_the_flag(mav):
    from mavflow import _lib, synth
    from mavflow.farneback import Farneback

    class Cap:
        def __init__(self, frames):
            self.frames = list(frames)

        def read(self):
            return True, self.frames.pop(0)

    class Gaussian(Farneback):
        PARAMS = dict(Farneback.PARAMS, flags=_lib.OPTFLOW_FARNEBACK_GAUSSIAN)

    W, H = 96, 64
    prev, nxt = synth.make_pair(W, H, 1)[:2]
    f = Gaussian(Cap([prev, nxt]))
    assert f.ctx.window == "gaussian"
    f.process()
    with _lib.Context(W, H, window="gaussian") as g:
        assert np.array_equal(f.flow, g.farneback(prev, nxt)[0])
    f.ctx.close()
