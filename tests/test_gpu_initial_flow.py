"""OPTFLOW_USE_INITIAL_FLOW on the MI355X: cv2.calcOpticalFlowFarneback(prev, next, flow0, ..., flags=OPTFLOW_USE_INITIAL_FLOW) through
mav_farneback_init / mav_farneback_init_dev and the Python surface (Context.farneback(initial_flow=), farneback_chain, the Farneback
shim).  The expected values come from tests/initial_flow_ref.py, the oracle's stage functions with the top layer's INTER_AREA start."""

import numpy as np
import pytest

import initial_flow_ref as ref
import schedule_cases as sc
from mavflow import synth
from oracle import fb_oracle as fbo
from oracle.tolerances import check_flow

pytestmark = pytest.mark.gpu


def _fb(**kw):
    from mavflow import _lib
    fb = _lib.fb_defaults()
    for k, v in kw.items():
        setattr(fb, k, v)
    return fb


def _params(fb):
    return fbo.Params(fb.pyr_scale, fb.levels, fb.winsize, fb.iterations, fb.poly_n, fb.poly_sigma, 0)


def _inits(W, H, B, seed=3):
    return np.stack([ref.smooth_initial_flow(W, H, seed + b) for b in range(B)])


# ---- 1. an all-zero initial flow is the flags = 0 computation ------------------------------------------------------------
@pytest.mark.parametrize("size,batch,levels,group", [((1280, 720), 1, 1, 0),      # small group: the pyramid from two launches
                                                     ((1920, 1080), 2, 1, 0),     # two pairs in flight, band-major initial M
                                                     ((320, 240), 20, 1, 4),      # deep batch: the top layer runs for all 20 pairs
                                                     ((3840, 2160), 1, 5, 0)])    # bands
def test_zero_initial_flow_is_bit_identical_to_no_initial_flow(mav, size, batch, levels, group):
    from mavflow import _lib
    W, H = size
    prev, nxt = synth.make_batch(W, H, batch, distinct=min(batch, 4))
    with _lib.Context(W, H, batch, _fb(levels=levels)) as c:
        if group:
            c.set_option("group", group)
        ref0 = c.farneback(prev, nxt).copy()
        got = c.farneback(prev, nxt, initial_flow=np.zeros((batch, H, W, 2), np.float32))
        assert np.array_equal(got, ref0), int((got != ref0).sum())


# ---- 2. against the checker ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,kw", [((640, 480), {}), ((1920, 1080), {}),
                                     ((640, 480), {"iterations": 1}),                 # the resized start reaches the output almost as it is
                                     ((640, 480), {"pyr_scale": 0.5}),                # ratio 2: the fast-area path
                                     ((640, 480), {"pyr_scale": 0.5, "iterations": 1}),
                                     ((640, 480), {"levels": 0}),                     # the start is the field itself
                                     ((333, 227), {"iterations": 1}),                 # ragged ratio
                                     ((3840, 2160), {"levels": 5})])
def test_initial_flow_matches_the_checker(mav, fb_oracle, size, kw):
    from mavflow import _lib
    W, H = size
    fb = _fb(**kw)
    k = 0.004 if W >= 3840 else 0.01                  # the 4K pair of tests/test_gpu_flow.py: a gentler radial field
    f0, f1, _ = synth.make_pair(W, H, 7 if W >= 3840 else 2, k=k)
    init = ref.smooth_initial_flow(W, H, k=k)
    with _lib.Context(W, H, 1, fb) as c:
        got = c.farneback(f0, f1, initial_flow=init)[0]
        zero = c.farneback(f0, f1)[0]
    exp = ref.calc_init(fb_oracle, f0, f1, init, _params(fb))
    check_flow(got, exp, f"initial flow {size} {kw}")
    if fb.iterations == 1 or fb.levels == 0:
        # the start reaches the result (with ten sweeps on two or more layers both starts converge to the same flow here)
        assert np.abs(got - zero).max() > 1e-2
        assert np.abs(ref.calc_init(fb_oracle, f0, f1, np.zeros_like(init), _params(fb)) - exp).max() > 1e-2


# ---- 3. every schedule gives the same bits with a non-zero initial flow --------------------------------------------------
@pytest.mark.parametrize("size,batch", [((640, 480), 5), ((1920, 1080), 3)])
def test_schedule_options_are_bit_identical_with_an_initial_flow(mav, size, batch):
    from mavflow import _lib
    W, H = size
    prev, nxt = synth.make_batch(W, H, batch, distinct=batch)
    init = _inits(W, H, batch)
    other = -0.5 * _inits(W, H, batch, seed=40)                      # the start of the picture that dirties the buffers

    def dirty(c, n):                                                   # every compared call on buffers another picture has just gone through
        sc.dirty(c, W, H, n, call=lambda p, q: c.farneback(p, q, initial_flow=other[:n]))

    with _lib.Context(W, H, batch) as c:
        c.set_option("pairs_in_flight", 1)
        c.set_option("group", 1)
        c.set_option("small_batch", 0)
        want = c.farneback(prev, nxt, initial_flow=init).copy()
        c.set_option("small_batch", 1)
        dirty(c, batch)
        assert np.array_equal(c.farneback(prev, nxt, initial_flow=init), want), "small_batch"
        for b in range(batch):                                         # one pair per call
            dirty(c, 1)
            assert np.array_equal(c.farneback(prev[b], nxt[b], initial_flow=init[b])[0], want[b]), b
        variants = [dict(group=g, pairs_in_flight=pif) for g in (2, batch) for pif in (1, 2)]
        variants += [dict(group=batch, group_fine=0), dict(group=batch, share_m=0), dict(group=2, deep_batch=0),
                     dict(group=2, pairs_in_flight=2, band_skew=0), dict(group=2, pairs_in_flight=2, coarse_half=1)]
        if H >= 1080:
            variants += [dict(group=g, pairs_in_flight=pif, bands=J) for g in (1, batch) for pif in (1, 2) for J in (2, 3, 4)]
        for v in variants:
            for k, val in v.items():
                c.set_option(k, val)
            dirty(c, batch)
            got = c.farneback(prev, nxt, initial_flow=init)
            assert np.array_equal(got, want), (v, int((got != want).sum()))
            for k in v:
                c.set_option(k, {"group": batch, "pairs_in_flight": 2, "bands": 0, "group_fine": 1, "share_m": 1, "deep_batch": 1,
                                 "band_skew": -1, "coarse_half": 0}[k])


def test_deep_batch_and_frame_sequences_with_an_initial_flow(mav):
    """320x240 x 20 in groups of 4: the top layer runs in the deep set, once for the call.  And a frame sequence (next = prev + one
    frame: share_frames) with an initial flow per pair."""
    from mavflow import _lib
    W, H, B = 320, 240, 20
    frames = synth.make_sequence(W, H, B + 1)
    prev, nxt = frames[:-1].copy(), frames[1:].copy()
    init = _inits(W, H, B)
    with _lib.Context(W, H, B) as c:
        c.set_option("group", 4)
        assert c.schedule_info(B)["deep_pairs"] > 0
        want = c.farneback(prev, nxt, initial_flow=init).copy()
        c.set_option("deep_batch", 0)
        assert np.array_equal(c.farneback(prev, nxt, initial_flow=init), want)
        c.set_option("deep_batch", 1)
        assert np.array_equal(c.farneback(frames[:-1], frames[1:], initial_flow=init), want)       # one run: the frames shared
        c.set_option("share_frames", 0)
        assert np.array_equal(c.farneback(frames[:-1], frames[1:], initial_flow=init), want)
        c.set_option("share_frames", 1)
        for b in (0, 7, 19):
            assert np.array_equal(c.farneback(prev[b], nxt[b], initial_flow=init[b])[0], want[b]), b


# ---- 4. in place ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,batch,kw,opts", [((640, 480), 3, {}, {}),
                                                ((640, 480), 3, {"levels": 0, "iterations": 1}, {}),
                                                ((1920, 1080), 2, {"levels": 0, "iterations": 1}, {"bands": 4, "pairs_in_flight": 2}),
                                                ((1920, 1080), 2, {"levels": 0, "iterations": 1}, {"bands": 4, "pairs_in_flight": 1}),
                                                ((1920, 1080), 2, {"iterations": 1}, {"bands": 4})])
def test_in_place_equals_out_of_place(mav, size, batch, kw, opts):
    """flow_init == flow (cv2's idiom): the top layer's start is a snapshot taken before anything writes the output -- with levels = 0,
    one sweep and band-major initial M, band j's initial M would otherwise read rows band j - 1 has already overwritten."""
    from mavflow import _lib
    W, H = size
    prev, nxt = synth.make_batch(W, H, batch, distinct=batch)
    init = _inits(W, H, batch)
    with _lib.Context(W, H, batch, _fb(**kw)) as c:
        for k, v in opts.items():
            c.set_option(k, v)
        want = c.farneback(prev, nxt, initial_flow=init).copy()
        # host pointers, one array for both
        lib = c.lib
        buf = init.copy()
        _lib.check(lib.mav_farneback_init(c.h, _lib._ptr(prev), _lib._ptr(nxt), batch, _lib._ptr(buf), _lib._ptr(buf)))
        assert np.array_equal(buf, want)
        # device pointers, out of place and in place
        dp, dn = c.alloc(prev.nbytes).upload(prev), c.alloc(nxt.nbytes).upload(nxt)
        di, df = c.alloc(init.nbytes).upload(init), c.alloc(init.nbytes)
        c.farneback_dev(dp.ptr, dn.ptr, batch, df.ptr, flow_init_ptr=di.ptr)
        c.sync()
        assert np.array_equal(df.download(np.float32, init.shape), want)
        c.farneback_dev(dp.ptr, dn.ptr, batch, di.ptr, flow_init_ptr=di.ptr)
        c.sync()
        assert lib.mav_last_flow_dev(c.h) == di.ptr
        assert np.array_equal(di.download(np.float32, init.shape), want)
        for b in range(batch):
            assert np.array_equal(c.last_flow(b), want[b])
        # ranges that overlap without being the same field are refused before anything is enqueued
        fbytes = W * H * 2 * 4
        with pytest.raises(ValueError, match="overlap"):
            c.farneback_dev(dp.ptr, dn.ptr, 1, df.ptr, flow_init_ptr=df.ptr + fbytes // 2)
        for d in (dp, dn, di, df):
            d.free()


# ---- 5. what the feature is for: motions the zero start cannot capture --------------------------------------------------
def test_a_start_near_the_truth_recovers_a_shift_the_zero_start_cannot(mav):
    from mavflow import _lib
    W, H = 320, 240
    shift = (15.3, -6.6)                  # CPU checker, levels 0: zero start mean error 17 px; start (15.3, -7.3): 0.012 px
    f0, f1 = ref.textured_translation(W, H, shift)
    init = np.empty((H, W, 2), np.float32)
    init[..., 0], init[..., 1] = round(shift[0]) + 0.3, round(shift[1]) - 0.3
    s = np.s_[30:-30, 30:-30]
    with _lib.Context(W, H, 1, _fb(levels=0)) as c:
        zero = c.farneback(f0, f1)[0]
        got = c.farneback(f0, f1, initial_flow=init)[0]
    e_zero = np.hypot(zero[..., 0][s] - shift[0], zero[..., 1][s] - shift[1])
    e_init = np.hypot(got[..., 0][s] - shift[0], got[..., 1][s] - shift[1])
    assert e_zero.mean() > 5, e_zero.mean()
    assert e_init.mean() <= 0.05, e_init.mean()


# ---- 6. Python surface ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_init", [False, True])
def test_farneback_chain_equals_a_host_loop(mav, with_init):
    from mavflow import _lib
    W, H, n = 640, 480, 5
    frames = synth.make_sequence(W, H, n + 1)
    init0 = ref.smooth_initial_flow(W, H) if with_init else None
    with _lib.Context(W, H, 1) as c:
        got = c.farneback_chain(frames, initial_flow=init0)
        prevf, want = init0, []
        for i in range(n):
            f = c.farneback(frames[i], frames[i + 1], initial_flow=prevf)[0].copy()
            want.append(f)
            prevf = f
        assert got.shape == (n, H, W, 2)
        assert np.array_equal(got, np.stack(want))
        assert np.array_equal(got[0], c.farneback(frames[0], frames[1])[0]) != with_init


class _Frames:
    def __init__(self, frames):
        self.frames, self.i = list(frames), 0

    def read(self):
        f = self.frames[self.i]
        self.i += 1
        return True, f


def test_farneback_shim_with_the_flag_starts_from_its_previous_flow(mav):
    from mavflow import _lib
    from mavflow.farneback import Farneback

    class Warm(Farneback):
        PARAMS = dict(Farneback.PARAMS, flags=_lib.OPTFLOW_USE_INITIAL_FLOW)

    W, H = 320, 240
    frames = synth.make_sequence(W, H, 3)
    plain, warm = Farneback(_Frames(frames)), Warm(_Frames(frames))
    plain.process(); warm.process()
    assert np.array_equal(warm.flow, plain.flow)                      # before the first frame the previous flow is zero
    first = warm.flow.copy()
    plain.process(); warm.process()
    with _lib.Context(W, H, 1) as c:
        assert np.array_equal(warm.flow, c.farneback(frames[1], frames[2], initial_flow=first)[0])
        assert np.array_equal(plain.flow, c.farneback(frames[1], frames[2])[0])
    assert not np.array_equal(warm.flow, plain.flow)
    warm.ctx.close(); plain.ctx.close()


def test_arguments(mav):
    from mavflow import _lib
    W, H = 320, 240
    prev, nxt = synth.make_batch(W, H, 2, distinct=2)
    with _lib.Context(W, H, 2, _fb(flags=_lib.OPTFLOW_USE_INITIAL_FLOW)) as c:        # a cv2 argument list with the flag passes
        # the bit alone starts nothing from a field: the calls without one start from zero
        with _lib.Context(W, H, 2) as c0:
            assert np.array_equal(c.farneback(prev, nxt), c0.farneback(prev, nxt))
        for bad in (np.zeros((H, W, 2), np.float32),                    # one field for two pairs
                    np.zeros((2, H, W), np.float32), np.zeros((2, W, H, 2), np.float32), np.zeros((2, H, W, 2), np.float64)):
            with pytest.raises(ValueError):
                c.farneback(prev, nxt, initial_flow=bad)
        out = np.empty((2, H, W, 2), np.float32)
        with pytest.raises(ValueError):
            _lib.check(c.lib.mav_farneback_init(c.h, _lib._ptr(prev), _lib._ptr(nxt), 2, None, _lib._ptr(out)))
        d = c.alloc(out.nbytes)
        with pytest.raises(ValueError):
            c.farneback_dev(d.ptr, d.ptr, 1, d.ptr, flow_init_ptr=0)
        d.free()
        with pytest.raises(ValueError):
            c.farneback_chain(prev[:1])
        with pytest.raises(ValueError):
            c.farneback_chain(np.concatenate([prev, nxt]), initial_flow=np.zeros((2, H, W, 2), np.float32))
    for flags in (256, 4 | 256, 1, 8):
        with pytest.raises(ValueError):
            _lib.Context(W, H, 1, _fb(flags=flags))


def test_workspace_grows_only_with_the_first_initial_flow_call(mav):
    from mavflow import _lib
    W, H, B = 640, 480, 2
    prev, nxt = synth.make_batch(W, H, B, distinct=B)
    with _lib.Context(W, H, B) as a, _lib.Context(W, H, B, _fb(flags=_lib.OPTFLOW_USE_INITIAL_FLOW)) as b:
        a.farneback(prev, nxt)
        b.farneback(prev, nxt)
        ws = a.mem_info()["workspace_bytes"]
        assert ws > 0 and b.mem_info()["workspace_bytes"] == ws
        b.farneback(prev, nxt, initial_flow=_inits(W, H, B))
        w1, h1 = b.layer_dims(b.num_layers() - 1)[:2]
        grown = b.mem_info()["workspace_bytes"] - ws
        assert 0 < grown <= B * 4 * (2 * w1 * h1 + 64), grown
        b.farneback(prev, nxt, initial_flow=_inits(W, H, B))
        assert b.mem_info()["workspace_bytes"] == ws + grown
        assert a.mem_info()["workspace_bytes"] == ws
