"""16-bit and float32 frames on the MI355X (cv2.calcOpticalFlowFarneback on CV_16U / CV_32F input): mav_farneback_ex /
mav_farneback_ex_dev / mav_stage_blur_resize_ex / mav_schedule_info_ex and the Python surface that takes uint16 / float32 / float64.

  1. identity   frames that hold u8 values give the u8 flow bit for bit, whatever their dtype, through every entry point and schedule
  2. stage      layer images of genuine 16-bit / fractional float frames against tests/depth_ref.blur_resize_f32; fused == two-pass
  3. end to end genuine 16-bit / fractional float pairs against depth_ref.calc_depth through the strict gate
  4. scale      a [0, 1]-normalised pair is not rescaled
  5. refusals   other dtypes, mixed dtypes, unknown depth codes
"""
import ctypes as C

import numpy as np
import pytest

import depth_ref
from mavflow import synth
from oracle import fb_oracle as fbo
from oracle.tolerances import check_flow
from stage_cases import COARSE_REL, F32_LAYER0_REL

pytestmark = pytest.mark.gpu

WIDE = (np.uint16, np.float32, np.float64)


def _fb(**kw):
    from mavflow import _lib
    fb = _lib.fb_defaults()
    for k, v in kw.items():
        setattr(fb, k, v)
    return fb


def _params(fb):
    return fbo.Params(fb.pyr_scale, fb.levels, fb.winsize, fb.iterations, fb.poly_n, fb.poly_sigma, 0)


# ---- 1. identity ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,levels,batch,group", [((640, 480), 1, 1, 0), ((640, 480), 1, 20, 4),       # small group / deep + groups
                                                     ((1000, 562), 1, 3, 0), ((333, 227), 1, 2, 0),
                                                     ((58, 174), 1, 2, 0), ((1920, 1080), 1, 1, 0),
                                                     ((1920, 1080), 1, 4, 2), ((3840, 2160), 5, 1, 0)])
def test_u8_values_give_the_u8_flow_at_every_depth(mav, size, levels, batch, group):
    from mavflow import _lib
    W, H = size
    prev, nxt = synth.make_batch(W, H, batch, distinct=min(batch, 4))
    with _lib.Context(W, H, batch, _fb(levels=levels)) as c:
        if group:
            c.set_option("group", group)
        ref = c.farneback(prev, nxt).copy()
        for dt in WIDE:
            got = c.farneback(prev.astype(dt), nxt.astype(dt))
            assert np.array_equal(got, ref), (np.dtype(dt).name, int((got != ref).sum()))


@pytest.mark.parametrize("size,levels", [((640, 480), 1), ((333, 227), 1), ((1920, 1080), 1)])
def test_u8_values_sequence_chain_initial_flow_and_dev(mav, size, levels):
    from mavflow import _lib
    import initial_flow_ref
    W, H = size
    n = 3
    video = synth.make_sequence(W, H, n + 1) if hasattr(synth, "make_sequence") else None
    if video is None:
        p, q = synth.make_batch(W, H, n, distinct=n)
        video = np.concatenate([p, q[-1:]], 0)
    f0 = initial_flow_ref.smooth_initial_flow(W, H)
    with _lib.Context(W, H, n, _fb(levels=levels)) as c:
        seq_ref = c.farneback_sequence(video).copy()
        chain_ref = c.farneback_chain(video, initial_flow=f0).copy()
        init_ref = c.farneback(video[:1], video[1:2], initial_flow=f0).copy()
        px = W * H
        d_flow = c.alloc(n * px * 2 * 4)
        try:
            for dt in WIDE:
                v = video.astype(dt)
                assert np.array_equal(c.farneback_sequence(v), seq_ref), np.dtype(dt).name
                assert np.array_equal(c.farneback_chain(v, initial_flow=f0), chain_ref), np.dtype(dt).name
                assert np.array_equal(c.farneback(v[:1], v[1:2], initial_flow=f0), init_ref), np.dtype(dt).name
                # the _dev form on a frame run (next = prev + one frame), depth given as a dtype
                v32 = v.astype(np.float32) if v.dtype == np.float64 else v
                d_frames = c.alloc(v32.nbytes).upload(np.ascontiguousarray(v32))
                try:
                    c.farneback_dev(d_frames.ptr, d_frames.ptr + px * v32.itemsize, n, d_flow.ptr, depth=v32.dtype)
                    c.sync()
                    assert np.array_equal(d_flow.download(np.float32, (n, H, W, 2)), seq_ref), np.dtype(dt).name
                finally:
                    c.sync()
                    d_frames.free()
        finally:
            d_flow.free()


# ---- 2. stage ------------------------------------------------------------------------------------------------------------
# bounds: stage_cases.F32_LAYER0_REL / COARSE_REL, max |GPU - checker| / max |checker| of a layer image
def _stage_frames(W, H):
    img16 = depth_ref.pair16(W, H)[0]
    return {"uint16": img16, "float32": (img16.astype(np.float64) / 257.0).astype(np.float32)}


@pytest.mark.parametrize("size,levels", [((640, 480), 1), ((1920, 1080), 1), ((333, 227), 1), ((3840, 2160), 5)])
def test_stage_layer_images_of_wide_frames(mav, fb_oracle, size, levels):
    from mavflow import _lib
    W, H = size
    worst = {}
    with _lib.Context(W, H, 1, _fb(levels=levels)) as c:
        for name, img in _stage_frames(W, H).items():
            for k in range(c.num_layers()):
                w, h, sigma, ks = c.layer_dims(k)
                exp = depth_ref.blur_resize_f32(img, w, h, ks, sigma, fb_oracle)
                got = c.stage_blur_resize(img, k)
                if k == 0 and name == "uint16":
                    assert np.array_equal(got, exp), (name, k, float(np.abs(got - exp).max()))    # taps 1/4, 1/2, 1/4: exact
                    continue
                rel = float(np.abs(got.astype(np.float64) - exp).max() / np.abs(exp).max())
                worst[(name, k)] = rel
                assert rel <= (F32_LAYER0_REL if k == 0 else COARSE_REL), (name, k, ks, rel)
    print("worst relative error per (dtype, layer):", {f"{a}/{b}": f"{v:.2e}" for (a, b), v in worst.items()})


@pytest.mark.parametrize("size,levels", [((640, 480), 1), ((1920, 1080), 1), ((333, 227), 1), ((1000, 562), 1), ((3840, 2160), 5)])
def test_fused_equals_two_pass_for_wide_frames(mav, size, levels):
    from mavflow import _lib
    W, H = size
    rng = np.random.default_rng(11)
    with _lib.Context(W, H, 1, _fb(levels=levels)) as c:
        for name, img in _stage_frames(W, H).items():
            noise = rng.integers(0, 65536, (H, W)).astype(img.dtype) if name == "uint16" else rng.random((H, W), np.float32) * 255
            fused = [l["layer"] for l in c.schedule_info(1, img.dtype)["layers"] if l["blur"] == "fused"]
            assert fused, (name, c.schedule_info(1, img.dtype))
            for k in range(1, c.num_layers()):
                for x in (img, noise):
                    a, b = c.stage_blur_resize(x, k), c.stage_blur_resize(x, k, two_pass=True)
                    assert np.array_equal(a, b), (name, k, int((a != b).sum()))


def test_schedule_query_names_every_form_per_depth(mav):
    """mav_schedule_info_ex: u8 is mav_schedule_info byte for byte; the wide depths reach the 3x3, fused and two-pass forms, and where
    a staged fused tile of 2 / 4-byte pixels would not fit 64 KB of LDS (layer 2 of the 4K / 5-layer preset) they take the two-pass
    form while u8 keeps its 64 x 8 fused tile."""
    from mavflow import _lib
    lib = _lib.load()
    with _lib.Context(3840, 2160, 16, _fb(levels=5)) as c:
        for b in (1, 16):
            plain = C.create_string_buffer(8192); ex = C.create_string_buffer(8192)
            assert lib.mav_schedule_info(c.h, b, plain, len(plain)) == 0
            assert lib.mav_schedule_info_ex(c.h, b, _lib.DEPTH_8U, ex, len(ex)) == 0
            assert plain.value == ex.value
        blur = {dt: [l["blur"] for l in c.schedule_info(16, dt)["layers"]] for dt in (np.uint8, np.uint16, np.float32)}
        assert blur[np.uint8][:3] == ["3x3", "fused", "fused"], blur
        for dt in (np.uint16, np.float32):
            assert blur[dt][:3] == ["3x3", "fused", "two-pass"], (dt, blur)
            assert set(blur[dt]) == {"3x3", "fused", "two-pass"}
    with _lib.Context(1280, 720, 1) as c:                    # a small group: the whole pyramid through k_blur_multi
        for dt in (np.uint16, np.float32):
            s = c.schedule_info(1, dt)
            assert s["pyramid_in_two_launches"] and [l["blur"] for l in s["layers"]] == ["3x3", "fused"], s


# ---- 3. end to end -------------------------------------------------------------------------------------------------------
# 16-bit frames at 4K with 5 levels are not gated: at 65535-scale intensities the solve's 1e-3 regulariser is ~4e9 times weaker than at
# 255-scale, the coarse layers' 2x2 systems are near-singular in flat regions, and two float32 implementations of the SAME arithmetic
# part there by pixels (measured: mean EPE 3e-3 .. 160 px over six synth scenes -- GPU vs checker, whose layer images agree to 5e-7
# relative).  The layer images of that configuration are pinned by test_stage_layer_images_of_wide_frames, and u8-valued 16-bit
# frames give the u8 flow there bit for bit (test_u8_values_give_the_u8_flow_at_every_depth).
@pytest.mark.parametrize("dtype,size,levels", [("uint16", (640, 480), 1), ("uint16", (1920, 1080), 1),
                                               ("float32", (640, 480), 1), ("float32", (1920, 1080), 1), ("float32", (3840, 2160), 5)])
def test_wide_frames_match_the_checker(mav, fb_oracle, dtype, size, levels):
    from mavflow import _lib
    W, H = size
    fb = _fb(levels=levels)
    p = _params(fb)
    a16, b16 = depth_ref.pair16(W, H)
    if dtype == "uint16":
        a, b = a16, b16
    else:                                                     # fractional values on the 0 .. 255 scale
        a, b = a16.astype(np.float32) / np.float32(257), b16.astype(np.float32) / np.float32(257)
    with _lib.Context(W, H, 1, fb) as c:
        got = c.farneback(a, b)[0].copy()
        check_flow(got, depth_ref.calc_depth(fb_oracle, a, b, p), f"{dtype} {W}x{H}")
        if dtype == "uint16":
            hi = c.farneback((a16 >> 8).astype(np.uint8), (b16 >> 8).astype(np.uint8))[0]
            assert float(np.abs(got - hi).max()) > 1e-3        # the low byte is used


# ---- 4. scale ------------------------------------------------------------------------------------------------------------
def test_normalised_float_frames_are_not_rescaled(mav, fb_oracle):
    from mavflow import _lib
    W, H = 640, 480
    fb = _fb()
    a, b = synth.make_batch(W, H, 1)
    a01, b01 = a[0].astype(np.float32) / np.float32(255), b[0].astype(np.float32) / np.float32(255)
    with _lib.Context(W, H, 1, fb) as c:
        got = c.farneback(a01, b01)[0].copy()
        full = c.farneback(a, b)[0]
    exp = depth_ref.calc_depth(fb_oracle, a01, b01, _params(fb))
    check_flow(got, exp, "[0, 1] float32")
    mg, me = float(np.abs(got).mean()), float(np.abs(exp).mean())
    assert abs(mg - me) <= 0.01 * me, (mg, me)
    assert mg < 0.5 * float(np.abs(full).mean())              # cv2's 1e-3 regulariser: normalised frames give much smaller flow


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------
def test_other_dtypes_and_codes_are_refused(mav):
    from mavflow import _lib
    lib = _lib.load()
    W, H = 64, 48
    a, b = synth.make_batch(W, H, 1)
    with _lib.Context(W, H, 2) as c:
        for dt in (np.int16, np.int32, np.bool_):
            with pytest.raises(ValueError, match="uint8, uint16 or float32"):
                c.farneback(a.astype(dt), b.astype(dt))
            with pytest.raises(ValueError, match="uint8, uint16 or float32"):
                c.farneback_sequence(np.concatenate([a, b]).astype(dt))
            with pytest.raises(ValueError, match="uint8, uint16 or float32"):
                c.farneback_chain(np.concatenate([a, b]).astype(dt))
            with pytest.raises(ValueError, match="uint8, uint16 or float32"):
                c.stage_blur_resize(a[0].astype(dt), 0)
            with pytest.raises(ValueError):
                c.schedule_info(1, dt)
        with pytest.raises(ValueError, match="differ in dtype"):
            c.farneback(a.astype(np.uint16), b.astype(np.float32))
        with pytest.raises(ValueError, match="differ in dtype"):
            c.farneback(a, b.astype(np.uint16))
        # unknown depth codes: MAV_ERR_ARG, the output untouched (nothing enqueued)
        pa, pb = np.ascontiguousarray(a.astype(np.uint16)), np.ascontiguousarray(b.astype(np.uint16))
        flow = np.full((1, H, W, 2), 7.0, np.float32)
        ptr = lambda x: x.ctypes.data_as(C.c_void_p)
        for depth in (1, 3, 4, 6, -1, 99):
            assert lib.mav_farneback_ex(c.h, ptr(pa), ptr(pb), depth, 1, None, ptr(flow)) == -1, depth
            assert (flow == 7.0).all()
            out = np.full((H, W), 7.0, np.float32)
            assert lib.mav_stage_blur_resize_ex(c.h, ptr(pa[0]), depth, 0, 0, ptr(out)) == -1
            assert (out == 7.0).all()
            buf = C.create_string_buffer(8192)
            assert lib.mav_schedule_info_ex(c.h, 1, depth, buf, len(buf)) == -1
            with pytest.raises(ValueError):
                c.farneback_dev(0, 0, 1, 0, depth=depth)
        d = c.alloc(2 * W * H * 2)
        try:
            assert lib.mav_farneback_ex_dev(c.h, d.ptr, d.ptr + W * H * 2, 3, 1, None, d.ptr) == -1
        finally:
            d.free()
        # the context still computes afterwards
        assert np.isfinite(c.farneback(a.astype(np.uint16), b.astype(np.uint16))).all()
