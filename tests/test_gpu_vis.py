"""The flow pictures on the device (include/mavflow_vis.h) against their definitions, byte for byte, on every case of tests/vis_cases.py:
MAV_HSV_PROCESS against mavflow.farneback.flow_to_hsv / hsv_to_bgr (the existing host functions), MAV_HSV_DRAW against the
reference-made fixture, the colour conversions against hsv_to_bgr and vis_ref.bgr2hsv, draw_flow against vis_ref.draw_flow.

atan2f is the one operation that is not IEEE arithmetic in a fixed order: the constructed fields keep every hue at least 0.1 away from a
whole number (asserted on the host first), so no tolerance exists or is needed; on real Farneback flows a pixel may differ only inside
the 5e-4 hue band, by one hue step, and the band's share is asserted on the host."""
import os

import numpy as np
import pytest

import vis_cases as vc
import vis_ref as R

pytestmark = pytest.mark.gpu
GUARD = 64                                         # bytes in front of and behind every picture of the enqueue forms (a multiple of 16)
FILL = 0xA5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vis.npz")


@pytest.fixture(scope="module")
def fixture():
    return vc.load_fixture(GOLDEN)


class Guarded:
    """a device block of `nbytes` at `offset` bytes behind a 16-aligned address, between two guards"""

    def __init__(self, ctx, nbytes, offset, init=None):
        self.nbytes, self.offset = nbytes, offset
        raw = np.full(GUARD + offset + nbytes + GUARD, FILL, np.uint8)
        if init is not None:
            raw[GUARD + offset:GUARD + offset + nbytes] = np.ascontiguousarray(init).reshape(-1).view(np.uint8)
        self.buf = ctx.alloc(raw.nbytes).upload(raw)
        self.ptr = self.buf.ptr + GUARD + offset
        assert self.buf.ptr % 16 == 0

    def take(self):
        """the block's bytes; asserts the guards are untouched; frees the block"""
        raw = self.buf.download(np.uint8, (self.buf.nbytes,))
        self.buf.free()
        a = GUARD + self.offset
        assert (raw[:a] == FILL).all() and (raw[a + self.nbytes:] == FILL).all(), "bytes outside the picture were written"
        return raw[a:a + self.nbytes]


def flow_hsv_dev(ctx, flow, mode, offset=0, want_hsv=True):
    """mav_flow_hsv_dev on caller-owned blocks -> (bgr, hsv | None, records)"""
    from mavflow import vis
    Bn, H, W = flow.shape[:3]
    n = Bn * H * W
    fb = ctx.alloc(flow.nbytes).upload(flow)
    bgr, hsv, rec = Guarded(ctx, 3 * n, offset), Guarded(ctx, 3 * n, offset), Guarded(ctx, 16 * Bn, 0)
    assert vis.vis_form(W, H, Bn, fb.ptr, bgr.ptr, hsv.ptr if want_hsv else None) == vc.form_of(W, H, Bn, 0, offset, offset if want_hsv else None)
    ctx.flow_hsv_enqueue(fb.ptr, bgr.ptr, rec.ptr, mode, hsv_ptr=hsv.ptr if want_hsv else None, batch=Bn)
    ctx.sync()
    fb.free()
    h = hsv.take()
    assert want_hsv or (h == FILL).all()
    return bgr.take().reshape(Bn, H, W, 3), h.reshape(Bn, H, W, 3) if want_hsv else None, rec.take().view(vis.RECORD_DTYPE)


def host_process(flow):
    """the definition: flow_to_hsv + hsv_to_bgr per image, and the record"""
    from mavflow import vis
    from mavflow.farneback import flow_to_hsv, hsv_to_bgr
    hs, bg, rec = [], [], np.zeros(len(flow), vis.RECORD_DTYPE)
    for b, f in enumerate(flow):
        hsv, invalid = flow_to_hsv(f)
        mag = np.sqrt(f[..., 0] * f[..., 0] + f[..., 1] * f[..., 1])
        lo, hi = float(mag.min()), float(mag.max())
        norm = np.zeros_like(mag) if hi - lo <= np.finfo(np.float64).eps else (mag - lo) * np.float32(255.0 / (hi - lo))
        nz = int(np.count_nonzero((norm * 2.0).astype(np.int64) & 255))
        assert invalid == (nz == 0)
        rec[b] = (mag.min(), mag.max(), nz, int(invalid))
        hs.append(hsv); bg.append(hsv_to_bgr(hsv))
    return np.stack(bg), np.stack(hs), rec


def assert_equal_process(got, want, what):
    (gb, gh, gr), (wb, wh, wr) = got, want
    assert gr.tobytes() == wr.tobytes(), (what, gr, wr)                     # mag_min and mag_max by bits, nonzero, invalid
    if gh is not None:
        assert np.array_equal(gh, wh), (what, "hsv", int((gh != wh).any(axis=-1).sum()))
    assert np.array_equal(gb, wb), (what, "bgr", int((gb != wb).any(axis=-1).sum()))


# ---- MAV_HSV_PROCESS ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", vc.CASES, ids=vc.case_id)
def test_process_equals_the_host_functions_on_constructed_fields(mav, case):
    from mavflow import _lib, vis  # noqa: F401
    flow = np.ascontiguousarray(vc.constructed_fields(case.W, case.H)[:case.batch])
    hue = R.process_hue_float(flow)
    assert np.abs(hue - np.rint(hue)).min() > 0.05 and not vc.in_band(hue).any()       # the margin is 0.1 by construction
    want = host_process(flow)
    if case.W * case.H > 1:
        lo, hi = want[2]["mag_min"], want[2]["mag_max"]
        mag = np.sqrt((flow.astype(np.float32) ** 2).sum(-1))
        assert all((mag[b] > (lo[b] + hi[b]) / 2).any() for b in range(case.batch))    # the upper half of the range, whose value wraps, is present
    with _lib.Context(case.W, case.H, vc.B) as ctx:
        assert_equal_process(flow_hsv_dev(ctx, flow, "process", case.offset, True), want, "dev, with hsv")
        assert_equal_process(flow_hsv_dev(ctx, flow, "process", case.offset, False), want, "dev, without hsv")
        if case.offset == 0:
            out = ctx.flow_hsv(flow if case.batch > 1 else flow[0], "process", hsv=True)
            lead = (slice(None),) if case.batch > 1 else (None,)
            assert_equal_process((out["bgr"][lead], out["hsv"][lead], np.atleast_1d(out["record"])), want, "host form")
            h = ctx.alloc(flow.nbytes).upload(flow)                                      # a device handle through the host-facing method
            try:
                out = ctx.flow_hsv(h, "process", hsv=True, batch=case.batch)
            finally:
                h.free()
            assert_equal_process((out["bgr"].reshape(want[0].shape), out["hsv"].reshape(want[1].shape), np.atleast_1d(out["record"])), want, "handle")


@pytest.mark.parametrize("W,H", [(131, 67), (17, 5)])
def test_process_on_degenerate_fields(mav, W, H):
    from mavflow import _lib, vis  # noqa: F401
    from mavflow.farneback import hsv_to_bgr
    repaint = hsv_to_bgr(np.array([[[127, 255, 255]]], np.uint8))[0, 0]
    const = np.full((H, W, 2), (1.5, -2.25), np.float32)
    zero = np.zeros((H, W, 2), np.float32)
    one = const.copy()
    one[H // 2, W - 1] = (3.0, 4.0)                                # exactly one differing pixel: its norm is 255, its value wraps
    flow = np.stack([const, zero, one])
    want = host_process(flow)
    assert list(want[2]["invalid"]) == [1, 1, 0] and list(want[2]["nonzero"]) == [0, 0, 1]
    with _lib.Context(W, H, vc.B) as ctx:
        for off in vc.OFFSETS:
            got = flow_hsv_dev(ctx, flow, "process", off, True)
            assert_equal_process(got, want, f"offset {off}")
            assert (got[0][:2] == repaint).all() and (got[1][:2] == (127, 255, 255)).all()
            assert tuple(got[1][2, H // 2, W - 1][:2]) == (26, 255) and got[1][2, H // 2, W - 1][2] >= 253      # 2 * 255 wraps to 254 (or 253: scale is rounded)
            assert (got[0][2] != repaint).any(axis=-1).sum() == 1


@pytest.mark.parametrize("W,H", [(131, 67), (66, 33)])
def test_process_on_real_farneback_flows(mav, W, H):
    """Every pixel that differs from the host functions lies in the 5e-4 hue band and differs by one hue step only; the band holds
    about 1e-3 of the pixels (hues spread over a step: 2 * 5e-4) -- asserted below 1e-2 on the host, so that it cannot hide a failure."""
    from mavflow import _lib, synth, vis  # noqa: F401
    from mavflow.farneback import hsv_to_bgr
    f0, f1, _ = synth.make_pair(W, H, 5)
    with _lib.Context(W, H, vc.B) as ctx:
        flow = np.ascontiguousarray(np.asarray(ctx.farneback(f0, f1))[:1], np.float32)
        band = vc.in_band(R.process_hue_float(flow))
        share = band.mean()
        print(f"real flow {W}x{H}: {int(band.sum())} of {band.size} pixels in the hue band (share {share:.2e})")
        assert share < 1e-2
        wb, wh, wr = host_process(flow)
        for off in vc.OFFSETS:
            gb, gh, gr = flow_hsv_dev(ctx, flow, "process", off, True)
            assert gr.tobytes() == wr.tobytes()
            diff = (gh != wh).any(axis=-1)
            print(f"  offset {off}: {int(diff.sum())} pixels differ, {int((diff & ~band).sum())} of them outside the band")
            assert not (diff & ~band).any()
            assert np.array_equal(gh[..., 1:], wh[..., 1:])                                  # saturation and value are IEEE arithmetic: equal
            step = np.abs(gh[..., 0].astype(int) - wh[..., 0].astype(int))
            assert (np.minimum(step, 180 - step)[diff] == 1).all()
            assert np.array_equal(gb, hsv_to_bgr(gh))                                         # the picture is the HSV image's, everywhere
            assert np.array_equal(gb[~diff], wb[~diff])


# ---- MAV_HSV_DRAW -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ("66x33", "131x67"))
def test_draw_equals_the_reference_made_image(mav, fixture, key):
    from mavflow import _lib, vis  # noqa: F401
    from mavflow.farneback import Farneback, hsv_to_bgr
    flow, want = fixture[f"flow_{key}"], fixture[f"hsv_{key}"]
    H, W = flow.shape[:2]
    assert not vc.in_band(R.draw_hue_float(flow)).any()              # else: regenerate the fixture with another seed
    with _lib.Context(W, H, vc.B) as ctx:
        for off in vc.OFFSETS:
            gb, gh, gr = flow_hsv_dev(ctx, flow[None], "draw", off, True)
            assert np.array_equal(gh[0], want) and np.array_equal(gb[0], hsv_to_bgr(want)) and not gr.tobytes().strip(b"\0")
        out = ctx.flow_hsv(flow, "draw")
        assert set(out) == {"bgr", "record"} and np.array_equal(out["bgr"], hsv_to_bgr(want))
    fb = Farneback.__new__(Farneback)                               # the method of the class, on a cached context of the field's size
    fb.ctx = type("C", (), {"W": 0, "H": 0})()
    assert np.array_equal(fb.draw_hsv(flow), hsv_to_bgr(want))
    with pytest.raises(TypeError, match="float64"):
        fb.draw_hsv(flow.astype(np.float64))


@pytest.mark.parametrize("case", [c for c in vc.CASES if c.batch == 3], ids=vc.case_id)
def test_draw_on_batches_of_constructed_fields(mav, case):
    from mavflow import _lib, vis  # noqa: F401
    from mavflow.farneback import hsv_to_bgr
    flow = np.ascontiguousarray(vc.constructed_fields(case.W, case.H)[:case.batch])
    assert not vc.in_band(R.draw_hue_float(flow)).any()
    want = R.draw_hsv_stage(flow)
    with _lib.Context(case.W, case.H, vc.B) as ctx:
        gb, gh, gr = flow_hsv_dev(ctx, flow, "draw", case.offset, True)
        assert np.array_equal(gh, want) and np.array_equal(gb, hsv_to_bgr(want)) and not gr.tobytes().strip(b"\0")
        gb, _, _ = flow_hsv_dev(ctx, flow, "draw", case.offset, False)
        assert np.array_equal(gb, hsv_to_bgr(want))


# ---- cvtColor -----------------------------------------------------------------------------------------------------------------------------
def cvt_dev(ctx, img, code, offset):
    src, dst = Guarded(ctx, img.nbytes, offset, img), Guarded(ctx, img.nbytes, offset)
    ctx.cvt_color_enqueue(src.ptr, code, dst.ptr, batch=img.shape[0])
    ctx.sync()
    assert np.array_equal(src.take(), img.reshape(-1))
    return dst.take().reshape(img.shape)


def test_hsv2bgr_equals_hsv_to_bgr_for_every_hue_and_value(mav):
    from mavflow import _lib, vis
    from mavflow.farneback import hsv_to_bgr
    h, s, v = np.meshgrid(np.arange(256), np.array([0, 1, 128, 254, 255]), np.arange(256), indexing="ij")
    tri = np.stack([h, s, v], -1).reshape(-1, 3).astype(np.uint8)
    want = hsv_to_bgr(tri)
    img = vc.as_frames(tri, 256, 256)
    with _lib.Context(256, 256, len(img)) as ctx:
        assert np.array_equal(ctx.cvt_color(img, vis.COLOR_HSV2BGR).reshape(-1, 3)[:len(tri)], want)
    part = vc.as_frames(tri, 131, 67)[:vc.B]                          # and through the enqueue form at both alignments
    with _lib.Context(131, 67, vc.B) as ctx:
        for off in vc.OFFSETS:
            assert np.array_equal(cvt_dev(ctx, part, vis.COLOR_HSV2BGR, off), hsv_to_bgr(part))


def test_bgr2hsv_equals_the_integer_path(mav):
    from mavflow import _lib, vis
    rng = np.random.default_rng(40)
    tri = np.concatenate([vc.lattice(), rng.integers(0, 256, (200000, 3), dtype=np.uint8)])
    want = R.bgr2hsv(tri)
    img = vc.as_frames(tri, 256, 256)
    with _lib.Context(256, 256, len(img)) as ctx:
        assert np.array_equal(ctx.cvt_color(img, vis.COLOR_BGR2HSV).reshape(-1, 3)[:len(tri)], want)
    part = vc.as_frames(tri[-131 * 67 * vc.B:], 131, 67)
    with _lib.Context(131, 67, vc.B) as ctx:
        for off in vc.OFFSETS:
            assert np.array_equal(cvt_dev(ctx, part, vis.COLOR_BGR2HSV, off), R.bgr2hsv(part))
            assert np.array_equal(cvt_dev(ctx, part[:1, :], vis.COLOR_BGR2HSV, off), R.bgr2hsv(part[:1]))
    one = tri[12345].reshape(1, 1, 1, 3)
    with _lib.Context(1, 1, 1) as ctx:
        assert np.array_equal(ctx.cvt_color(one, vis.COLOR_BGR2HSV), R.bgr2hsv(one))


def test_get_flow_radial_equals_the_composition(mav):
    from mavflow import im_helpers, vis
    from mavflow.farneback import hsv_to_bgr
    rng = np.random.default_rng(41)
    img = rng.integers(0, 256, (67, 131, 3), dtype=np.uint8)
    img[:8] = rng.integers(0, 256, (8, 131, 1), dtype=np.uint8)      # gray rows: d = 0
    want = R.flow_radial(img, hsv_to_bgr)
    assert np.array_equal(im_helpers.get_flow_radial(img), want)
    hsv = vis.cvtColor(img, vis.COLOR_BGR2HSV)                       # the two calls with the assignment between them
    assert np.array_equal(hsv, R.bgr2hsv(img))
    hsv[..., 1:] = 255
    assert np.array_equal(vis.cvtColor(hsv, vis.COLOR_HSV2BGR), want)
    with pytest.raises(NotImplementedError, match="COLOR_HSV2BGR"):
        vis.cvtColor(img, 6)


# ---- draw_flow ----------------------------------------------------------------------------------------------------------------------------
def draw_dev(ctx, img, flow, step, threshold, colour, offset=0):
    fb = ctx.alloc(flow.nbytes).upload(flow)
    pic = Guarded(ctx, img.nbytes, offset, img)
    ctx.draw_flow_enqueue(pic.ptr, fb.ptr, step, threshold, colour, batch=img.shape[0])
    ctx.sync()
    fb.free()
    return pic.take().reshape(img.shape)


@pytest.mark.parametrize("key", ("66x33", "131x67"))
def test_draw_flow_equals_the_restatement_on_the_fixture_fields(mav, fixture, key):
    from mavflow import _lib, vis  # noqa: F401
    flow = fixture[f"flow_{key}"]
    H, W = flow.shape[:2]
    rng = np.random.default_rng(50)
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    with _lib.Context(W, H, vc.B) as ctx:
        for step in (1, 8, 50):
            for thr in (0.0, 1.0):
                want = R.draw_flow(img, flow, step, thr, (0, 255, 0))
                assert (want != img).any()                         # (step 50 has one grid point, (25, 25))
                got = draw_dev(ctx, img[None], flow[None], step, thr, (0, 255, 0), offset=step % 2)
                assert np.array_equal(got[0], want), (step, thr, int((got[0] != want).any(axis=-1).sum()))
                mine = img.copy()
                assert ctx.draw_flow(mine, flow, step=step, threshold=thr) is mine and np.array_equal(mine, want)
        # a batch: each picture with its own field; another colour
        flows = np.stack([flow, flow[::-1].copy(), -flow])
        imgs = np.stack([img, img[::-1].copy(), np.zeros_like(img)])
        got = draw_dev(ctx, imgs, flows, 8, 1.0, (7, 8, 9))
        for b in range(3):
            assert np.array_equal(got[b], R.draw_flow(imgs[b], flows[b], 8, 1.0, (7, 8, 9))), b
        # all below the threshold, and a NaN threshold: unchanged
        assert np.array_equal(draw_dev(ctx, img[None], flow[None], 8, 1e9, (0, 255, 0))[0], img)
        assert np.array_equal(draw_dev(ctx, img[None], flow[None], 8, float("nan"), (0, 255, 0))[0], img)


def test_draw_flow_across_every_border_and_corner(mav):
    """Lines from the grid points of a 66 x 33 picture through each border and each corner, far beyond it (clipped), and to the last
    pixel inside.  (A line with both ends outside cannot be asked for: a line starts at a grid point; clip_line's rejection of such a
    segment is held on the CPU, tests/test_vis_ref_cpu.py.)"""
    from mavflow import _lib, vis  # noqa: F401
    from mavflow.farneback import Farneback
    W, H, step = 66, 33, 8
    targets = [(-40, 10), (W + 40, 12), (20, -30), (25, H + 30), (-50, -50), (W + 50, -50), (-50, H + 50), (W + 50, H + 50),
               (0, 0), (W - 1, H - 1), (W - 1, 0), (0, H - 1), (-1, -1), (W, H), (-3000, 7), (9, 4000), (1e7, -1e7), (-2e9, 3e9)]
    ys, xs = R.grid_points(W, H, step)
    flow = np.zeros((H, W, 2), np.float32)
    for (y, x), (tx, ty) in zip(zip(ys, xs), targets * 3):
        flow[y, x] = (tx - x, ty - y)
    img = np.full((H, W, 3), 30, np.uint8)
    want = R.draw_flow(img, flow, step, 1.0, (0, 255, 0))
    on = (want != img).any(axis=-1)
    assert on[0, 0] and on[0, W - 1] and on[H - 1, 0] and on[H - 1, W - 1] and on[:, 0].sum() > 3 and on[0].sum() > 3
    with _lib.Context(W, H, 1) as ctx:
        for off in vc.OFFSETS:
            assert np.array_equal(draw_dev(ctx, img[None], flow[None], step, 1.0, (0, 255, 0), off)[0], want)
        fb = Farneback.__new__(Farneback)
        fb.ctx = ctx
        mine = img.copy()
        assert fb.draw_flow(mine, flow) is mine and np.array_equal(mine, want)             # the class's method, step 8, green
        with pytest.raises(TypeError, match="float64"):
            fb.draw_flow(mine, flow.astype(np.float64))


# ---- refusals, and non-finite fields --------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_before_anything_is_enqueued(mav):
    from mavflow import _lib, vis
    lib = vis.load()
    W, H = 17, 5
    with _lib.Context(W, H, 2) as ctx:
        f = ctx.alloc(2 * W * H * 8).upload(np.zeros((2, H, W, 2), np.float32))
        pic = Guarded(ctx, 2 * W * H * 3, 0)
        rec = Guarded(ctx, 32, 0)
        col = np.array([0, 255, 0], np.uint8)
        cp = col.ctypes.data
        h = ctx.h
        calls = [
            lib.mav_flow_hsv_dev(h, None, 1, 0, pic.ptr, None, rec.ptr), lib.mav_flow_hsv_dev(h, f.ptr, 1, 0, None, None, rec.ptr),
            lib.mav_flow_hsv_dev(h, f.ptr, 1, 0, pic.ptr, None, None), lib.mav_flow_hsv_dev(h, f.ptr, 0, 0, pic.ptr, None, rec.ptr),
            lib.mav_flow_hsv_dev(h, f.ptr, 3, 0, pic.ptr, None, rec.ptr), lib.mav_flow_hsv_dev(h, f.ptr, 1, 2, pic.ptr, None, rec.ptr),
            lib.mav_flow_hsv_dev(h, f.ptr + 2, 1, 0, pic.ptr, None, rec.ptr), lib.mav_flow_hsv_dev(None, f.ptr, 1, 0, pic.ptr, None, rec.ptr),
            lib.mav_cvt_color_dev(h, None, 54, 1, pic.ptr), lib.mav_cvt_color_dev(h, pic.ptr, 54, 1, None), lib.mav_cvt_color_dev(h, pic.ptr, 4, 1, pic.ptr),
            lib.mav_cvt_color_dev(h, pic.ptr, 54, 3, pic.ptr),
            lib.mav_draw_flow_dev(h, None, f.ptr, 1, 8, 1.0, cp), lib.mav_draw_flow_dev(h, pic.ptr, None, 1, 8, 1.0, cp),
            lib.mav_draw_flow_dev(h, pic.ptr, f.ptr, 1, 0, 1.0, cp), lib.mav_draw_flow_dev(h, pic.ptr, f.ptr, 1, 8, 1.0, None),
            lib.mav_draw_flow_dev(h, pic.ptr, f.ptr, 0, 8, 1.0, cp),
        ]
        assert calls == [-1] * len(calls), calls                                   # MAV_ERR_ARG
        ctx.sync()
        f.free()
        assert (pic.take() == FILL).all() and (rec.take() == FILL).all()          # nothing was written


def test_non_finite_fields_return_and_leave_the_next_call_alone(mav):
    from mavflow import _lib, vis  # noqa: F401
    W, H = 131, 67
    clean = np.ascontiguousarray(vc.constructed_fields(W, H))
    want = host_process(clean)
    rng = np.random.default_rng(60)
    bad = clean.copy()
    pick = rng.random(bad.shape) < 0.05
    bad[pick] = rng.choice(np.array([np.nan, np.inf, -np.inf, 3e38, -3e38], np.float32), int(pick.sum()))
    img = np.zeros((vc.B, H, W, 3), np.uint8)
    with _lib.Context(W, H, vc.B) as ctx:
        for off in vc.OFFSETS:
            for mode in ("process", "draw"):
                gb, gh, gr = flow_hsv_dev(ctx, bad, mode, off, True)                # returns; the guards are untouched
                assert gb.shape == gh.shape
            for step, thr in ((1, 0.0), (8, 1.0)):
                draw_dev(ctx, img, bad, step, thr, (0, 255, 0), off)
            assert_equal_process(flow_hsv_dev(ctx, clean, "process", off, True), want, "after the non-finite fields")
