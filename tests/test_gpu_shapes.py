"""Shapes on the device (include/mavflow_shapes.h) against tests/shapes_ref.py, byte for byte, on every case of tests/shapes_cases.py:
the ordered form on a scratch plane full of 0xA5, the direct form where the table has one colour, the host form, the device's own
count, skipped records beside drawn ones, image 1 of the batch untouched, unaligned images; then cv2.add, the mosaic, blob boxes, and a
mav_last_* reader that returns the same bytes after every new call."""
import numpy as np
import pytest

import components_ref
import shapes_cases as sc
import shapes_ref as R

pytestmark = pytest.mark.gpu
GUARD = 64
FILL = sc.FILL
_expected = {}


def expected(case):
    """the restatement's picture of a case, computed once"""
    key = sc.case_id(case)
    if key not in _expected:
        img = sc.canary(case.W, case.H, case.channels)
        want = R.draw_shapes(img, case.shapes)
        want.setflags(write=False)
        _expected[key] = (img, want)
    return _expected[key]


class Guarded:
    """a device block of `nbytes` at `offset` bytes behind a 16-aligned address, between two guards"""

    def __init__(self, ctx, nbytes, offset=0, init=None):
        self.nbytes, self.offset = nbytes, offset
        raw = np.full(GUARD + offset + nbytes + GUARD, FILL, np.uint8)
        if init is not None:
            raw[GUARD + offset:GUARD + offset + nbytes] = np.ascontiguousarray(init).reshape(-1).view(np.uint8)
        self.buf = ctx.alloc(raw.nbytes).upload(raw)
        self.ptr = self.buf.ptr + GUARD + offset
        assert self.buf.ptr % 16 == 0

    def take(self):
        raw = self.buf.download(np.uint8, (self.buf.nbytes,))
        self.buf.free()
        a = GUARD + self.offset
        assert (raw[:a] == FILL).all() and (raw[a + self.nbytes:] == FILL).all(), "bytes outside the block were written"
        return raw[a:a + self.nbytes]


def draw_dev(ctx, img, shapes, channels, offset=0, ordered=True, n_dev=None):
    """mav_draw_shapes_dev on caller-owned blocks -> the picture"""
    from mavflow import shapes as S
    Bn, H, W = img.shape[:3]
    pic = Guarded(ctx, img.nbytes, offset, img)
    tab = Guarded(ctx, max(shapes.nbytes, 32), 0, shapes if len(shapes) else None)
    plane = Guarded(ctx, S.scratch_bytes(W, H, Bn), 0) if ordered else None               # full of 0xA5: the call clears it itself
    cnt = Guarded(ctx, 4, 0, np.array([n_dev], np.int32)) if n_dev is not None else None
    ctx.draw_shapes_enqueue(pic.ptr, tab.ptr, len(shapes), channels, Bn, n_ptr=None if cnt is None else cnt.ptr,
                            scratch_ptr=None if plane is None else plane.ptr)
    ctx.sync()
    assert tab.take()[:shapes.nbytes].tobytes() == shapes.tobytes()                        # the table is read, never written
    if plane is not None:
        plane.take()
    if cnt is not None:
        assert cnt.take().view(np.int32)[0] == n_dev
    return pic.take().reshape(img.shape)


def differing(a, b):
    return int((a != b).any(axis=-1).sum())


@pytest.mark.parametrize("k", range(len(sc.CASES)), ids=[sc.case_id(c) for c in sc.CASES])
def test_device_equals_the_restatement(mav, k):
    from mavflow import _lib, shapes as S
    case = sc.CASES[k]
    img, want = expected(case)
    assert (want[1] == img[1]).all() and (want[0] != img[0]).any()                          # image 1 is no record's; image 0 is drawn into
    with _lib.Context(case.W, case.H, sc.B) as ctx:
        got = draw_dev(ctx, img, case.shapes, case.channels, offset=k % 2 * (1 + k % 5), ordered=True)
        assert np.array_equal(got[1], img[1]), "image 1 of the batch was written"
        assert np.array_equal(got, want), (sc.case_id(case), "ordered", differing(got, want))
        if sc.one_colour(case.shapes, case.channels):
            got = draw_dev(ctx, img, case.shapes, case.channels, offset=3, ordered=False)
            assert np.array_equal(got, want), (sc.case_id(case), "direct", differing(got, want))
        host = img.copy()
        if case.name == "skipped":
            with pytest.raises(ValueError, match="record 2 "):
                ctx.draw_shapes(host, case.shapes)
            assert np.array_equal(host, img)                                               # a refused call has written nothing
        else:
            assert ctx.draw_shapes(host, case.shapes) is host
            assert S.shapes_form(case.shapes, case.channels) == (S.FORM_DIRECT if sc.one_colour(case.shapes, case.channels) else S.FORM_ORDERED)
            assert np.array_equal(host, want), (sc.case_id(case), "host form", differing(host, want))


def heavy():
    return [c for c in sc.CASES if c.name == "heavy-overlap"][0]


def test_the_reversed_table_gives_the_reversed_order(mav):
    from mavflow import _lib
    case = heavy()
    img, want = expected(case)
    rev = np.ascontiguousarray(case.shapes[::-1])
    want_rev = R.draw_shapes(img, rev)
    assert differing(want, want_rev) >= 2000
    with _lib.Context(case.W, case.H, sc.B) as ctx:
        got = draw_dev(ctx, img, rev, 3)
        assert np.array_equal(got, want_rev), differing(got, want_rev)
        again = draw_dev(ctx, img, rev, 3, offset=5)
        assert np.array_equal(again, got)                                                  # the same bytes on every run


@pytest.mark.parametrize("n_dev", [700, 2, 0, -1, -(1 << 31), 2301, (1 << 31) - 1])
def test_the_devices_own_count(mav, n_dev):
    from mavflow import _lib
    case = heavy()
    img, _ = expected(case)
    assert len(case.shapes) == 2300
    want = R.draw_shapes(img, case.shapes, n_dev)
    assert (want != img).any() == (0 < n_dev <= 2300)
    with _lib.Context(case.W, case.H, sc.B) as ctx:
        for ordered in (True, False):                                                       # (the direct form: only that nothing is drawn)
            if ordered or not 0 < n_dev <= 2300:
                got = draw_dev(ctx, img, case.shapes, 3, ordered=ordered, n_dev=n_dev)
                assert np.array_equal(got, want), (n_dev, ordered, differing(got, want))


def test_direct_equals_ordered_on_a_one_colour_table(mav):
    from mavflow import _lib
    for case in [c for c in sc.CASES if c.name == "one-colour"]:
        img, want = expected(case)
        with _lib.Context(case.W, case.H, sc.B) as ctx:
            a = draw_dev(ctx, img, case.shapes, case.channels, ordered=True)
            b = draw_dev(ctx, img, case.shapes, case.channels, ordered=False)
            assert np.array_equal(a, b) and np.array_equal(a, want)


@pytest.mark.parametrize("case", sc.ADD_CASES, ids=lambda c: c.name)
def test_add_saturate(mav, case):
    from mavflow import _lib, shapes as S
    a, b = sc.add_inputs(case)
    want = np.minimum(a.astype(np.int32) + b, 255).astype(np.uint8)
    with _lib.Context(case.W, case.H, sc.B) as ctx:
        da, db, dd = Guarded(ctx, a.nbytes, case.offset, a), Guarded(ctx, b.nbytes, case.offset, b), Guarded(ctx, a.nbytes, case.offset)
        assert S.bytes_form(a.nbytes, da.ptr, db.ptr, dd.ptr) == sc.bytes_form_of(a.nbytes, case.offset)
        ctx.add_saturate_enqueue(da.ptr, db.ptr, dd.ptr, case.channels, case.batch)
        ctx.add_saturate_enqueue(da.ptr, db.ptr, da.ptr, case.channels, case.batch)       # in place, as cv2.add(frame, mask, frame)
        ctx.sync()
        assert np.array_equal(dd.take().reshape(a.shape), want)
        assert np.array_equal(da.take().reshape(a.shape), want) and np.array_equal(db.take().reshape(a.shape), b)
        assert np.array_equal(ctx.add_saturate(a, b), want)
        if case.batch == 1 and case.channels in (1, 3):
            assert np.array_equal(S.add(a[0], b[0]), want[0])


@pytest.mark.parametrize("case", sc.MOSAIC_CASES, ids=lambda c: c.name)
def test_mosaic(mav, case):
    from mavflow import _lib, shapes as S
    tiles = sc.mosaic_inputs(case)
    rgb = [np.zeros((case.batch, case.H, case.W, 3), np.uint8) if t is None else np.repeat(t, 3, 3) if t.shape[3] == 1 else t for t in tiles]
    want = np.stack([np.vstack([np.hstack([rgb[r * case.cols + c][b] for c in range(case.cols)]) for r in range(case.rows)])
                     for b in range(case.batch)])
    with _lib.Context(case.W, case.H, sc.B) as ctx:
        dev = [None if t is None else Guarded(ctx, t.nbytes, (i * 3) % 7, t) for i, t in enumerate(tiles)]
        out = Guarded(ctx, want.nbytes, case.offset)
        assert S.bytes_form(want.nbytes, out.ptr) == sc.bytes_form_of(want.nbytes, case.offset)
        ctx.mosaic_enqueue([None if d is None else d.ptr for d in dev], [max(c, 1) for c in case.channels], case.rows, case.cols, out.ptr, case.batch)
        ctx.sync()
        assert np.array_equal(out.take().reshape(want.shape), want)
        for d, t in zip(dev, tiles):
            if d is not None:
                assert d.take().tobytes() == t.tobytes()
        assert np.array_equal(ctx.mosaic(tiles, case.rows, case.cols), want)


def blob_masks(W, H):
    rng = np.random.RandomState(21)
    m = np.zeros((sc.B, H, W), np.uint8)
    for b in (0, 2):
        for _ in range(9):
            x, y, w, h = rng.randint(0, W - 8), rng.randint(0, H - 6), rng.randint(1, 14), rng.randint(1, 9)
            m[b, y:y + h, x:x + w] = 255
    m[2, 0, 0] = m[2, H - 1, W - 1] = 1                                                    # one-pixel blobs in two corners
    return m


@pytest.mark.parametrize("W,H", sc.FRAMES)
@pytest.mark.parametrize("max_blobs,thickness", [(256, 2), (3, 1), (16, R.FILLED)])
def test_blob_boxes_equal_the_restatement_on_the_reference_table(mav, W, H, max_blobs, thickness):
    from mavflow import _lib
    masks = blob_masks(W, H)
    _, counts, tables = components_ref.components_batch(masks, 8, 1, max_blobs)
    assert counts["n_blobs"][1] == 0 and counts["n_blobs"][0] > 3 and (max_blobs != 3 or counts["n_blobs"][0] > max_blobs)
    boxes = [[(int(r["x"]), int(r["y"]), int(r["w"]), int(r["h"])) for r in tables[b]] for b in range(sc.B)]
    shapes = R.shapes_from_blobs(boxes, counts["n_blobs"], max_blobs, thickness, sc.RED)
    img = sc.canary(W, H, 3)
    want = R.draw_shapes(img, shapes)
    with _lib.Context(W, H, sc.B) as ctx:
        got = ctx.draw_blob_boxes(img.copy(), mask=masks, thickness=thickness, color=sc.RED, max_blobs=max_blobs)
        assert np.array_equal(got, want), differing(got, want)
        assert np.array_equal(got[1], img[1])
        cc = ctx.components(masks, max_blobs=max_blobs)
        got = ctx.draw_blob_boxes(img.copy(), cc, thickness=thickness, color=sc.RED)
        assert np.array_equal(got, want), differing(got, want)


def test_bad_arguments_are_refused_before_anything_is_enqueued(mav):
    from mavflow import _lib, shapes as S
    W, H = sc.FRAMES[1]
    img = sc.canary(W, H, 3)
    tab = R.table(sc.octant_lines(W, H, 2))
    with _lib.Context(W, H, sc.B) as ctx:
        pic, dt = Guarded(ctx, img.nbytes, 0, img), Guarded(ctx, tab.nbytes, 0, tab)
        for kw in (dict(channels=2), dict(channels=4), dict(batch=0), dict(batch=sc.B + 1), dict(n_max=-1)):
            args = dict(n_max=len(tab), channels=3, batch=sc.B)
            args.update(kw)
            with pytest.raises(ValueError, match="mav_draw_shapes_dev"):
                ctx.draw_shapes_enqueue(pic.ptr, dt.ptr, **args)
        with pytest.raises(ValueError, match="aligned"):
            ctx.draw_shapes_enqueue(pic.ptr, dt.ptr + 2, len(tab) - 1, 3, sc.B)
        with pytest.raises(ValueError, match="aligned"):
            ctx.draw_shapes_enqueue(pic.ptr, dt.ptr, len(tab), 3, sc.B, scratch_ptr=pic.ptr + 2)
        with pytest.raises(ValueError, match="mav_add_saturate_dev"):
            ctx.add_saturate_enqueue(pic.ptr, pic.ptr, pic.ptr, 5, sc.B)
        with pytest.raises(ValueError, match="mav_mosaic_dev"):
            ctx.mosaic_enqueue([pic.ptr], [2], 1, 1, pic.ptr, 1)
        with pytest.raises(ValueError, match="tiles"):
            ctx.mosaic_enqueue([pic.ptr] * 17, [3] * 17, 1, 17, pic.ptr, 1)
        ctx.draw_shapes_enqueue(pic.ptr, dt.ptr, 0, 3, sc.B)                               # no record: nothing drawn, no error
        ctx.sync()
        assert np.array_equal(pic.take().reshape(img.shape), img)
        dt.take()
        with pytest.raises(ValueError, match="record 1 "):
            ctx.draw_shapes(img.copy(), [S.shape(S.LINE, 1, 1, 5, 5, 2, sc.RED), S.shape(S.LINE, 1, 1, 5, 5, 300, sc.RED)])
        with pytest.raises(TypeError):
            ctx.draw_shapes(img.astype(np.float32), tab)


def test_a_resident_reader_returns_the_same_bytes_after_every_new_call(mav):
    """mav_last_masks_tpr_fpr reads the masks a phi_mask call left on the device: each new entry point keeps them"""
    from mavflow import _lib
    W, H = sc.FRAMES[0]
    rng = np.random.RandomState(4)
    flow = rng.randn(sc.B, H, W, 2).astype(np.float32) * 3
    gt = (rng.rand(sc.B, H, W) > 0.7).astype(np.uint8) * 255
    img = sc.canary(W, H, 3)
    case = heavy()
    masks = blob_masks(W, H)
    with _lib.Context(W, H, sc.B) as ctx:
        ctx.phi_mask(flow, np.tile([W / 2, H / 2], (sc.B, 1)))
        before = [c.tobytes() for c in ctx.last_masks_tpr_fpr(gt)]
        calls = [lambda: ctx.draw_shapes(img.copy(), case.shapes), lambda: draw_dev(ctx, img, case.shapes, 3),
                 lambda: draw_dev(ctx, img, case.shapes[:50], 3, ordered=False), lambda: ctx.add_saturate(img, img),
                 lambda: ctx.mosaic([img, gt[..., None], None, img], 2, 2), lambda: ctx.draw_blob_boxes(img.copy(), mask=masks)]
        for i, call in enumerate(calls):
            call()
            assert [c.tobytes() for c in ctx.last_masks_tpr_fpr(gt)] == before, f"call {i} disturbed the resident masks"


def test_motion_pictures_equal_the_host_output_renders_and_keep_the_resident_masks(mav):
    """mav_motion_pictures_dev against mav_flow_to_color and mav_last_global_motion_render (the same pictures with host outputs), its
    refusals, and the resident masks of an earlier phi_mask call after it"""
    from mavflow import _lib, shapes  # noqa: F401
    W, H = sc.FRAMES[0]
    Bn, n = 2, W * H
    rng = np.random.RandomState(12)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    flow = np.stack([np.stack([0.02 * xx + 1.5, -0.01 * yy + 0.5], -1)] * Bn) + rng.randn(Bn, H, W, 2).astype(np.float32) * 0.05
    flow = np.ascontiguousarray(flow, np.float32)
    coords = np.stack([rng.randint(5, W - 5, 40), rng.randint(5, H - 5, 40)], 1)
    gt = (rng.rand(Bn, H, W) > 0.7).astype(np.uint8) * 255
    with _lib.Context(W, H, sc.B) as ctx:
        dflow = Guarded(ctx, flow.nbytes, 0, flow)
        field = Guarded(ctx, 8 * n * Bn, 0)
        pics = [Guarded(ctx, 3 * n * Bn, 16 * k) for k in range(3)]
        res = Guarded(ctx, _lib.MOTION_DTYPE.itemsize * Bn, 0)
        with pytest.raises(_lib.MavflowError, match="mav_motion_pictures_dev: no flow"):        # MAV_ERR_STATE: nothing is resident yet
            ctx.motion_pictures_enqueue(Bn, dflow.ptr, field.ptr, None, pics[1].ptr, None)
        ctx.phi_mask(flow, np.tile([W / 2, H / 2], (Bn, 1)))
        before = [c.tobytes() for c in ctx.last_masks_tpr_fpr(gt)]
        ctx.global_motion_step(dflow.ptr, coords, Bn, res.ptr)
        for kw, what in ((dict(field_ptr=None, img_flow_ptr=pics[0].ptr, flow_ptr=dflow.ptr), "NULL field"),
                         (dict(field_ptr=field.ptr, img_flow_ptr=pics[0].ptr), "img_flow without flow"),
                         (dict(field_ptr=field.ptr + 2, img_warped_ptr=pics[1].ptr), "aligned"),
                         (dict(field_ptr=field.ptr, flow_ptr=dflow.ptr + 1, img_flow_ptr=pics[0].ptr), "aligned")):
            with pytest.raises(ValueError, match=what):
                ctx.motion_pictures_enqueue(Bn, **kw)
        with pytest.raises(ValueError, match="batch"):
            ctx.motion_pictures_enqueue(sc.B + 1, dflow.ptr, field.ptr, pics[0].ptr)
        with pytest.raises(_lib.MavflowError, match="no flow of a 1-item"):
            ctx.motion_pictures_enqueue(1, dflow.ptr, field.ptr, None, pics[1].ptr)
        ctx.motion_pictures_enqueue(Bn, dflow.ptr, field.ptr, pics[0].ptr, pics[1].ptr, pics[2].ptr)
        ctx.sync()
        got = [p.take().reshape(Bn, H, W, 3) for p in pics]
        assert [c.tobytes() for c in ctx.last_masks_tpr_fpr(gt)] == before, "the call disturbed the resident masks"
        want = ctx.render_last_global_motion(Bn)
        assert np.array_equal(got[1], want["warped"]) and np.array_equal(got[2], want["global"])
        assert dflow.take().tobytes() == flow.tobytes()
        field.take()
        res.take()
        assert np.array_equal(got[0], ctx.flow_to_color(flow))


# ---- past the caps of the launches (tests/shapes_cases.py RESOLVE_FRAME, ROWS_RECORDS) ---------------------------------------------------------
@pytest.mark.parametrize("channels", (3, 1))
def test_resolve_past_its_cap_equals_the_restatement(mav, channels):
    """701 x 499 x 3: k_shapes_resolve's second trip reads the owner plane past 2^20 elements, the last rows of image 2, where records of
    different colours overlap and order decides"""
    from mavflow import _lib
    W, H = sc.RESOLVE_FRAME
    shapes = sc.resolve_cap_table(W, H)
    img = sc.canary(W, H, channels)
    want = R.draw_shapes(img, shapes)
    assert not sc.one_colour(shapes, channels)
    with _lib.Context(W, H, sc.B) as ctx:
        got = draw_dev(ctx, img, shapes, channels, offset=3 if channels == 3 else 0, ordered=True)
        assert np.array_equal(got, want), ("ordered", channels, differing(got, want), np.argwhere((got != want).any(axis=-1))[:4].tolist())
        host = img.copy()
        assert ctx.draw_shapes(host, shapes) is host
        assert np.array_equal(host, want), ("host form", channels, differing(host, want))


@pytest.fixture(scope="module")
def rows_cap():
    """the 8 300 records and the restatement's pictures of them, computed once: (canary, table, ordered, green table, direct, ordered up to n_dev)"""
    W, H = sc.FRAMES[0]
    img = sc.canary(W, H, 3)
    t, g = sc.rows_cap_table(W, H), sc.rows_cap_table(W, H, green=True)
    out = (img, t, R.draw_shapes(img, t), g, R.draw_shapes(img, g), R.draw_shapes(img, t, sc.ROWS_N_DEV))
    for a in out:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("form", ("ordered", "direct", "n_dev"))
def test_rows_past_their_cap_equal_the_restatement(mav, rows_cap, form):
    """8 300 records: k_shapes_rows reaches records 8192 .. on its workgroups' second trip -- in ORDERED form the records that must win
    every overlap"""
    from mavflow import _lib
    W, H = sc.FRAMES[0]
    img, t, want, g, want_g, want_n = rows_cap
    assert len(t) == sc.ROWS_RECORDS and ">1:partial-last" in sc.rows_forms(len(t))
    with _lib.Context(W, H, sc.B) as ctx:
        if form == "ordered":
            got = draw_dev(ctx, img, t, 3, offset=5, ordered=True)
            assert np.array_equal(got, want), (form, differing(got, want))
            assert (want != want_n).any()                                                  # the records past n_dev decide pixels
        elif form == "direct":
            assert sc.one_colour(g, 3)
            for ordered in (False, True):
                got = draw_dev(ctx, img, g, 3, ordered=ordered)
                assert np.array_equal(got, want_g), (form, ordered, differing(got, want_g))
        else:
            got = draw_dev(ctx, img, t, 3, ordered=True, n_dev=sc.ROWS_N_DEV)
            assert np.array_equal(got, want_n), (form, differing(got, want_n))
