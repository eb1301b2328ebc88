"""The image resize on the GPU (csrc/kernels_resize.hip and the calls around it) against the numpy restatement tests/resize_ref.py at every
run of tests/resize_cases.py: every pixel format and interpolation at every shape, in the host and the _dev forms, at batch 1 and 3, the
_dev forms on plain pointers and on pointers offset by one element into canary-filled blocks whose heads and tails stay untouched.  Equal
bytes everywhere (NaNs are compared by position and payload): no tolerance appears in this file.  The fused sky mask equals the two-step
route and the restatement; two contexts of different frames give the same bytes."""
import ctypes as C

import numpy as np
import pytest

import resize_cases as T
import resize_ref as R

pytestmark = pytest.mark.gpu
CANARY, TAIL = 0xA5, 64
_refs = {}
ids = lambda s: f"{s.src[0]}x{s.src[1]}-{s.dst[0]}x{s.dst[1]}"
vp = lambda p: C.c_void_p(int(p))


def _ref(fmt, shape, interp):
    """(src (B, ...), want (B, ...)) of one (format, shape, interpolation), computed once and shared, read-only"""
    key = (fmt, shape.src, shape.dst, interp)
    if key not in _refs:
        src = T.images(fmt, *shape.src)
        want = np.stack([R.resize(src[b], shape.dst[0], shape.dst[1], interp) for b in range(T.B)])
        src.setflags(write=False)
        want.setflags(write=False)
        _refs[key] = (src, want)
    return _refs[key]


def _sky_ref(shape):
    key = ("sky", shape.src, shape.dst)
    if key not in _refs:
        pred = T.prediction(*shape.src)
        want = np.stack([R.sky_mask(pred[b], shape.dst[0], shape.dst[1], T.SKY) for b in range(T.B)])
        pred.setflags(write=False)
        want.setflags(write=False)
        _refs[key] = (pred, want)
    return _refs[key]


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    a, b = (R.bits(got), R.bits(want)) if got.dtype == np.float32 else (got, want)            # bits: a NaN by position and payload
    bad = np.argwhere(a != b)
    assert len(bad) == 0, (what, len(bad), bad[:4].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


class _Dev:
    """caller-owned blocks of one context: an array uploaded `shift` bytes into a canary-filled block with a tail behind it"""

    def __init__(self, ctx):
        self.ctx, self.bufs = ctx, []

    def put(self, a, shift):
        a = np.ascontiguousarray(a)
        raw = np.full(shift + a.nbytes + TAIL, CANARY, np.uint8)
        raw[shift:shift + a.nbytes] = a.view(np.uint8).ravel()
        b = self.ctx.alloc(raw.nbytes).upload(raw)
        self.bufs.append(b)
        return b, b.ptr + shift

    def blank(self, nbytes, shift):
        return self.put(np.full(nbytes, CANARY, np.uint8), shift)

    def get(self, b, shift, dtype, shape):
        raw = b.download(np.uint8, (b.nbytes,))
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        assert (raw[:shift] == CANARY).all() and (raw[shift + n:] == CANARY).all(), "the block's head or tail was written"
        return raw[shift:shift + n].view(dtype).reshape(shape).copy()

    def close(self):
        for b in self.bufs:
            b.free()
        self.bufs = []


@pytest.fixture(scope="module")
def contexts(mav):
    from mavflow import _lib
    made = {}

    def get(W, H):
        if (W, H) not in made:
            made[(W, H)] = _lib.Context(W, H, T.B)
        return made[(W, H)]
    yield get
    for c in made.values():
        c.close()


@pytest.mark.parametrize("shape", T.SHAPES, ids=ids)
def test_device_bytes_equal_the_restatement(contexts, shape):
    from mavflow import resize
    from mavflow._lib import _ptr
    lib = resize.load()
    ctx = contexts(37, 23)                                   # the context's frame has nothing to do with the sizes of a resize
    (sw, sh), (dw, dh) = shape.src, shape.dst
    dev = _Dev(ctx)
    try:
        for run in T.runs(shape):
            fmt, interp, n = T.FORMATS[run.fmt], T.INTERPS[run.interp], run.batch
            src, want = _ref(fmt, shape, interp)
            src, want = np.ascontiguousarray(src[:n]), want[:n]
            if not run.shifted:                              # the host form, once per (format, interpolation, batch)
                dst = np.full_like(want, CANARY) if want.dtype == np.uint8 else np.full(want.shape, np.float32(-777.25))
                assert lib.mav_resize(ctx.h, _ptr(src), fmt, sw, sh, dw, dh, interp, n, _ptr(dst)) == 0, (run, lib.mav_last_error())
                _same(dst, want, ("host",) + tuple(run))
            e = src.dtype.itemsize if run.shifted else 0
            _, ds = dev.put(src, e)
            db, dd = dev.blank(want.nbytes, e)
            assert lib.mav_resize_dev(ctx.h, vp(ds), fmt, sw, sh, dw, dh, interp, n, vp(dd)) == 0, (run, lib.mav_last_error())
            ctx.sync()
            _same(dev.get(db, e, want.dtype, want.shape), want, ("dev",) + tuple(run))
            dev.close()
    finally:
        dev.close()


@pytest.mark.parametrize("shape", T.SHAPES, ids=ids)
def test_sky_mask_equals_the_two_step_route_and_the_restatement(contexts, shape):
    from mavflow import resize
    from mavflow._lib import _ptr
    lib = resize.load()
    ctx = contexts(37, 23)
    (sw, sh), (dw, dh) = shape.src, shape.dst
    pred, want = _sky_ref(shape)
    if min(sw, sh) >= 8:
        assert want.any() and not want.all()
    dev = _Dev(ctx)
    try:
        for run in T.sky_runs():
            if run.shape is not shape:
                continue
            n = run.batch
            p, w = np.ascontiguousarray(pred[:n]), want[:n]
            e = 1 if run.shifted else 0
            if not run.shifted:
                sky = np.full_like(w, CANARY)
                assert lib.mav_sky_mask(ctx.h, _ptr(p), sw, sh, dw, dh, T.SKY[0], T.SKY[1], n, _ptr(sky)) == 0, (run, lib.mav_last_error())
                _same(sky, w, ("host",) + tuple(run))
                # the two-step route, on the host: the library's own resized picture, keyed
                pic = np.empty((n, dh, dw, 3), np.uint8)
                assert lib.mav_resize(ctx.h, _ptr(p), R.U8C3, sw, sh, dw, dh, R.LINEAR, n, _ptr(pic)) == 0
                _same(((pic[..., 0] == T.SKY[0]) & (pic[..., 1] == T.SKY[1])).astype(np.uint8), sky, ("two-step",) + tuple(run))
            _, dp = dev.put(p, e)
            db, dd = dev.blank(w.nbytes, e)
            assert lib.mav_sky_mask_dev(ctx.h, vp(dp), sw, sh, dw, dh, T.SKY[0], T.SKY[1], n, vp(dd)) == 0, (run, lib.mav_last_error())
            ctx.sync()
            _same(dev.get(db, e, np.uint8, w.shape), w, ("dev",) + tuple(run))
            dev.close()
        # another key: the third stripe's colour
        k0, k1 = T.STRIPES[2][:2]
        sky = np.empty_like(want)
        assert lib.mav_sky_mask(ctx.h, _ptr(np.ascontiguousarray(pred)), sw, sh, dw, dh, k0, k1, T.B, _ptr(sky)) == 0
        _same(sky, np.stack([R.sky_mask(pred[b], dw, dh, (k0, k1)) for b in range(T.B)]), ("other key", ids(shape)))
    finally:
        dev.close()


def test_two_contexts_of_different_frames_give_the_same_bytes(contexts):
    a, b = contexts(37, 23), contexts(131, 67)
    shape = T.SHAPES[6]
    assert shape.dst == (65, 70)
    outs = []
    for ctx in (a, b, a):
        parts = []
        for f, fmt in T.FORMATS.items():
            src, want = _ref(fmt, shape, R.LINEAR)
            got = ctx.resize(src, shape.dst, interpolation=R.LINEAR, batched=True)
            _same(got, want, (f, "batched"))
            one = ctx.resize(src[1], shape.dst)
            assert one.tobytes() == got[1].tobytes()                      # batch 1 and batch 3, every batch position its own image
            parts.append(got.tobytes())
        pred, want = _sky_ref(shape)
        m = ctx.sky_mask(pred, shape.dst)
        assert m.dtype == np.bool_ and np.array_equal(m.view(np.uint8), want)
        parts.append(m.tobytes())
        outs.append(b"".join(parts))
    assert outs[0] == outs[1] == outs[2]


def test_refusals_that_need_the_context(contexts):
    """what the arguments alone decide is tests/test_abi_resize.py's; here: a batch above the context's, in every entry point, and the
    arguments' refusals on a live context, outputs untouched"""
    from mavflow import _lib, resize
    from mavflow._lib import _ptr
    lib = resize.load()
    ctx = contexts(37, 23)
    n = T.B + 1
    src, dst = np.zeros((n, 6, 8, 3), np.uint8), np.full((n, 12, 16, 3), CANARY, np.uint8)
    blk = ctx.alloc(dst.nbytes + src.nbytes + 256).upload(np.full(dst.nbytes + src.nbytes + 256, CANARY, np.uint8))
    try:
        d_src, d_dst = vp(blk.ptr), vp(blk.ptr + src.nbytes + 128)
        for name, args, dargs in (("mav_resize", (_ptr(src), R.U8C3, 8, 6, 16, 12, R.LINEAR, n, _ptr(dst)), (d_src, R.U8C3, 8, 6, 16, 12, R.LINEAR, n, d_dst)),
                                  ("mav_sky_mask", (_ptr(src), 8, 6, 16, 12, 180, 130, n, _ptr(dst)), (d_src, 8, 6, 16, 12, 180, 130, n, d_dst))):
            assert getattr(lib, name)(ctx.h, *args) == _lib.MAV_ERR_ARG, name
            assert b"batch" in lib.mav_last_error() and name.encode() + b":" in lib.mav_last_error()
            assert getattr(lib, name + "_dev")(ctx.h, *dargs) == _lib.MAV_ERR_ARG, name
            assert b"batch" in lib.mav_last_error() and name.encode() + b"_dev:" in lib.mav_last_error()
        ok = T.B
        for name, args in {"mav_resize": (_ptr(src), R.U8C3, 8, 6, 16, 12, 2, ok, _ptr(dst)),
                           "mav_resize_dev": (d_src, R.U8C3, 8, 6, 16, 12, R.AREA, ok, d_dst),
                           "mav_sky_mask": (_ptr(src), 8, 6, 16, 12, 256, 130, ok, _ptr(dst)),
                           "mav_sky_mask_dev": (d_src, 8, 6, 16, 0, 180, 130, ok, d_dst)}.items():
            assert getattr(lib, name)(ctx.h, *args) == _lib.MAV_ERR_ARG, name
            assert name.encode() + b":" in lib.mav_last_error()
        assert lib.mav_resize_dev(ctx.h, d_src, R.U8C3, 8, 6, 16, 12, R.LINEAR, 1, vp(blk.ptr + 100)) == _lib.MAV_ERR_ARG     # overlap
        ctx.sync()
        assert (dst == CANARY).all() and (blk.download(np.uint8, (blk.nbytes,)) == CANARY).all()
    finally:
        blk.free()
