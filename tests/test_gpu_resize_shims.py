"""mavflow.resize's Python layer on the GPU: `resize` with cv2's signature (dsize, fx / fy, dst=), the reference-named pieces
(im_helpers.resize_percent, resize.sky_segmentation, resize.gt_of_resized), the Context methods on host arrays and on device handles, and
the point of it all: ctx.detect fed a sky mask and a field that were resized on the device returns the bytes it returns for the
restatement's host arrays.  The expected values are tests/resize_ref.py's, byte for byte."""
import ctypes as C

import numpy as np
import pytest

import resize_cases as T
import resize_ref as R

pytestmark = pytest.mark.gpu


def test_resize_with_cv2s_signature(mav):
    from mavflow import resize as K
    u8 = T.images(R.U8C3, 33, 17)[1]
    f2 = T.images(R.F32C2, 33, 17)[0]
    g1 = T.images(R.U8C1, 64, 48)[1]
    assert np.array_equal(K.resize(u8, (65, 70)), R.resize(u8, 65, 70, R.LINEAR))                     # INTER_LINEAR by default
    assert R.bits(K.resize(f2, (65, 70))).tobytes() == R.bits(R.resize(f2, 65, 70, R.LINEAR)).tobytes()
    assert np.array_equal(K.resize(g1, (37, 29), interpolation=K.INTER_AREA), R.resize(g1, 37, 29, R.AREA))
    assert np.array_equal(K.resize(g1, (37, 29), interpolation=K.INTER_NEAREST), R.resize(g1, 37, 29, R.NEAREST))
    # (H, W, 1) keeps its axis
    one = K.resize(g1[..., None], (32, 24))
    assert one.shape == (24, 32, 1) and np.array_equal(one[..., 0], R.resize(g1, 32, 24, R.LINEAR))
    # fx / fy with dsize None and (0, 0): round half to even -- 33 * 0.5 = 16.5 -> 16, 17 * 0.5 = 8.5 -> 8
    for dsize in (None, (0, 0)):
        out = K.resize(u8, dsize, fx=0.5, fy=0.5, interpolation=K.INTER_AREA)
        assert out.shape == (8, 16, 3) and np.array_equal(out, R.resize(u8, 16, 8, R.AREA))
    # dst=
    dst = np.zeros((70, 65, 3), np.uint8)
    assert K.resize(u8, (65, 70), dst) is dst and np.array_equal(dst, R.resize(u8, 65, 70, R.LINEAR))
    # a batch through the keyword
    batch = T.images(R.U8C3, 33, 17)
    out = K.resize(batch, (65, 70), batched=True)
    assert out.shape == (T.B, 70, 65, 3) and all(np.array_equal(out[b], R.resize(batch[b], 65, 70, R.LINEAR)) for b in range(T.B))
    # what is not built, on a machine where the built things run
    with pytest.raises(NotImplementedError):
        K.resize(u8, (65, 70), interpolation=K.INTER_CUBIC)
    with pytest.raises(NotImplementedError):
        K.resize(u8, (65, 70), interpolation=K.INTER_AREA)
    with pytest.raises(NotImplementedError):
        K.resize(np.zeros((5, 7, 4), np.uint8), (3, 3))
    with pytest.raises(NotImplementedError):
        K.resize(np.zeros((5, 7), np.uint16), (3, 3))
    with pytest.raises(TypeError):
        K.resize(np.zeros((5, 7), np.float64), (3, 3))


def test_the_reference_named_pieces(mav):
    from mavflow import im_helpers, resize as K
    img = T.images(R.U8C3, 63, 48)[1]
    half = im_helpers.resize_percent(img, 50)                              # int(63 * 50 / 100) = 31, 24
    assert half.shape == (24, 31, 3) and np.array_equal(half, R.resize(img, 31, 24, R.AREA))
    even = T.images(R.U8C3, 64, 48)[1]
    assert np.array_equal(im_helpers.resize_percent(even, 50), R.resize(even, 32, 24, R.AREA))         # the 2 x 2 form
    pred = T.prediction(60, 32)[0]
    sky = K.sky_segmentation(pred, size=(120, 64))
    assert sky.dtype == np.bool_ and sky.shape == (64, 120) and np.array_equal(sky, R.sky_mask(pred, 120, 64).astype(bool)) and sky.any() and not sky.all()
    full = K.sky_segmentation(T.prediction(96, 52)[0])                     # the reference's size by default
    assert full.shape == (1024, 1920)
    flow = T.images(R.F32C2, 33, 17, special=False)[1]
    assert K.gt_of_resized(flow, (33, 17)) is flow
    up = K.gt_of_resized(flow, (65, 70))
    assert up.tobytes() == R.resize(flow, 65, 70, R.LINEAR).tobytes()      # the vectors are not rescaled, as in the reference


def test_context_methods_on_host_arrays_and_device_handles(mav):
    from mavflow import _lib, resize as K
    W, H = 64, 48
    pred = T.prediction(32, 24)
    field = T.images(R.F32C2, 32, 24, special=False)
    with _lib.Context(W, H, T.B) as ctx:
        m = ctx.sky_mask(pred[0])                                           # dsize: the context's (W, H)
        assert m.shape == (H, W) and m.dtype == np.bool_ and np.array_equal(m, R.sky_mask(pred[0], W, H).astype(bool))
        mb = ctx.sky_mask(pred, key=T.STRIPES[2][:2])
        assert mb.shape == (T.B, H, W) and all(np.array_equal(mb[b].view(np.uint8), R.sky_mask(pred[b], W, H, T.STRIPES[2][:2])) for b in range(T.B))
        want = np.stack([R.resize(field[b], W, H, R.LINEAR) for b in range(T.B)])
        assert ctx.resize(field, (W, H), batched=True).tobytes() == want.tobytes()
        # device handles: the result stays on the device
        dp, df = ctx.alloc(pred.nbytes).upload(pred), ctx.alloc(field.nbytes).upload(field)
        bufs = [dp, df]
        try:
            sky = ctx.sky_mask(dp, ssize=(32, 24), batch=T.B)
            out = ctx.resize(df, (W, H), format=R.F32C2, ssize=(32, 24), batch=T.B)
            bufs += [sky, out]
            assert np.array_equal(sky.download(np.uint8, (T.B, H, W)), np.stack([R.sky_mask(pred[b], W, H) for b in range(T.B)]))
            assert out.download(np.float32, (T.B, H, W, 2)).tobytes() == want.tobytes()
            small = ctx.alloc(T.B * 12 * 16 * 8)
            bufs.append(small)
            assert ctx.resize(df, None, fx=0.5, fy=0.5, format=R.F32C2, ssize=(32, 24), batch=T.B, dst=small) is small
            assert small.download(np.float32, (T.B, 12, 16, 2)).tobytes() == np.stack([R.resize(field[b], 16, 12, R.LINEAR) for b in range(T.B)]).tobytes()
            ctx.resize_enqueue(dp, R.U8C3, 32, 24, 16, 12, K.INTER_NEAREST, T.B, small)
            ctx.sync()
            assert np.array_equal(small.download(np.uint8, (T.B, 12, 16, 3)), np.stack([R.resize(pred[b], 16, 12, R.NEAREST) for b in range(T.B)]))
            with pytest.raises(ValueError, match="mav_resize_dev: MAV_INTER_AREA enlarging"):
                ctx.resize_enqueue(dp, R.U8C3, 32, 24, 64, 48, K.INTER_AREA, T.B, small)
        finally:
            for b in bufs:
                b.free()


def test_detect_on_device_resized_inputs_equals_detect_on_the_restatements(mav):
    """The sky mask (sky_mask_enqueue) and a field resized to the frame (resize_enqueue, as get_gt_of resizes a .flo field) never leave
    the device; mav_detect_dev on them returns what ctx.detect returns for the restatement's host arrays."""
    from mavflow import _lib, resize as K, synth
    W, H = 64, 48
    pred = T.prediction(32, 24)[:1]
    small = (np.random.default_rng(11).normal(0, 2.0, (1, 24, 32, 2)) + np.array([1.5, -0.5])).astype(np.float32)
    samples = synth.foe_samples(W, H, 0).astype(np.uint32)
    fp, tp = _lib.foe_defaults(), _lib.thr_defaults()
    with _lib.Context(W, H, 1) as ctx:
        bufs = [ctx.alloc(pred.nbytes).upload(pred), ctx.alloc(small.nbytes).upload(small), ctx.alloc(W * H), ctx.alloc(W * H * 8),
                ctx.alloc(samples.nbytes).upload(samples), ctx.alloc(_lib.RESULT_DTYPE.itemsize), ctx.alloc(W * H), ctx.alloc(W * H)]
        dpred, dsmall, dsky, dflow, dsmp, dres, dmf, dmd = bufs
        try:
            ctx.sky_mask_enqueue(dpred, 32, 24, W, H, dsky)
            ctx.resize_enqueue(dsmall, R.F32C2, 32, 24, W, H, K.INTER_LINEAR, 1, dflow)
            _lib.check(ctx.lib.mav_detect_dev(ctx.h, dflow.ptr, dsmp.ptr, None, None, None, dsky.ptr, 1, C.byref(fp), C.byref(tp), None, dmf.ptr, dmd.ptr, dres.ptr))
            dev = (dres.download(_lib.RESULT_DTYPE, (1,)), dmf.download(np.uint8, (H, W)), dmd.download(np.uint8, (H, W)))
            sky, flow = R.sky_mask(pred[0], W, H), R.resize(small[0], W, H, R.LINEAR)
            assert sky.any() and not sky.all()
            host = ctx.detect(flow, samples, sky=sky)
            assert dev[0].tobytes() == host["results"].tobytes()
            assert np.array_equal(dev[1], host["mask_fixed"][0].view(np.uint8)) and np.array_equal(dev[2], host["mask_dyn"][0].view(np.uint8))
            without = ctx.detect(flow, samples)
            assert not np.array_equal(without["mask_fixed"], host["mask_fixed"]) or without["results"].tobytes() != host["results"].tobytes()   # the sky matters
        finally:
            for b in bufs:
                b.free()
