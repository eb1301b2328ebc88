"""The Python surface of the device PNG decoder: Context.png_decode / farneback_png, frame_source.imread_many and the decoder= options
of the capture and the providers, held to the PIL-decoded fixtures (tests/golden/png_frames.npz) and to the host route.  Bytes are
compared by equality."""
import os
import zlib

import numpy as np
import pytest

import order_cases as oc
import png_decode_cases as pc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ELIGIBLE = ("gray8_forced", "graya8_forced", "rgb8_forced", "rgba8_forced", "rgb8_pil", "gray8_pil", "rgba8_pil", "seq0", "seq1", "seq2")
W, H = 66, 33


@pytest.fixture(scope="module")
def fixtures():
    z = np.load(os.path.join(GOLDEN, "png_frames.npz"), allow_pickle=False)
    return {k[4:]: (z[k].tobytes(), z["bgr_" + k[4:]]) for k in z.files if k.startswith("png_")}


@pytest.fixture(scope="module")
def ctx(mav):
    from mavflow import _lib
    with _lib.Context(W, H, 4) as c:
        yield c


@pytest.fixture(scope="module")
def frames():
    """7 BGR frames of 66 x 33 with a moving pattern, and their files (filter type 0, zlib level 1: frame_source.encode_png)"""
    from mavflow import frame_source
    rng = np.random.default_rng(66)
    base = rng.integers(0, 256, (H + 8, W + 16, 3), dtype=np.uint8)
    base = (base // 4 + np.add.outer(np.arange(H + 8) * 3, np.arange(W + 16) * 2)[..., None]).astype(np.uint8)
    imgs = [np.ascontiguousarray(base[k // 2:k // 2 + H, k:k + W]) for k in range(7)]
    return imgs, [frame_source.encode_png(f) for f in imgs]


def test_every_eligible_fixture_decodes_to_the_pil_array_on_the_device(ctx, fixtures):
    from mavflow import frame_source
    for name in ELIGIBLE:
        data, bgr = fixtures[name]
        got = frame_source.imread_many([data], ctx)
        assert got.routes == ["device"] and np.array_equal(got.frames[0], bgr), name
        assert np.array_equal(ctx.png_decode([data])[0], bgr), name
        px, ctype = frame_source.decode_png(data)
        assert np.array_equal(ctx.png_decode([data], out="samples")[0], px), name
        assert np.array_equal(ctx.png_decode([data], out="gray")[0], frame_source._to_out(px, ctype, "gray")), name


def test_ineligible_fixtures_take_the_fallback(ctx, fixtures):
    from mavflow import frame_source
    rest = sorted(set(fixtures) - set(ELIGIBLE))
    assert len(rest) == 26
    got = frame_source.imread_many([fixtures[n][0] for n in rest], ctx)
    assert got.routes == ["host"] * len(rest)
    for n, f in zip(rest, got.frames):
        assert np.array_equal(f, fixtures[n][1]), n
    with pytest.raises(ValueError, match="file 0 is not one the device decodes"):
        ctx.png_decode([fixtures[rest[0]][0]])


def test_imread_many_on_a_mixed_list(ctx, fixtures, tmp_path):
    from mavflow import frame_source
    names = ["seq0", "pal_pil", "rgb8_forced", "seq1", "adam7_rgb8", "gray16_forced", "seq2", "gray8_pil", "rgb8_forced"]
    items = [fixtures[n][0] for n in names]
    path = tmp_path / "one.png"
    path.write_bytes(items[0])
    items[0] = str(path)                                     # a path among the bytes
    items += [b"not a png", str(tmp_path / "missing.png")]
    for out in ("bgr", "gray", "samples"):
        got = frame_source.imread_many(items, ctx, out)
        assert got.routes == ["device", "host", "device", "device", "host", "host", "device", "device", "device", None, None]
        assert got.frames[-1] is None and got.frames[-2] is None
        for n, f in zip(names, got.frames):
            px, ctype = frame_source.decode_png(fixtures[n][0])
            assert np.array_equal(f, frame_source._to_out(px, ctype, out)), (n, out)
            if out == "bgr":
                assert np.array_equal(f, fixtures[n][1]), n
    # the frames left on the device
    got = frame_source.imread_many(items, ctx, "gray")
    dev = frame_source.imread_many(items, ctx, "gray", to_host=False)
    try:
        assert dev.routes == got.routes and sorted(dev.device) == [0, 2, 3, 6, 7, 8] and dev.frames[2] is None
        buf, off, shape = dev.device[3]
        whole = buf.download(np.uint8, (buf.nbytes,))
        assert np.array_equal(whole[off:off + shape[0] * shape[1]].reshape(shape), got.frames[3])
    finally:
        dev.free()


def test_capture_device_decoder_reads_what_the_host_decoder_reads(frames, tmp_path):
    from mavflow import frame_source
    imgs, files = frames
    for k, data in enumerate(files):
        (tmp_path / f"image_{k:05d}.png").write_bytes(data)
    pattern = str(tmp_path / "image_%05d.png")
    host = frame_source.PngSequenceCapture(pattern)
    dev = frame_source.PngSequenceCapture(pattern, decoder="device", ahead=3)
    try:
        assert host.isOpened() and dev.isOpened() and [dev.get(p) for p in (3, 4, 7)] == [host.get(p) for p in (3, 4, 7)] == [W, H, 7]
        for seek in (None, 5, 1, 6, 0):
            if seek is not None:
                assert host.set(1, seek) and dev.set(1, seek)
            for _ in range(4):
                (ok_h, f_h), (ok_d, f_d) = host.read(), dev.read()
                assert ok_h == ok_d and host.get(1) == dev.get(1)
                if ok_h:
                    assert np.array_equal(f_h, f_d) and np.array_equal(f_d, imgs[int(dev.get(1)) - 1])
                else:
                    assert f_d is None
    finally:
        host.release()
        dev.release()


def test_farneback_png_equals_farneback_byte_for_byte(ctx, frames, tmp_path):
    from mavflow.flow_provider import FarnebackFlowProvider
    imgs, files = frames
    gray = ctx.bgr2gray(np.stack(imgs[:4]))
    want = ctx.farneback(gray[:-1], gray[1:])
    got = ctx.farneback_png(files[:4])
    assert got.shape == (3, H, W, 2) and got.tobytes() == want.tobytes()
    with pytest.raises(ValueError, match="max_batch"):
        ctx.farneback_png(files[:6])
    for k, data in enumerate(files[:4]):
        (tmp_path / f"image_{k:05d}.png").write_bytes(data)
    host = FarnebackFlowProvider.from_png_sequence(str(tmp_path), window=3, n_frames=4)
    dev = FarnebackFlowProvider.from_png_sequence(str(tmp_path), window=3, n_frames=4, png_decoder="device")
    try:
        for i in range(3):
            assert np.asarray(dev.get_flow_uv(i)).tobytes() == np.asarray(host.get_flow_uv(i)).tobytes() == want[i].tobytes(), i
    finally:
        host.release()
        dev.release()


def test_a_corrupt_file_in_the_middle_of_a_batch_is_named(ctx, frames):
    from mavflow import frame_source
    imgs, files = frames
    bad = bytearray(files[2])
    _, _, _, spans = frame_source.png_chunks(files[2])
    o, n = spans[0]
    bad[o + n // 2] ^= 0x10                                  # inside the deflate data
    batch = [files[0], files[1], bytes(bad), files[3]]
    with pytest.raises(ValueError, match=r"file 2: MAV_PNG_E_"):
        ctx.png_decode(batch)
    with pytest.raises(ValueError, match=r"file 2: MAV_PNG_E_"):
        ctx.farneback_png(batch)
    img, st = ctx.png_decode(batch, return_status=True)
    assert (st["code"] != 0).tolist() == [False, False, True, False] and not img[2].any()
    for k in (0, 1, 3):
        assert np.array_equal(img[k], imgs[k])
    got = frame_source.imread_many(batch, ctx)
    assert got.routes == ["device", "device", None, "device"] and got.frames[2] is None and frame_source.decode_png(files[3])[1] == 2


def test_verify_crc_both_ways(ctx, frames):
    """a wrong IDAT CRC over intact data: the device route decodes it, the host route and verify_crc=True do not"""
    from mavflow import frame_source
    imgs, files = frames
    _, _, _, spans = frame_source.png_chunks(files[1])
    o, n = spans[0]
    bad = bytearray(files[1])
    bad[o + n] ^= 0xFF                                       # the chunk's CRC field
    bad = bytes(bad)
    with pytest.raises(ValueError, match="CRC"):
        frame_source.decode_png(bad)
    assert np.array_equal(ctx.png_decode([files[0], bad])[1], imgs[1])
    with pytest.raises(ValueError, match="file 1: .*CRC"):
        ctx.png_decode([files[0], bad], verify_crc=True)
    got = frame_source.imread_many([files[0], bad], ctx)
    assert got.routes == ["device", "device"] and np.array_equal(got.frames[1], imgs[1])
    got = frame_source.imread_many([files[0], bad], ctx, verify_crc=True)
    assert got.routes == ["device", None] and got.frames[1] is None
    ihdr_bad = bytearray(files[1])
    ihdr_bad[8 + 8 + 13] ^= 0xFF                             # IHDR's CRC: a small chunk, checked on every route
    with pytest.raises(ValueError, match="file 0: .*CRC"):
        ctx.png_decode([bytes(ihdr_bad)])


def test_detect_after_a_seventy_stream_decode_is_a_fresh_contexts(mav):
    """light after heavy, in the spirit of tests/test_gpu_call_order.py: the decoder's staging blocks, scratch and launches leave nothing
    a later detect call reads"""
    from mavflow import _lib, _truth, _validation      # noqa: F401
    fw, fh = oc.FRAME
    with _lib.Context(fw, fh, oc.B) as fresh:
        want = oc.detect_light(fresh, {})
    rng = np.random.default_rng(7)
    raws = [bytes([k % 5]) + rng.integers(0, 256, 3 * 997, dtype=np.uint8).tobytes() for k in range(70)]
    streams, index = pc.pack([zlib.compress(r, 1) if k % 9 else zlib.compress(r, 1)[:40] for k, r in enumerate(raws)])
    with _lib.Context(fw, fh, oc.B) as c:
        img, st = c.png_decode_streams(streams, index, 997, 1, 3, "bgr", return_status=True)
        assert (st["code"] != 0).tolist() == [k % 9 == 0 for k in range(70)] and img[1].any()
        assert oc.detect_light(c, {}) == want
        c.png_decode_streams(streams, index, 997, 1, 3, "gray", return_status=True)
        assert oc.detect_light(c, {}) == want
