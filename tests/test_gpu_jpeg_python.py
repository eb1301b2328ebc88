"""The Python layer over the JPEG decoder: imread_many's routes, frames left on the device, jpg_to_png and farneback_jpeg."""
import os

import numpy as np
import pytest

import jpeg_cases as jc

pytestmark = pytest.mark.gpu
BY = {c.name: c for c in jc.cases()}


def test_imread_many_routes_png_jpeg_progressive_and_missing(mav, tmp_path):
    from mavflow import _lib, frame_source
    a, b, g = BY["pil_37x53_420_q90_rmr1"], BY["pil_37x53_444_q100_optimize"], BY["pil_37x53_gray_q100_plain"]
    png = frame_source.encode_png(a.bgr)
    files = [png, a.file, BY["pil_progressive"].file, str(tmp_path / "missing.jpg"), b.file, g.file, BY["cut_in_last_mcu"].file]
    with _lib.Context(64, 48, 1) as ctx:
        res = frame_source.imread_many(files, ctx, "bgr")
        assert res.routes == ["device", "device", None, None, "device", "device", None]
        assert sorted(res.refused) == [2, 6] and "SOF2 (progressive)" in res.refused[2] and "MAV_JPEG_E_TRUNCATED (1)" in res.refused[6]
        for k, want in ((0, a.bgr), (1, a.bgr), (4, b.bgr), (5, g.bgr)):
            assert np.array_equal(res.frames[k], want), k
        assert res.frames[2] is None and res.frames[3] is None and res.frames[6] is None
        gray = frame_source.imread_many(files, ctx, "gray")
        dev = frame_source.imread_many(files, ctx, "gray", to_host=False)
        try:
            assert dev.routes == res.routes and sorted(dev.refused) == [2, 6] and all(f is None for f in dev.frames)
            assert sorted(dev.device) == [0, 1, 4, 5]
            for k in dev.device:
                buf, off, shape = dev.device[k]
                whole = buf.download(np.uint8, (buf.nbytes,))
                assert np.array_equal(whole[off:off + shape[0] * shape[1]].reshape(shape), gray.frames[k]), k
        finally:
            dev.free()


def test_jpg_to_png_in_a_directory_of_five_files(mav, tmp_path):
    from mavflow import _lib, frame_source
    five = [c for c in jc.valid() if c.name.startswith("pil_37x53_") and "gray" not in c.name]
    five = (five * 2)[:5]
    numbers = [0, 3, 12, 250, 99999]
    for encoder in ("device", "host"):
        d = tmp_path / encoder
        d.mkdir()
        for n, c in zip(numbers, five):
            (d / f"{n}.jpg").write_bytes(c.file)
        (d / "notes.txt").write_text("stays")
        with _lib.Context(37, 53, 1) as ctx:
            got = frame_source.jpg_to_png(str(d), ctx, png_encoder=encoder)
        assert sorted(os.listdir(d)) == sorted([f"image_{n:05d}.png" for n in numbers] + ["notes.txt"])
        assert not got["refused"] and sorted(got["written"]) == sorted(str(d / f"image_{n:05d}.png") for n in numbers)
        for n, c in zip(numbers, five):
            assert np.array_equal(frame_source.imread(str(d / f"image_{n:05d}.png")), c.bgr), (encoder, n)
    d = tmp_path / "kept"
    d.mkdir()
    (d / "1.jpg").write_bytes(five[0].file)
    (d / "2.jpg").write_bytes(BY["pil_progressive"].file)
    with _lib.Context(37, 53, 1) as ctx:
        got = frame_source.jpg_to_png(str(d), ctx, remove=False)
    assert sorted(os.listdir(d)) == ["1.jpg", "2.jpg", "image_00001.png"] and list(got["refused"]) == [str(d / "2.jpg")]


def test_farneback_jpeg_equals_farneback_sequence_of_the_host_decoded_frames(mav):
    from mavflow import _lib
    frames = [BY[n].file for n in ("pil_64x48_420_q90_rmr1", "pil_64x48_444_q90_plain", "pil_64x48_422_q35_rmb2")]
    gray = np.stack([_lib.jpeg_decode_host(f, "gray") for f in frames])
    assert len({g.tobytes() for g in gray}) == 3
    with _lib.Context(64, 48, 2) as ctx:
        flow = ctx.farneback_jpeg(frames)
        want = ctx.farneback_sequence(gray)
        assert flow.shape == (2, 48, 64, 2) and flow.tobytes() == np.asarray(want).tobytes() and np.abs(flow).max() > 0
        with pytest.raises(ValueError, match="at least two files"):
            ctx.farneback_jpeg(frames[:1])
    with _lib.Context(32, 48, 2) as ctx:
        with pytest.raises(ValueError, match="the files are 64 x 48, the context is 32 x 48"):
            ctx.farneback_jpeg(frames)
