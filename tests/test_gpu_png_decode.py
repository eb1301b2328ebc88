"""PNG decode on the device (include/mavflow_png_decode.h) held to zlib, to the host build of the same inflate source, to
tests/unfilter_ref.py and to the images themselves.  Bytes are compared by equality; there is no tolerance anywhere.

A valid case's raw bytes go up as ONE image row (H = 1, W = raw size - 1, one channel: the first raw byte is the row's filter type, 0 - 4
by the table's construction), so the decoded samples are the un-filtered rest of the raw bytes: every raw byte is held."""
import ctypes as C
import zlib

import numpy as np
import pytest

import order_cases as oc
import png_decode_cases as pc
import unfilter_ref as ur

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(mav):
    from mavflow import _lib
    with _lib.Context(131, 67, 2) as c:
        yield c


@pytest.fixture(scope="module")
def lib(mav):
    from mavflow import _lib
    return _lib.load()


def _row_of(raw):
    """what a valid case's raw bytes decode to as one row of one-channel samples"""
    return ur.unfilter(raw, 1, len(raw) - 1, 1).reshape(-1)


def _host_status(lib, c):
    return pc.inflate_host(lib, c.stream, c.raw_size)[1]


def test_every_valid_case_alone(ctx, lib):
    for c in pc.valid_cases():
        streams, index = pc.pack([c.stream])
        img, st = ctx.png_decode_streams(streams, index, c.raw_size - 1, 1, 1, "samples", return_status=True)
        got = pc.status_dict(st[0])
        assert got["code"] == 0 and got == _host_status(lib, c), (c.name, got)
        assert got["adler_computed"] == zlib.adler32(c.raw) and c.claim(got), c.name
        assert np.array_equal(img.reshape(-1), _row_of(c.raw)), c.name
        assert zlib.decompress(c.stream) == c.raw


def test_malformed_family_in_one_call_with_valid_neighbours(ctx, lib):
    """every malformed case in ONE call, each between two valid streams: codes and counters equal to the host build's, refused images
    all zero, the neighbours unharmed"""
    group = list(pc.malformed_cases())
    size = group[0].raw_size
    assert all(c.raw_size == size for c in group)
    good_raw = b"\x01" + bytes((7 * i + size) & 255 for i in range(size - 1))
    good = zlib.compress(good_raw, 6)
    streams, index = pc.pack([z for c in group for z in (good, c.stream)] + [good])
    img, st = ctx.png_decode_streams(streams, index, size - 1, 1, 1, "samples", return_status=True)
    assert img.shape == (2 * len(group) + 1, 1, size - 1)
    seen = set()
    for j, c in enumerate(group):
        got = pc.status_dict(st[2 * j + 1])
        assert got["code"] == c.code and got == _host_status(lib, c) and c.claim(got), (c.name, got)
        assert not img[2 * j + 1].any(), c.name
        seen.add(got["code"])
    for j in range(0, 2 * len(group) + 1, 2):
        assert st["code"][j] == 0 and np.array_equal(img[j].reshape(-1), _row_of(good_raw)), j
    assert seen == set(pc.E.values()) - {pc.E["FILTER"]}
    # FILTER: a stream that inflates well to a row whose filter byte is 5
    f = pc.filter_case()
    ok = zlib.compress(b"\x02" + f.raw[1:], 1)
    streams, index = pc.pack([ok, f.stream, ok])
    img, st = ctx.png_decode_streams(streams, index, f.raw_size - 1, 1, 1, "bgr", return_status=True)
    assert st["code"].tolist() == [0, pc.E["FILTER"], 0] and not img[1].any() and img[0].any() and np.array_equal(img[0], img[2])
    assert st["adler_computed"][1] == st["adler_stream"][1] == zlib.adler32(f.raw) and st["produced"][1] == f.raw_size
    with pytest.raises(ValueError, match=r"file 1: MAV_PNG_E_FILTER \(11\)"):
        ctx.png_decode_streams(streams, index, f.raw_size - 1, 1, 1, "bgr")


@pytest.mark.parametrize("bpp", [1, 2, 3, 4])
def test_unfilter_and_convert(ctx, bpp):
    """all 25 ordered pairs of filter types on rows 0, 1 and 1, 2 (pc.filter_types), random bytes and bytes built for Paeth ties, every
    shape, all three output formats: the decoded images are the images that were filtered; raw random bytes decode to what
    tests/unfilter_ref.py makes of them"""
    for W, H in pc.SHAPES:
        imgs, raws = pc.unfilter_images(W, H, bpp)
        streams, index = pc.pack([zlib.compress(r, 1) for r in raws])
        for out in ("samples", "bgr", "gray"):
            got = ctx.png_decode_streams(streams, index, W, H, bpp, out)
            want = ur.convert(imgs, out)
            assert np.array_equal(got.reshape(want.shape), want), (W, H, bpp, out)
        if (W, H) in pc.RAW_SHAPES:
            want, raws = pc.unfilter_raw(W, H, bpp)
            streams, index = pc.pack([zlib.compress(r, 1) for r in raws])
            got = ctx.png_decode_streams(streams, index, W, H, bpp, "samples")
            assert np.array_equal(got.reshape(want.shape), want), (W, H, bpp)


def test_gray_equals_bgr2gray_of_the_bgr_output(ctx):
    W, H = ctx.W, ctx.H
    rng = np.random.default_rng(5)
    for bpp in (1, 2, 3, 4):
        imgs = rng.integers(0, 256, (2, H, W, bpp), dtype=np.uint8)
        raws = [ur.filter_rows(imgs[k].reshape(H, W * bpp), bpp, pc.filter_types(7 + k, H)) for k in range(2)]
        streams, index = pc.pack([zlib.compress(r, 6) for r in raws])
        bgr = ctx.png_decode_streams(streams, index, W, H, bpp, "bgr")
        gray = ctx.png_decode_streams(streams, index, W, H, bpp, "gray")
        assert np.array_equal(gray, ctx.bgr2gray(bgr)) and np.array_equal(bgr, ur.convert(imgs, "bgr")), bpp


def test_round_trip_of_the_device_encoder_on_its_device_index(ctx):
    """mav_png_encode_dev's streams and index, as they lie on the device, are mav_png_decode_dev's inputs: the identity"""
    from mavflow import _lib
    noise, flat = oc.png_images(ctx.W, ctx.H)
    W, H = ctx.W, ctx.H
    for imgs, ch in ((noise[:2], 4), (np.ascontiguousarray(noise[:2, :, :, :3]), 3), (flat[..., None], 1)):
        n = imgs.shape[0]
        bound = ctx.lib.mav_png_bound(W, H, ch) * n
        d_img, d_z, d_idx = ctx.alloc(imgs.nbytes).upload(imgs), ctx.alloc(bound), ctx.alloc(16 * n)
        d_out, d_st = ctx.alloc(imgs.nbytes), ctx.alloc(48 * n)
        d_scr = ctx.alloc(ctx.png_decode_scratch_bytes(W, H, ch, n))
        try:
            _lib.check(ctx.lib.mav_png_encode_dev(ctx.h, d_img.ptr, n, ch, d_z.ptr, C.c_size_t(bound), d_idx.ptr))
            ctx.png_decode_dev(d_z, d_idx, n, W, H, ch, "samples", d_out, d_st, d_scr)
            st = d_st.download(_lib.PNG_STATUS_DTYPE, (n,))
            got = d_out.download(np.uint8, imgs.shape)
            assert not st["code"].any() and (st["produced"] == H * (1 + W * ch)).all()
            # the file holds RGB(A): the samples are the BGR(A) image with B and R exchanged
            want = imgs if ch == 1 else imgs[..., [2, 1, 0] + ([3] if ch == 4 else [])]
            assert np.array_equal(got, want), ch
            if ch >= 3:
                ctx.png_decode_dev(d_z, d_idx, n, W, H, ch, "bgr", d_out, d_st, d_scr)
                assert np.array_equal(d_out.download(np.uint8, (n, H, W, 3)), imgs[..., :3]), ch
        finally:
            ctx.sync()
            for b in (d_img, d_z, d_idx, d_out, d_st, d_scr):
                b.free()


def test_seventy_mixed_streams_in_one_call(ctx, lib):
    """more streams than a workgroup has lanes and more than max_batch: valid streams of every writer and refused ones, interleaved"""
    size = 300
    rng = np.random.default_rng(70)
    raws, streams = [], []
    for k in range(70):
        body = rng.integers(0, 256 if k % 3 else 4, size - 1, dtype=np.uint8).tobytes()
        raw = bytes([k % 5]) + body
        z = zlib.compress(raw, (0, 1, 6, 9)[k % 4])
        if k % 7 == 3:
            z = z[:len(z) // 2]                        # TRUNCATED
            raw = None
        elif k % 7 == 5:
            z = z[:-1] + bytes([z[-1] ^ 1])            # ADLER
            raw = None
        raws.append(raw)
        streams.append(z)
    packed, index = pc.pack(streams)
    img, st = ctx.png_decode_streams(packed, index, size - 1, 1, 1, "samples", return_status=True)
    for k in range(70):
        want = pc.inflate_host(lib, streams[k], size)[1]
        assert pc.status_dict(st[k]) == want, k
        if raws[k] is None:
            assert want["code"] in (pc.E["TRUNCATED"], pc.E["ADLER"]) and not img[k].any(), k
        else:
            assert want["code"] == 0 and np.array_equal(img[k].reshape(-1), _row_of(raws[k])), k
