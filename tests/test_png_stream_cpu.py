"""Host side of the device PNG encoder, no GPU: the chunk framing (frame_source.png_wrap), the way independent deflate segments are
joined into one zlib stream (the device's layout, restated with the stdlib's raw deflate and with tests/png_stream_ref.py's literal
block layout) with the Adler-32 combined from per-segment partials, and mav_png_bound's formula."""
import ctypes
import struct
import zlib

import numpy as np
import pytest

import png_stream_ref as ref
from mavflow import _lib
from mavflow.frame_source import decode_png, encode_png, png_wrap

SEG = 24576                                                   # the device's segment length (DESIGN.md "PNG encoder")
MOD = 65521


def _scanlines(rows, ftype=0):
    """filter type 0 scanline stream of (H, n) u8 rows"""
    raw = np.empty((rows.shape[0], 1 + rows.shape[1]), np.uint8)
    raw[:, 0] = ftype
    raw[:, 1:] = rows
    return raw.tobytes()


@pytest.mark.parametrize("channels", [1, 3, 4])
def test_png_wrap_decodes_to_the_image(channels):
    rng = np.random.default_rng(channels)
    H, W = 37, 53
    img = rng.integers(0, 256, (H, W, channels), dtype=np.uint8)
    file_order = img[:, :, 0:1] if channels == 1 else img[:, :, [2, 1, 0] if channels == 3 else [2, 1, 0, 3]]
    png = png_wrap(W, H, channels, zlib.compress(_scanlines(file_order.reshape(H, -1)), 1))
    assert png == encode_png(img)                             # the same framing as the host encoder's, around the same stream
    px, ctype = decode_png(png)
    assert ctype == {1: 0, 3: 2, 4: 6}[channels]
    assert np.array_equal(px, file_order[:, :, 0] if channels == 1 else file_order)
    # a Sub-filtered stream (what the device sends) decodes to the same pixels
    sub = ref.sub_rows(np.ascontiguousarray(file_order))
    px2, _ = decode_png(png_wrap(W, H, channels, zlib.compress(sub)))
    assert np.array_equal(px2, px)
    with pytest.raises(ValueError):
        png_wrap(W, H, 2, b"")
    with pytest.raises(ValueError):
        png_wrap(0, H, 3, b"")


def _partial(seg: bytes):
    """(a, b, len) of one segment, as zlib counts: a = 1 + sum, b = len + sum of byte * (len - i), both mod 65521"""
    d = np.frombuffer(seg, np.uint8).astype(np.uint64)
    n = len(seg)
    return int((1 + d.sum()) % MOD), int((n + (d * np.arange(n, 0, -1, dtype=np.uint64)).sum()) % MOD), n


def _combine(p1, p2):
    (a1, b1, n1), (a2, b2, n2) = p1, p2
    return (a1 + a2 - 1) % MOD, (b1 + b2 + n2 * (a1 - 1)) % MOD, n1 + n2


def _joined(raw: bytes, seg: int) -> bytes:
    """the device's stream layout with the stdlib as the segment coder: 78 01, every segment a raw-deflate stream of its own that ends
    on a byte boundary (Z_FULL_FLUSH: an empty stored block; no match reaches back), the last one finished, Adler-32 from the partials"""
    out = [b"\x78\x01"]
    acc = (1, 0, 0)
    for o in range(0, len(raw), seg):
        part = raw[o:o + seg]
        c = zlib.compressobj(1, zlib.DEFLATED, -15)
        out.append(c.compress(part) + (c.flush(zlib.Z_FINISH) if o + seg >= len(raw) else c.flush(zlib.Z_FULL_FLUSH)))
        acc = _combine(acc, _partial(part))
    assert acc[2] == len(raw)
    return b"".join(out) + struct.pack(">I", (acc[1] << 16) | acc[0])


@pytest.mark.parametrize("n,seg", [(1, SEG), (SEG, SEG), (SEG + 1, SEG), (5 * SEG + 77, SEG), (300000, 65536), (200000, 100000)])
def test_joined_segments_inflate_and_the_adler_combine_is_exact(n, seg):
    rng = np.random.default_rng(n)
    raw = np.full(n, 255, np.uint8)                           # bytes of 255: the b partial of a 64 KB segment passes 2^32 unreduced
    raw[rng.integers(0, n, n // 3)] = rng.integers(0, 256, n // 3, dtype=np.uint8)
    raw = raw.tobytes()
    z = _joined(raw, seg)
    d = zlib.decompressobj()
    assert d.decompress(z) == raw and d.eof and d.unused_data == b""
    acc = (1, 0, 0)
    for o in range(0, n, seg):
        acc = _combine(acc, _partial(raw[o:o + seg]))
    assert ((acc[1] << 16) | acc[0]) == zlib.adler32(raw)
    if seg >= 65536:
        d8 = np.frombuffer(raw[:seg], np.uint8).astype(object)
        assert int((d8 * np.arange(seg, 0, -1).astype(object)).sum()) >= 1 << 32


def test_the_reference_block_layout_is_a_second_producer():
    """tests/png_stream_ref.py writes the device's block layout bit by bit (dynamic code, fixed code-length code, one 1-bit distance
    code, byte-run tokens, segments joined by empty stored blocks): zlib inflates it."""
    rng = np.random.default_rng(2)
    H, W = 24, 200
    y, x = np.mgrid[0:H, 0:W]
    for img in (np.full((H, W, 3), 7, np.uint8), np.stack([x % 256, (5 * y) % 256, (x + y) % 256], -1).astype(np.uint8),
                rng.integers(0, 256, (H, W, 3), dtype=np.uint8), np.full((1, 1, 3), 9, np.uint8)):
        raw = ref.sub_rows(img)
        z = ref.stream(raw, 8 * (1 + img.shape[1] * 3))
        d = zlib.decompressobj()
        assert d.decompress(z) == raw and d.eof and d.unused_data == b""
        px, ctype = decode_png(png_wrap(img.shape[1], img.shape[0], 3, z))
        assert ctype == 2 and np.array_equal(px, img)


def test_png_bound_is_its_documented_formula():
    lib = _lib.load()
    for W, H, C in [(1, 1, 1), (1, 7, 3), (3, 2, 4), (333, 227, 3), (640, 480, 1), (1920, 1080, 3), (3840, 2160, 3), (24575, 1, 1),
                    (24576, 1, 1), (8191, 3, 4)]:
        raw = H * (1 + W * C)
        segments = -(-raw // SEG)
        got = lib.mav_png_bound(W, H, C)
        assert got == raw + 5 * segments + 6, (W, H, C)
        assert got <= raw + 5 * -(-raw // 65535) + 9 * segments + 6          # a segment never costs more than its stored form
        assert got <= 1.01 * raw + 1024
    for bad in [(0, 5, 3), (5, 0, 3), (5, 5, 2), (5, 5, 0), (-1, 5, 1)]:
        assert lib.mav_png_bound(*bad) == 0
    assert lib.mav_png_bound.restype is ctypes.c_size_t
