"""The inflate core on the host (mav_png_inflate_host: inflate_core.h with the serial copy) held to zlib over the case table of
tests/png_decode_cases.py, the case table held to its own names, the host un-filter pass held to tests/unfilter_ref.py, and the rule
for which files the device decodes.  Runs without a GPU.  Bytes are compared by equality."""
import os
import zlib

import numpy as np
import pytest

import png_decode_cases as pc
import unfilter_ref as ur

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def lib(mav):
    from mavflow import _lib
    return _lib.load()


def test_status_zero_iff_zlib_accepts_and_then_equal_bytes(lib):
    for c in pc.cases():
        want = pc.zlib_verdict(c.stream)
        raw, st = pc.inflate_host(lib, c.stream, c.raw_size)
        if want is not None and len(want) == c.raw_size:
            assert st["code"] == 0 and raw == want == c.raw, c.name
            assert st["adler_computed"] == st["adler_stream"] == zlib.adler32(want) and st["produced"] == len(want), c.name
        else:
            # zlib refuses the stream -- or accepts it with another size than the image has, which only this decoder can know
            assert c.raw is None and st["code"] == c.code != 0, (c.name, st)
            assert want is None or c.code in (pc.E["OVERFLOW"], pc.E["SHORT"]), c.name


def test_every_case_reaches_what_its_name_claims(lib):
    names = [c.name for c in pc.cases()]
    assert len(set(names)) == len(names)
    for c in pc.cases():
        _, st = pc.inflate_host(lib, c.stream, c.raw_size)
        assert c.claim(st), (c.name, st)
    assert sum(c.name.startswith("truncated_at_") for c in pc.cases()) == len(pc.cases()[-1].stream) + 1      # every byte of the short stream


def test_every_error_code_is_produced_by_some_case(lib, mav):
    from mavflow import _lib
    got = {pc.inflate_host(lib, c.stream, c.raw_size)[1]["code"] for c in pc.malformed_cases()}
    assert got == set(pc.E.values()) - {pc.E["FILTER"]}
    # FILTER is the un-filter pass's code (on the device: tests/test_gpu_png_decode.py): its case inflates well, and the host pass refuses it
    f = pc.filter_case()
    raw, st = pc.inflate_host(lib, f.stream, f.raw_size)
    assert st["code"] == 0 and raw == f.raw and f.claim(st)
    out = np.zeros(len(raw) - 1, np.uint8)
    rows = np.frombuffer(raw, np.uint8)
    assert lib.mav_png_unfilter(rows.ctypes.data, 1, len(raw) - 1, 1, out.ctypes.data) == _lib.MAV_ERR_ARG
    assert list(_lib.PNG_ERRORS[1:]) == list(pc.E) and [pc.E[k] for k in pc.E] == list(range(1, 12))
    assert _lib.PNG_STATUS_DTYPE == pc.STATUS_DTYPE


def test_seeded_mutations_agree_with_zlib(lib):
    """bit flips, truncations, splices and insertions of the valid streams: accepted iff zlib accepts, and then the same bytes (the size
    asked for is zlib's where it accepts, the original's where it does not)"""
    accepted = 0
    for z, n in pc.mutations(4000, 20261021):
        want = pc.zlib_verdict(z)
        raw, st = pc.inflate_host(lib, z, n if want is None else len(want))
        assert (st["code"] == 0) == (want is not None), (z.hex(), st)
        if want is not None:
            assert raw == want
            accepted += 1
    assert 0 < accepted < 4000


def test_trailing_bytes_are_ignored_as_zlib_ignores_them(lib):
    c = next(c for c in pc.cases() if c.name == "trailing_bytes_after_adler")
    assert zlib.decompress(c.stream) == c.raw
    _, st = pc.inflate_host(lib, c.stream, c.raw_size)
    assert st["consumed"] == len(c.stream) - len(b"trailing junk")


def test_host_unfilter_equals_the_numpy_reference(lib):
    for W, H in pc.RAW_SHAPES:
        for bpp in (1, 2, 3, 4):
            want, raws = pc.unfilter_raw(W, H, bpp)
            imgs, img_raws = pc.unfilter_images(W, H, bpp)
            for k in range(25):
                for raw, exp in ((raws[k], want[k]), (img_raws[k], imgs[k])):
                    a = np.frombuffer(raw, np.uint8)
                    out = np.empty((H, W * bpp), np.uint8)
                    assert lib.mav_png_unfilter(a.ctypes.data, H, W * bpp, bpp, out.ctypes.data) == 0
                    assert np.array_equal(out.reshape(H, W, bpp), exp), (W, H, bpp, k)
    # the 25 images of a shape carry every ordered pair of filter types on rows 0, 1 and on rows 1, 2
    pairs01 = {tuple(pc.filter_types(k, 3)[:2]) for k in range(25)}
    pairs12 = {tuple(pc.filter_types(k, 3)[1:3]) for k in range(25)}
    assert len(pairs01) == len(pairs12) == 25


def test_eligibility_of_the_golden_fixtures(mav):
    """8-bit, colour type 0 / 2 / 4 / 6, not interlaced: the seven single files of those types -- and the three frames of the fixture's
    sequence, which are plain 8-bit RGB files as well.  Every other fixture (depths 1 / 2 / 4 / 16, palette, Adam7) is not."""
    from mavflow import frame_source
    z = np.load(os.path.join(GOLDEN, "png_frames.npz"), allow_pickle=False)
    names = [k[4:] for k in z.files if k.startswith("png_")]
    eligible = {n for n in names if frame_source.device_eligible(frame_source.png_chunks(z["png_" + n].tobytes())[0])}
    assert eligible == {"gray8_forced", "graya8_forced", "rgb8_forced", "rgba8_forced", "rgb8_pil", "gray8_pil", "rgba8_pil", "seq0", "seq1", "seq2"}
    assert len(names) == 36
    for n in set(names) - eligible:
        W, H, depth, ctype, _, _, interlace = frame_source.png_chunks(z["png_" + n].tobytes())[0]
        assert depth != 8 or ctype == 3 or interlace == 1, n


def test_png_chunks_crc_modes(mav):
    from mavflow import frame_source
    z = np.load(os.path.join(GOLDEN, "png_frames.npz"), allow_pickle=False)
    data = bytearray(z["png_rgb8_forced"].tobytes())
    ihdr, plte, trns, spans = frame_source.png_chunks(bytes(data))
    assert ihdr[:5] == (33, 29, 8, 2, 0) and plte is None and trns is None and len(spans) >= 1
    o, n = spans[0]
    data[o + n] ^= 0xFF                                # the IDAT chunk's CRC
    with pytest.raises(ValueError, match="CRC"):
        frame_source.png_chunks(bytes(data))
    assert frame_source.png_chunks(bytes(data), "small")[3] == spans
    data[o + n] ^= 0xFF
    data[8 + 8 + 13] ^= 0xFF                           # IHDR's CRC: checked on both routes
    with pytest.raises(ValueError, match="CRC"):
        frame_source.png_chunks(bytes(data), "small")
