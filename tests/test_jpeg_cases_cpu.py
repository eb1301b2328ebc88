"""The JPEG decoding source on the host (mav_jpeg_decode_host, the source the device runs) against the case table: equal bytes to
Pillow's pixels -- stored, and live when Pillow imports -- in all three output formats, every claim, every refusal with its code and
zeros, and the parser against a Python walk of the segments.  Runs without a GPU."""
import io

import numpy as np
import pytest

import jpeg_cases as jc
import jpeg_ref

VALID = jc.valid()
REFUSED = [c for c in jc.cases() if c.code != 0]


def _status(st):
    return {k: int(st[k]) for k in st.dtype.names}


@pytest.fixture(scope="module")
def reference():
    """the numpy restatement of every valid case, computed once"""
    return {c.name: jpeg_ref.decode(c.file) for c in VALID}


@pytest.mark.parametrize("case", VALID, ids=lambda c: c.name)
def test_valid_case_equals_pillow_in_every_format_and_keeps_its_claim(mav, reference, case):
    from mavflow import _lib
    ref = reference[case.name]
    assert np.array_equal(ref["bgr"], case.bgr), "the numpy restatement itself disagrees with Pillow"
    bgr, st = _lib.jpeg_decode_host(case.file, "bgr", return_status=True)
    assert st["code"] == 0 and np.array_equal(bgr, case.bgr)
    assert case.claim(_status(st)), _status(st)
    b, g, r = (case.bgr[..., k].astype(np.uint32) for k in range(3))
    gray = _lib.jpeg_decode_host(case.file, "gray")
    assert np.array_equal(gray, ((b * 1868 + g * 9617 + r * 4899 + 8192) >> 14).astype(np.uint8)) and np.array_equal(gray, ref["gray"])
    samples = _lib.jpeg_decode_host(case.file, "samples")
    want = ref["samples"][..., 0] if ref["samples"].shape[2] == 1 else ref["samples"]
    assert samples.shape == want.shape and np.array_equal(samples, want)


def test_valid_cases_equal_live_pillow(mav):
    Image = pytest.importorskip("PIL.Image")
    from mavflow import _lib
    for case in VALID:
        live = np.asarray(Image.open(io.BytesIO(case.file)))
        assert np.array_equal(live, case.pixels), case.name
        want = np.repeat(live[..., None], 3, 2) if live.ndim == 2 else live[..., ::-1]
        assert np.array_equal(_lib.jpeg_decode_host(case.file, "bgr"), want), case.name


def test_the_table_reaches_its_corners(mav):
    from mavflow import _lib
    sts = {c.name: _status(_lib.jpeg_decode_host(c.file, "bgr", return_status=True)[1]) for c in VALID}
    assert any(s["max_code_len"] == 16 for n, s in sts.items() if "_q100_" in n)
    assert sts["pil_37x53_444_q90_rmb2_wraps_rst7"]["intervals"] >= 9
    assert any(s["zrl"] > 0 for n, s in sts.items() if n.startswith("pil_"))
    assert any(s["stuffed"] > 0 for n, s in sts.items() if n.startswith("pil_"))
    px = np.concatenate([c.pixels.ravel() for c in VALID if "_q100_" in c.name])
    assert px.min() == 0 and px.max() == 255                       # clamping at both ends


@pytest.mark.parametrize("case", REFUSED, ids=lambda c: c.name)
def test_refused_case_carries_its_code_and_zeros(mav, case):
    from mavflow import _lib
    lib = _lib.load()
    raw = np.frombuffer(case.file + b"\0", np.uint8)
    info = np.zeros(1, _lib.JPEG_INFO_DTYPE)
    rc = lib.mav_jpeg_parse(raw.ctypes.data, len(case.file), info.ctypes.data)
    if case.parser is not None:
        assert rc == case.code
        why = lib.mav_last_error().decode()
        assert why.startswith("mav_jpeg_parse:") and case.parser in why, why
        assert not info.tobytes().strip(b"\0")                     # a refused file leaves an all-zero info
        assert _lib.jpeg_decode_host(case.file) is None
        with pytest.raises(ValueError, match="MAV_JPEG_E_"):
            _lib.jpeg_parse(case.file)
        info["W"], info["H"], info["components"] = 8, 8, 1         # the sizes alone do not make it an info the parser produces
        for fmt in range(3):
            out = np.full((8, 8, 3), 0xAB, np.uint8)
            st = np.zeros(1, _lib.JPEG_STATUS_DTYPE)
            assert lib.mav_jpeg_decode_host(raw.ctypes.data, len(case.file), info.ctypes.data, fmt, out.ctypes.data, st.ctypes.data) == 0
            assert st["code"][0] == jc.E["UNSUPPORTED"] and not out.reshape(-1)[:64 * (1, 3, 1)[fmt]].any()
        return
    assert rc == 0
    W, H, n = int(info["W"][0]), int(info["H"][0]), int(info["components"][0])
    for fmt, oc in ((0, n), (1, 3), (2, 1)):
        out = np.full((H, W, oc), 0xAB, np.uint8)
        st = np.zeros(1, _lib.JPEG_STATUS_DTYPE)
        assert lib.mav_jpeg_decode_host(raw.ctypes.data, len(case.file), info.ctypes.data, fmt, out.ctypes.data, st.ctypes.data) == 0
        assert st["code"][0] == case.code, (jc.E, _status(st[0]))
        assert not out.any()
        assert case.claim(_status(st[0])), _status(st[0])
    assert _lib.jpeg_decode_host(case.file) is None


def test_an_info_the_parser_would_not_produce_is_unsupported(mav):
    from mavflow import _lib
    lib = _lib.load()
    case = VALID[5]
    raw = np.frombuffer(case.file + b"\0", np.uint8)
    good, _ = _lib.jpeg_info(case.file)
    H, W = case.bgr.shape[:2]
    for field, value in (("td", 3), ("tq", 2), ("h", 3)):
        info = good.copy()
        info["comp"][0, 0][field] = value
        out = np.full((H, W, 3), 0xAB, np.uint8)
        st = np.zeros(1, _lib.JPEG_STATUS_DTYPE)
        assert lib.mav_jpeg_decode_host(raw.ctypes.data, len(case.file), info.ctypes.data, 1, out.ctypes.data, st.ctypes.data) == 0
        assert st["code"][0] == jc.E["UNSUPPORTED"] and not out.any(), field
    info = good.copy()
    info["entropy_bytes"] += 1                                     # behind the file's end
    st = np.zeros(1, _lib.JPEG_STATUS_DTYPE)
    out = np.full((H, W, 3), 0xAB, np.uint8)
    lib.mav_jpeg_decode_host(raw.ctypes.data, len(case.file), info.ctypes.data, 1, out.ctypes.data, st.ctypes.data)
    assert st["code"][0] == jc.E["UNSUPPORTED"] and not out.any()


@pytest.mark.parametrize("case", VALID, ids=lambda c: c.name)
def test_parser_equals_a_python_walk_of_the_segments(mav, case):
    from mavflow import _lib
    got, want = _lib.jpeg_parse(case.file), jpeg_ref.walk(case.file)
    assert (got["W"], got["H"], got["restart_interval"]) == (want["W"], want["H"], want["restart_interval"])
    assert got["components"] == want["components"]
    assert (got["entropy_offset"], got["entropy_bytes"]) == (want["entropy_offset"], want["entropy_bytes"])
    assert got["entropy_offset"] + got["entropy_bytes"] == len(case.file)
    assert sorted(got["quant"]) == sorted(want["quant"]) and all(np.array_equal(got["quant"][k], want["quant"][k]) for k in want["quant"])
    for kind in ("dc", "ac"):
        assert sorted(got[kind]) == sorted(want[kind])
        for k in want[kind]:
            assert np.array_equal(got[kind][k][0], want[kind][k][0]) and np.array_equal(got[kind][k][1], want[kind][k][1])


def test_truncating_a_valid_file_anywhere_is_refused_or_decodes_without_harm(mav):
    """every cut of two files behind SOS: TRUNCATED (or, cut behind the last MCU's bits, the full picture) -- never another verdict"""
    from mavflow import _lib
    for case in (VALID[9], VALID[14]):
        off = _lib.jpeg_parse(case.file)["entropy_offset"]
        for cut in range(off, len(case.file)):
            img, st = _lib.jpeg_decode_host(case.file[:cut], "bgr", return_status=True)
            assert st["code"] in (0, jc.E["TRUNCATED"], jc.E["RESTART"]), (case.name, cut, _status(st))
            assert (st["code"] == 0 and np.array_equal(img, case.bgr)) or not img.any(), (case.name, cut)
