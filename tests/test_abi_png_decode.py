"""The C boundary of include/mavflow_png_decode.h: the header declares and the cross-compiled library exports every entry point of
_lib.PNG_DECODE_EXPORTS, each is bound in _lib.py, the status record is 48 bytes, the pure functions answer without a GPU, and calls
are refused from their arguments alone.  Runs without a GPU."""
import os
import re

import numpy as np

import png_decode_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mavflow_png_decode.h")
CSRC = os.path.join(ROOT, "mav-detection_amd", "csrc")


def test_header_declares_library_exports_and_lib_binds_the_symbols(mav):
    from mavflow import _lib
    raw = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = re.findall(r"\b(mav_png_[a-z0-9_]+)\s*\(", txt)
    assert sorted(declared) == sorted(_lib.PNG_DECODE_EXPORTS) and len(declared) == 4
    lib = _lib.load()
    for s in _lib.PNG_DECODE_EXPORTS:
        assert hasattr(lib, s), f"libmavflow.so does not export {s}"
        assert s not in _lib.EXPORTS                                   # include/mavflow.h's list stays what it was
        assert getattr(lib, s).argtypes is not None, f"{s} is not bound in _lib.py"
    for other in os.listdir(os.path.join(ROOT, "include")):
        if other != "mavflow_png_decode.h":
            main = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", other)).read(), flags=re.S)
            assert not re.search(r"mav_png_decode|mav_png_inflate|mav_png_status|MAV_PNG_E_|MAV_PNG_OUT_", main), other
    for name, value in [("MAV_PNG_E_" + k, v) for k, v in pc.E.items()] + [("MAV_PNG_OUT_" + k.upper(), v) for k, v in _lib.PNG_OUT.items()] \
            + [("MAV_PNG_DECODE_MAX_COUNT", _lib.PNG_DECODE_MAX_COUNT)]:
        assert re.search(rf"#define\s+{name}\s+{value}\b", txt), name
    for phrase in ('#include "mavflow.h"', "the CALL'S OWN", "independent of the context's max_batch", "LEAVES ITS WHOLE OUTPUT AS ZERO BYTES",
                   "A refused call has enqueued and written nothing", "as zlib.decompress ignores them", "THE VERDICTS are zlib's own"):
        assert phrase in raw, phrase
    for member in ("png_decode", "png_decode_dev", "png_decode_streams", "png_decode_to_device", "farneback_png"):
        assert hasattr(_lib.Context, member), member
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert mk.count("$(BUILD)/kernels_png_decode.o") == 4              # its own rule, libmavflow.so, the diag and variant link lines
    rule = mk[mk.index("$(BUILD)/kernels_png_decode.o:"):].split("\n")
    assert "kernels_png_decode.hip" in rule[0] and "inflate_core.h" in rule[0] and "-ffp-contract=off" in rule[2]
    assert "inflate_check:" in mk and "-fsanitize=address,undefined" in mk
    assert _lib.PNG_STATUS_DTYPE.itemsize == 48
    assert [_lib.PNG_STATUS_DTYPE.fields[k][1] for k in ("code", "adler_stream", "adler_computed", "blocks", "consumed", "produced", "max_length",
                                                         "max_distance")] == [0, 4, 8, 12, 24, 32, 40, 44]


def test_one_inflate_source_for_host_and_device():
    """the kernels, the host entry point and the sanitizer program all include inflate_core.h, which has no assembly and no floating point"""
    core = open(os.path.join(CSRC, "inflate_core.h")).read()
    code = re.sub(r"//.*", "", core)
    assert "asm" not in code and not re.search(r"\b(float|double)\b", code)
    assert '#include "inflate_core.h"' in open(os.path.join(CSRC, "kernels_png_decode.hip")).read()
    assert '#include "inflate_core.h"' in open(os.path.join(ROOT, "tools", "inflate_check", "main.cpp")).read()
    hip = open(os.path.join(CSRC, "kernels_png_decode.hip")).read()
    assert "inf_run(" in hip and "inf_inflate_host(" in hip and "bgr2gray_px(" in hip
    assert "bgr2gray_px(" in open(os.path.join(CSRC, "kernels_detect.hip")).read()          # the one gray function of both paths


def test_scratch_bytes_and_refusals_without_a_gpu(mav):
    from mavflow import _lib
    lib = _lib.load()
    for W, H, ch, n in ((1, 1, 1, 1), (131, 67, 3, 70), (1920, 1080, 4, 1024)):
        raw = H * (1 + W * ch)
        assert lib.mav_png_decode_scratch_bytes(W, H, ch, n) == (raw + 15) // 16 * 16 * n
    for bad in ((0, 5, 1, 1), (5, 0, 1, 1), (5, 5, 0, 1), (5, 5, 5, 1), (5, 5, 1, 0), (5, 5, 1, 1025), (1 << 15, 1 << 15, 4, 1)):
        assert lib.mav_png_decode_scratch_bytes(*bad) == 0, bad
    buf = np.zeros(64, np.uint8)
    p = buf.ctypes.data
    assert lib.mav_png_decode(None, p, p, 1, 4, 4, 1, 0, p, p) == _lib.MAV_ERR_ARG and lib.mav_last_error().decode().startswith("mav_png_decode:")
    assert lib.mav_png_decode_dev(None, p, p, 1, 4, 4, 1, 0, p, p, p) == _lib.MAV_ERR_ARG
    assert lib.mav_last_error().decode().startswith("mav_png_decode_dev:")
    assert lib.mav_png_inflate_host(p, 4, p, 4, None) == _lib.MAV_ERR_ARG and lib.mav_last_error().decode().startswith("mav_png_inflate_host:")
    assert not buf.any()


def test_python_refusals_name_the_file(mav):
    import pytest
    from mavflow import _lib, frame_source
    z = np.load(os.path.join(ROOT, "tests", "golden", "png_frames.npz"), allow_pickle=False)
    rgb, gray, pal = (z["png_" + k].tobytes() for k in ("rgb8_forced", "gray8_forced", "pal_pil"))
    with pytest.raises(ValueError, match="file 1 is 48 x 37 x 1, file 0 is 33 x 29 x 3"):
        _lib.Context._png_streams([rgb, gray])
    with pytest.raises(ValueError, match="file 1 is not one the device decodes"):
        _lib.Context._png_streams([rgb, pal])
    with pytest.raises(ValueError, match="file 0: not a PNG file"):
        _lib.Context._png_streams([b"nothing"])
    W, H, ch, streams, index = _lib.Context._png_streams([rgb, rgb])
    assert (W, H, ch) == (33, 29, 3) and index.tolist() == [[0, index[0, 1]], [index[0, 1], index[0, 1]]]
    _, _, _, spans = frame_source.png_chunks(rgb)
    assert streams[:int(index[0, 1])].tobytes() == b"".join(rgb[o:o + n] for o, n in spans)
    st = np.zeros(3, _lib.PNG_STATUS_DTYPE)
    st["code"][1] = 10
    with pytest.raises(ValueError, match=r"file 1: MAV_PNG_E_ADLER \(10\)"):
        _lib.Context._png_raise(st)
    with pytest.raises(ValueError, match="decoder"):
        frame_source.PngSequenceCapture("/nonexistent/image_%05d.png", decoder="cuda")
