"""The C boundary of include/mavflow_jpeg.h: the header declares and the cross-compiled library exports every entry point of
_lib.JPEG_EXPORTS, each is bound in _lib.py, no other header names them, the records have their stated sizes, the scratch formula
holds, and calls are refused from their arguments alone with the function's name in mav_last_error().  Runs without a GPU."""
import os
import re

import numpy as np

import jpeg_cases as jc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mavflow_jpeg.h")
CSRC = os.path.join(ROOT, "mav-detection_amd", "csrc")


def test_header_declares_library_exports_and_lib_binds_the_symbols(mav):
    from mavflow import _lib
    raw = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = re.findall(r"\b(mav_jpeg_[a-z0-9_]+)\s*\(", txt)
    assert sorted(declared) == sorted(_lib.JPEG_EXPORTS) and len(declared) == 5
    lib = _lib.load()
    for s in _lib.JPEG_EXPORTS:
        assert hasattr(lib, s), f"libmavflow.so does not export {s}"
        assert s not in _lib.EXPORTS and s not in _lib.PNG_DECODE_EXPORTS
        assert getattr(lib, s).argtypes is not None, f"{s} is not bound in _lib.py"
    for other in os.listdir(os.path.join(ROOT, "include")):
        if other != "mavflow_jpeg.h":
            main = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", other)).read(), flags=re.S)
            assert not re.search(r"mav_jpeg_|MAV_JPEG_", main), other
    for name, value in [("MAV_JPEG_E_" + k, v) for k, v in jc.E.items()] + [("MAV_JPEG_OUT_" + k.upper(), v) for k, v in _lib.JPEG_OUT.items()] \
            + [("MAV_JPEG_MAX_COUNT", _lib.JPEG_MAX_COUNT)]:
        assert re.search(rf"#define\s+{name}\s+{value}\b", txt), name
    assert [_lib.JPEG_ERRORS.index(k) for k in jc.E] == list(jc.E.values())
    for phrase in ('#include "mavflow.h"', "the CALL'S OWN", "independent of the context's max_batch", "LEAVES ITS WHOLE OUTPUT AS ZERO BYTES",
                   "A refused call has enqueued and written nothing", "It is NOT\n *                           IMREAD_GRAYSCALE",
                   "LOWEST restart interval", "that table wraps, this decoder clamps", "warns and carries on"):
        assert phrase in raw, phrase
    for member in ("jpeg_decode", "jpeg_decode_dev", "jpeg_decode_packed", "jpeg_decode_to_device", "jpeg_decode_scratch_bytes", "farneback_jpeg"):
        assert hasattr(_lib.Context, member), member
    for fn in ("jpeg_parse", "jpeg_info", "jpeg_decode_host"):
        assert callable(getattr(_lib, fn))


def test_makefile_has_the_objects_own_rule_and_every_link_line(mav):
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert mk.count("$(BUILD)/kernels_jpeg.o") == 4                    # its own rule, libmavflow.so, the diag and variant link lines
    rule = mk[mk.index("$(BUILD)/kernels_jpeg.o:"):].split("\n")
    assert "kernels_jpeg.hip" in rule[0] and "jpeg_core.h" in rule[0] and "-ffp-contract=off" in rule[2]
    assert "jpeg_check:" in mk and "tools/jpeg_check.c" in mk and mk.count("-fsanitize=address,undefined") == 2
    assert mk.count("$(BUILD)/kernels_png_decode.o") == 4              # the PNG decoder's lines are as they were


def test_one_decoding_source_for_host_and_device():
    """the kernels, the host entry point and the sanitizer program all include jpeg_core.h, which has no assembly and no floating point"""
    core = open(os.path.join(CSRC, "jpeg_core.h")).read()
    code = re.sub(r"//.*", "", core)
    assert "asm" not in code and not re.search(r"\b(float|double)\b", code)
    hip = open(os.path.join(CSRC, "kernels_jpeg.hip")).read()
    assert '#include "jpeg_core.h"' in hip and "asm" not in re.sub(r"//.*", "", hip)
    assert '#include "jpeg_core.h"' in open(os.path.join(ROOT, "tools", "jpeg_check.c")).read()
    for fn in ("jc_decode_interval(", "jc_idct_pass(", "jc_pixel(", "jc_info_ok(", "jc_merge(", "jc_decode_host(", "jc_parse(", "bgr2gray_px("):
        assert fn in hip, fn
    for kernel in ("k_jpeg_intervals", "k_jpeg_entropy", "k_jpeg_idct", "k_jpeg_finish"):
        assert hip.count(f"hipLaunchKernelGGL({kernel},") == 1, kernel


def test_records_have_their_stated_sizes(mav):
    from mavflow import _lib
    assert _lib.JPEG_STATUS_DTYPE.itemsize == 40 and _lib.JPEG_INFO_DTYPE.itemsize == 2512
    assert [_lib.JPEG_STATUS_DTYPE.fields[k][1] for k in ("code", "intervals", "consumed", "mcus", "nonzero", "zrl", "stuffed", "max_code_len")] \
        == [0, 4, 8, 16, 20, 24, 28, 32]
    assert [_lib.JPEG_INFO_DTYPE.fields[k][1] for k in ("W", "H", "components", "restart_interval", "entropy_offset", "entropy_bytes", "comp",
                                                        "quant_defined", "dc_defined", "ac_defined", "quant", "dc", "ac")] \
        == [0, 4, 8, 12, 16, 24, 32, 64, 68, 72, 80, 336, 1424]
    raw = open(HEADER).read()
    assert "/* 40 bytes */" in raw and "/* 2512 bytes */" in raw


def test_scratch_bytes_and_refusals_without_a_gpu(mav):
    from mavflow import _lib
    lib = _lib.load()
    for W, H, comps, n in ((1, 1, 1, 1), (131, 67, 3, 70), (1920, 1080, 3, 1024), (1904, 1071, 1, 64), (65535, 65535, 3, 1)):
        blocks = 2 * ((W + 15) // 16) * 2 * ((H + 15) // 16)
        per = comps * blocks * 64 * 2 + comps * blocks * 64 + 16 + blocks * 16
        got = lib.mav_jpeg_decode_scratch_bytes(W, H, comps, n)
        assert got == per * n and got % 16 == 0
    for bad in ((0, 5, 1, 1), (5, 0, 1, 1), (5, 5, 0, 1), (5, 5, 2, 1), (5, 5, 4, 1), (5, 5, 1, 0), (5, 5, 1, 1025), (65536, 5, 1, 1), (5, 65536, 3, 1)):
        assert lib.mav_jpeg_decode_scratch_bytes(*bad) == 0, bad
    buf = np.zeros(4096, np.uint8)
    p = buf.ctypes.data
    assert lib.mav_jpeg_decode(None, p, p, p, 1, 4, 4, 1, p, p) == _lib.MAV_ERR_ARG and lib.mav_last_error().decode().startswith("mav_jpeg_decode:")
    assert lib.mav_jpeg_decode_dev(None, p, p, p, 1, 4, 4, 1, p, p, p) == _lib.MAV_ERR_ARG
    assert lib.mav_last_error().decode().startswith("mav_jpeg_decode_dev:")
    assert lib.mav_jpeg_parse(None, 4, p) == _lib.MAV_ERR_ARG and lib.mav_last_error().decode().startswith("mav_jpeg_parse:")
    assert lib.mav_jpeg_parse(p, 4, None) == _lib.MAV_ERR_ARG and lib.mav_last_error().decode().startswith("mav_jpeg_parse:")
    for args in ((None, 4, p, 1, p, p), (p, 4, None, 1, p, p), (p, 4, p, 1, None, p), (p, 4, p, 1, p, None), (p, 4, p, 7, p, p)):
        assert lib.mav_jpeg_decode_host(*args) == _lib.MAV_ERR_ARG and lib.mav_last_error().decode().startswith("mav_jpeg_decode_host:")
    assert not buf.any()


def test_python_refusals_name_the_file(mav):
    import pytest
    from mavflow import _lib, frame_source
    by = {c.name: c for c in jc.cases()}
    a, b = by["pil_33x31_420_q90_rmb2"].file, by["pil_33x31_gray_q35_rmb2"].file
    with pytest.raises(ValueError, match="file 1 is 33 x 31 x 1, file 0 is 33 x 31 x 3"):
        _lib.Context._jpeg_pack([a, b])
    with pytest.raises(ValueError, match=r"file 1: MAV_JPEG_E_UNSUPPORTED \(5\): mav_jpeg_parse: SOF2 \(progressive\)"):
        _lib.Context._jpeg_pack([a, by["pil_progressive"].file])
    with pytest.raises(ValueError, match="no files"):
        _lib.Context._jpeg_pack([])
    W, H, comps, packed, index, infos = _lib.Context._jpeg_pack([a, a])
    assert (W, H, comps) == (33, 31, 3) and index.tolist() == [[0, len(a)], [len(a), len(a)]] and packed[:len(a)].tobytes() == a
    assert infos.dtype == _lib.JPEG_INFO_DTYPE and infos.shape == (2,)
    st = np.zeros(3, _lib.JPEG_STATUS_DTYPE)
    st["code"][1] = 2
    with pytest.raises(ValueError, match=r"file 1: MAV_JPEG_E_CODE \(2\)"):
        _lib.Context._jpeg_raise(st)
    with pytest.raises(ValueError, match="png_encoder"):
        frame_source.jpg_to_png("/nonexistent", None, png_encoder="cuda")


def test_imread_dispatches_on_the_first_bytes(mav, tmp_path):
    from mavflow import frame_source
    by = {c.name: c for c in jc.cases()}
    good = by["pil_37x53_420_q90_rmr1"]
    (tmp_path / "7.jpg").write_bytes(good.file)
    (tmp_path / "disguised.png").write_bytes(good.file)                # the bytes decide, not the name
    (tmp_path / "p.jpg").write_bytes(by["pil_progressive"].file)
    (tmp_path / "cut.jpg").write_bytes(by["cut_in_last_mcu"].file)
    frame_source.imwrite(str(tmp_path / "real.png"), good.bgr)
    assert np.array_equal(frame_source.imread(str(tmp_path / "7.jpg")), good.bgr)
    assert np.array_equal(frame_source.imread(str(tmp_path / "disguised.png")), good.bgr)
    assert np.array_equal(frame_source.imread(str(tmp_path / "real.png")), good.bgr)
    assert frame_source.imread(str(tmp_path / "p.jpg")) is None and frame_source.imread(str(tmp_path / "cut.jpg")) is None
    assert frame_source.imread(str(tmp_path / "missing.jpg")) is None
