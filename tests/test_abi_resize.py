"""The C boundary of include/mavflow_resize.h: the header declares and the cross-compiled library exports exactly the entry points of
mavflow.resize.EXPORTS (none of them in another header or in _lib.EXPORTS), the constants are cv2's (a small C program compiled against
the header, here and now), and calls that must be refused from their arguments alone are refused with MAV_ERR_ARG, the function's name
in the message and the outputs untouched -- before the context is looked at.  Runs without a GPU."""
import ctypes as C
import glob
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mavflow_resize.h")
CANARY = 0x5A5A5A5A5A5A5A5A


def test_header_declares_and_library_exports_the_symbols(mav):
    from mavflow import _lib, resize
    raw = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = re.findall(r"\b(mav_(?:resize|sky_mask)[a-z0-9_]*)\s*\(", txt)
    assert sorted(declared) == sorted(resize.EXPORTS) and len(declared) == 4
    assert sorted(re.findall(r"\bint\s+(mav_\w+)\s*\(", txt)) == sorted(resize.EXPORTS)            # and declares nothing else
    lib = resize.load()
    for s in resize.EXPORTS:
        assert hasattr(lib, s), f"libmavflow.so does not export {s}"
        assert s not in _lib.EXPORTS                       # include/mavflow.h's list stays what it was
        assert (s + "_dev" in resize.EXPORTS) != s.endswith("_dev")           # a host form and a _dev form each
    for other in glob.glob(os.path.join(ROOT, "include", "*.h")):
        if os.path.basename(other) == "mavflow_resize.h":
            continue
        main = re.sub(r"/\*.*?\*/", "", open(other).read(), flags=re.S)
        assert not re.search(r"mav_resize|mav_sky_mask|MAV_INTER_", main), other
    for phrase in ('#include "mavflow_warp.h"', "as remembered from OpenCV 4.x `modules/imgproc/src/resize.cpp`, NOT pinned against a cv2 build",
                   "What to re-check first against a cv2 build", "cv2's SIMD helper for one-channel float32 and its summation order",
                   "A refused call has enqueued and written nothing", "IS the definition", "rounds a half UP", "ONE-TAP REGION", "0x7FC00000",
                   "never written", "(double)sw / dw", "no FMA", "DBL_EPSILON", "allocate nothing"):
        assert phrase in raw, phrase
    for member in ("resize", "sky_mask"):
        assert hasattr(_lib.Context, member) and hasattr(_lib.Context, member + "_enqueue"), member
    mk = open(os.path.join(ROOT, "mav-detection_amd", "csrc", "Makefile")).read()
    assert mk.count("$(BUILD)/kernels_resize.o") == 4              # its own rule, libmavflow.so, the diag and variant link lines
    rule = mk[mk.index("$(BUILD)/kernels_resize.o:"):]
    assert "-ffp-contract=off" in rule.split("\n")[2] and "kernels_resize.hip" in rule.split("\n")[0]
    # the area table has one home, used by both kernel files
    csrc = os.path.join(ROOT, "mav-detection_amd", "csrc")
    homes = [f for f in glob.glob(os.path.join(csrc, "*")) if os.path.isfile(f) and "struct AreaSpan" in open(f, errors="ignore").read()]
    assert [os.path.basename(f) for f in homes] == ["resize_area.h"]
    for user in ("kernels_window.hip", "kernels_resize.hip"):
        assert '#include "resize_area.h"' in open(os.path.join(csrc, user)).read(), user


def test_constants_match_the_header_and_cv2(mav, tmp_path):
    from mavflow import _lib, resize as K, warp
    import resize_ref as R
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc is not None, "a C compiler is needed to read the header's constants"
    macros = ("MAV_INTER_NEAREST", "MAV_INTER_LINEAR", "MAV_INTER_AREA", "MAV_RESIZE_MAX_SIDE", "MAV_WARP_U8C1", "MAV_WARP_U8C3", "MAV_WARP_F32C1", "MAV_WARP_F32C2")
    lines = ['#include <stdio.h>', '#include "mavflow_resize.h"', "int main(void) {"]
    for macro in macros:
        lines.append(f'  printf("{macro} %d\\n", (int)({macro}));')
    lines.append('  printf("step %zu\\n", sizeof(mav_frame_step));')
    lines.append("  return 0; }")
    src = tmp_path / "consts.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "consts"
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = {k: int(v) for k, v in (line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())}
    assert [got[m] for m in macros] == [K.INTER_NEAREST, K.INTER_LINEAR, K.INTER_AREA, K.MAX_SIDE, warp.WARP_U8C1, warp.WARP_U8C3, warp.WARP_F32C1, warp.WARP_F32C2]
    assert [got[m] for m in macros] == [R.NEAREST, R.LINEAR, R.AREA, R.MAX_SIDE, R.U8C1, R.U8C3, R.F32C1, R.F32C2] == [0, 1, 3, 32767, 0, 1, 2, 3]
    assert (K.INTER_NEAREST, K.INTER_LINEAR, K.INTER_CUBIC, K.INTER_AREA, K.INTER_LANCZOS4, K.INTER_LINEAR_EXACT) == (0, 1, 2, 3, 4, 5)      # cv2's values
    assert got["step"] == C.sizeof(_lib.FrameStep) == 488                   # nothing was added to the loop's struct


def test_refused_calls_leave_the_outputs_untouched(mav):
    from mavflow import _lib, resize as K, warp
    lib, ptr = K.load(), _lib._ptr
    src = np.ones(4096, np.float32)
    dst = np.full(4096, CANARY, np.uint64)
    fake_ctx = C.c_void_p(C.addressof(C.create_string_buffer(64)))          # a handle that must never be dereferenced
    s, d = ptr(src), ptr(dst)
    off = lambda v, n: C.c_void_p(v.value + n)

    def run(name, ok, calls):
        fn = getattr(lib, name)
        sub = lambda k, v: ok[:k] + (v,) + ok[k + 1:]
        for what, subs in calls.items():
            args = ok
            for k, v in (subs if isinstance(subs, list) else [subs]):
                args = args[:k] + (v,) + args[k + 1:]
            assert fn(*args) == _lib.MAV_ERR_ARG, (name, what)
            msg = lib.mav_last_error()
            assert name.encode() + b":" in msg and what.split(" ")[0].encode() in msg, (name, what, msg)

    for name in ("mav_resize", "mav_resize_dev"):
        # ctx, src, format, sw, sh, dw, dh, interpolation, batch, dst
        calls = {"NULL context": (0, None), "NULL src": (1, None), "NULL dst": (9, None), "format 4": (2, 4), "format -1": (2, -1),
                 "interpolation 2": (7, 2), "interpolation 4": (7, 4), "interpolation -1": (7, -1), "interpolation 5": (7, 5),
                 "sw 0": (3, 0), "sh -2": (4, -2), "dw 0": (5, 0), "dh 32768": (6, 32768), "sw 32768": (3, 32768), "dw 40000": (5, 40000),
                 "batch 0": (8, 0), "batch -3": (8, -3),
                 "MAV_INTER_AREA enlarging x": [(7, K.INTER_AREA), (5, 9)], "MAV_INTER_AREA enlarging y": [(7, K.INTER_AREA), (5, 4), (6, 7)],
                 "src and dst overlap (same)": (9, s), "src and dst overlap (tail)": (9, off(s, 8 * 6 * 8 - 4)), "src and dst overlap (head)": (1, off(d, 4 * 3 * 8 - 4))}
        if name.endswith("_dev"):
            calls.update({"src is not aligned": (1, off(s, 2)), "dst is not aligned": (9, off(d, 1))})
        run(name, (fake_ctx, s, warp.WARP_F32C2, 8, 6, 4, 3, K.INTER_LINEAR, 1, d), calls)
    for name in ("mav_sky_mask", "mav_sky_mask_dev"):
        # ctx, pred_bgr, sw, sh, dw, dh, key0, key1, batch, sky
        calls = {"NULL context": (0, None), "NULL pred_bgr": (1, None), "NULL sky": (9, None), "sw 0": (2, 0), "sh 40000": (3, 40000), "dw -1": (4, -1),
                 "dh 0": (5, 0), "key0 256": (6, 256), "key0 -1": (6, -1), "key1 256": (7, 256), "key1 -7": (7, -7), "batch 0": (8, 0),
                 "pred_bgr and sky overlap": (9, off(s, 8 * 6 * 3 - 1))}
        run(name, (fake_ctx, s, 8, 6, 16, 12, 180, 130, 1, d), calls)
    assert np.all(dst == CANARY) and np.all(src == 1)


def test_python_layer_refuses_what_is_not_built(mav):
    from mavflow import resize as K
    img = np.zeros((5, 7, 3), np.uint8)
    for interp in (K.INTER_CUBIC, K.INTER_LANCZOS4, K.INTER_LINEAR_EXACT, K.INTER_NEAREST_EXACT, 7):
        with pytest.raises(NotImplementedError):
            K.resize(img, (9, 9), interpolation=interp)
    with pytest.raises(NotImplementedError, match="INTER_AREA enlarging"):
        K.resize(img, (9, 4), interpolation=K.INTER_AREA)
    with pytest.raises(NotImplementedError, match="4 channels"):
        K.resize(np.zeros((5, 7, 4), np.uint8), (9, 9))
    with pytest.raises(NotImplementedError, match="uint16"):
        K.resize(np.zeros((5, 7), np.uint16), (9, 9))
    with pytest.raises(NotImplementedError):
        K.resize(np.zeros((5, 7, 3), np.float32), (9, 9))
    with pytest.raises(TypeError):
        K.resize(np.zeros((5, 7), np.float64), (9, 9))
    with pytest.raises(ValueError):
        K.resize(img, None)
    with pytest.raises(ValueError):
        K.resize(img, (0, 0), fx=0.5)
    assert K.dsize_of(7, 5, None, 0.5, 0.5) == (4, 2) and K.dsize_of(5, 7, (0, 0), 0.5, 0.5) == (2, 4)        # 3.5 -> 4, 2.5 -> 2: half to even
    assert K.dsize_of(7, 5, (3, 2), 9, 9) == (3, 2)


def test_shims_have_the_references_names(mav):
    from mavflow import im_helpers, resize as K
    assert list(inspect.signature(K.resize).parameters)[:6] == ["src", "dsize", "dst", "fx", "fy", "interpolation"]
    assert inspect.signature(K.resize).parameters["interpolation"].default == K.INTER_LINEAR
    assert list(inspect.signature(im_helpers.resize_percent).parameters) == ["img", "scale_percent"]
    assert list(inspect.signature(K.sky_segmentation).parameters) == ["prediction_bgr", "size"]
    assert inspect.signature(K.sky_segmentation).parameters["size"].default == (1920, 1024)
    assert list(inspect.signature(K.gt_of_resized).parameters) == ["flow", "capture_size"]
    f = np.zeros((6, 8, 2), np.float32)
    assert K.gt_of_resized(f, (8, 6)) is f                                  # the sizes agree: the input itself
