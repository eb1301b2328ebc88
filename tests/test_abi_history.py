"""The C boundary of the flow history: the header declares and the cross-compiled library exports every entry point, the layout of
mav_history_params matches its Python mirror (a small C program compiled against include/mavflow.h, here and now), the schedule is the
reference's loop, and calls that must be refused are refused with the outputs untouched.  Runs without a GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np

import history_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mav_history_defaults", "mav_history_schedule", "mav_history_create", "mav_history_destroy", "mav_history_reset",
           "mav_history_info", "mav_history_push", "mav_history_push_dev", "mav_stage_remap_linear")
CANARY = 0x5A5A5A5A5A5A5A5A


def test_header_declares_and_library_exports_the_symbols(mav):
    from mavflow import _lib
    raw = open(os.path.join(ROOT, "include", "mavflow.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    lib = _lib.load()
    for s in SYMBOLS:
        assert re.search(rf"\b{s}\s*\(", txt), f"include/mavflow.h does not declare {s}"
        assert hasattr(lib, s), f"libmavflow.so does not export {s}"
        assert s in _lib.EXPORTS
    # the semantics the header owes its reader
    for phrase in ("round_half_even(map_x * 32.0f)", "All four products are always formed", "NOT pinned against a cv2 build",
                   "k = (h + 1) % (L - 1); while k != h % (L - 1)", "would round and is MAV_ERR_ARG", "0x7FF8000000000000"):
        assert phrase in raw, phrase


def test_layout_and_constants_match_the_header(mav, tmp_path):
    from mavflow import _lib
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc is not None, "a C compiler is needed to read the header's layout"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mavflow.h"', "int main(void) {",
             '  printf("mav_history_params %zu\\n", sizeof(mav_history_params));']
    for name, _ in _lib.HistoryParams._fields_:
        lines.append(f'  printf("mav_history_params.{name} %zu\\n", offsetof(mav_history_params, {name}));')
    for macro in ("MAV_HISTORY_MAX_LENGTH", "MAV_HISTORY_AXES_XY", "MAV_HISTORY_OUT_REFERENCE", "MAV_HISTORY_OUT_FLOW_F32", "MAV_DEPTH_32F", "MAV_DEPTH_64F"):
        lines.append(f'  printf("{macro} %d\\n", {macro});')
    lines.append('  printf("step %zu\\n", sizeof(mav_frame_step));')
    lines.append("  return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = {k: int(v) for k, v in (line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())}
    assert got["mav_history_params"] == C.sizeof(_lib.HistoryParams) == 12
    for name, _ in _lib.HistoryParams._fields_:
        assert got[f"mav_history_params.{name}"] == getattr(_lib.HistoryParams, name).offset, name
    assert got["MAV_HISTORY_MAX_LENGTH"] == _lib.HISTORY_MAX_LENGTH == 64 and got["MAV_HISTORY_AXES_XY"] == _lib.HISTORY_AXES_XY == 1
    assert (got["MAV_HISTORY_OUT_REFERENCE"], got["MAV_HISTORY_OUT_FLOW_F32"]) == (_lib.HISTORY_OUT_REFERENCE, _lib.HISTORY_OUT_FLOW_F32) == (0, 1)
    assert (got["MAV_DEPTH_32F"], got["MAV_DEPTH_64F"]) == (_lib.DEPTH_32F, _lib.DEPTH_64F) == (5, 6)
    assert got["step"] == C.sizeof(_lib.FrameStep) == 488                   # nothing was added to the loop's struct
    p = _lib.HistoryParams()
    _lib.load().mav_history_defaults(C.byref(p))
    assert (p.length, p.depth, p.flags) == (20, _lib.DEPTH_32F, 0)


def test_schedule_is_the_loop_and_refuses_bad_arguments(mav):
    from mavflow import _lib
    lib = _lib.load()
    for L in range(3, _lib.HISTORY_MAX_LENGTH + 1):
        for h in range(L):
            assert _lib.history_schedule(L, h) == R.schedule(L, h), (L, h)
    slots = (C.c_int * 64)(*([-7] * 64))
    n = C.c_int(-7)
    for L, h in ((2, 0), (0, 0), (-1, 0), (65, 0), (20, 20), (20, -1), (3, 3)):
        assert lib.mav_history_schedule(L, h, slots, C.byref(n)) == _lib.MAV_ERR_ARG, (L, h)
        assert b"mav_history_schedule" in lib.mav_last_error()
    assert lib.mav_history_schedule(20, 0, None, C.byref(n)) == _lib.MAV_ERR_ARG
    assert lib.mav_history_schedule(20, 0, slots, None) == _lib.MAV_ERR_ARG
    assert n.value == -7 and list(slots) == [-7] * 64


def test_refused_calls_leave_the_outputs_untouched(mav):
    from mavflow import _lib
    lib, ptr = _lib.load(), _lib._ptr
    flow = np.zeros((4, 4, 2), np.float64)
    out = np.full(4 * 4 * 2 + 8, CANARY, np.uint64)
    mx = np.zeros((4, 4), np.float32)
    fake_ctx = C.c_void_p(C.addressof(C.create_string_buffer(64)))          # handles that must never be dereferenced
    fake_hist = C.c_void_p(C.addressof(C.create_string_buffer(64)))
    handle = C.c_void_p(CANARY)
    good = _lib.HistoryParams(20, _lib.DEPTH_32F, 0)

    # NULL handles
    assert lib.mav_history_create(None, C.byref(good), C.byref(handle)) == _lib.MAV_ERR_ARG and b"NULL context" in lib.mav_last_error()
    assert lib.mav_history_create(fake_ctx, C.byref(good), None) == _lib.MAV_ERR_ARG and b"NULL out" in lib.mav_last_error()
    for fn in (lib.mav_history_destroy, lib.mav_history_reset):
        assert fn(None, fake_hist) == _lib.MAV_ERR_ARG and b"NULL context" in lib.mav_last_error()
    assert lib.mav_history_info(None, fake_hist, None, None, None) == _lib.MAV_ERR_ARG
    # parameters are judged before the context is looked at
    for bad in ((2, _lib.DEPTH_32F, 0), (65, _lib.DEPTH_32F, 0), (20, _lib.DEPTH_8U, 0), (20, _lib.DEPTH_16U, 0), (20, 7, 0), (20, _lib.DEPTH_64F, 2),
                (20, _lib.DEPTH_32F, -1)):
        p = _lib.HistoryParams(*bad)
        assert lib.mav_history_create(fake_ctx, C.byref(p), C.byref(handle)) == _lib.MAV_ERR_ARG, bad
        assert b"mav_history_create" in lib.mav_last_error()
    assert handle.value == CANARY
    # a push: every argument that can be judged alone, for both entry points
    for name in ("mav_history_push", "mav_history_push_dev"):
        fn = getattr(lib, name)
        f, o = ptr(flow), ptr(out)
        f4, o4 = C.c_void_p(f.value + 4), C.c_void_p(o.value + 4)
        calls = {"NULL context": (None, fake_hist, f, _lib.DEPTH_64F, 1, 0, o), "NULL history": (fake_ctx, None, f, _lib.DEPTH_64F, 1, 0, o),
                 "NULL flow": (fake_ctx, fake_hist, None, _lib.DEPTH_64F, 1, 0, o), "NULL out": (fake_ctx, fake_hist, f, _lib.DEPTH_64F, 1, 0, None),
                 "flow_depth": (fake_ctx, fake_hist, f, _lib.DEPTH_8U, 1, 0, o), "out_form": (fake_ctx, fake_hist, f, _lib.DEPTH_32F, 1, 2, o),
                 "count": (fake_ctx, fake_hist, f, _lib.DEPTH_32F, 0, 0, o), "flow is not aligned": (fake_ctx, fake_hist, f4, _lib.DEPTH_64F, 1, 0, o),
                 "out is not aligned": (fake_ctx, fake_hist, f, _lib.DEPTH_32F, 1, 0, o4)}
        for what, args in calls.items():
            assert fn(*args) == _lib.MAV_ERR_ARG, (name, what)
            msg = lib.mav_last_error()
            assert name.encode() in msg and what.encode() in msg, (name, what, msg)
        assert fn(fake_ctx, fake_hist, f, _lib.DEPTH_32F, -3, 1, o) == _lib.MAV_ERR_ARG
    # the stage hook
    for args in ((None, ptr(flow), _lib.DEPTH_64F, ptr(mx), ptr(mx), ptr(out)), (fake_ctx, None, _lib.DEPTH_64F, ptr(mx), ptr(mx), ptr(out)),
                 (fake_ctx, ptr(flow), _lib.DEPTH_64F, None, ptr(mx), ptr(out)), (fake_ctx, ptr(flow), _lib.DEPTH_64F, ptr(mx), ptr(mx), None),
                 (fake_ctx, ptr(flow), _lib.DEPTH_8U, ptr(mx), ptr(mx), ptr(out))):
        assert lib.mav_stage_remap_linear(*args) == _lib.MAV_ERR_ARG
        assert b"mav_stage_remap_linear" in lib.mav_last_error()
    assert np.all(out == CANARY)


def test_python_layer_refuses_what_the_library_would(mav):
    from mavflow import _lib
    assert _lib.HISTORY_DEPTHS == {np.dtype(np.float32): 5, np.dtype(np.float64): 6}
    assert set(_lib.HISTORY_AXES) == {"reference", "xy"} and set(_lib.HISTORY_OUTS) == {"reference", "flow"}
    for member in ("push", "push_enqueue", "reset", "close", "index", "pushes"):
        assert hasattr(_lib.FlowHistory, member), member
    assert hasattr(_lib.Context, "flow_history") and hasattr(_lib.Context, "stage_remap_linear")
    from mavflow.detector import Detector
    assert hasattr(Detector, "get_history") and isinstance(Detector.history_index, property)
