"""The C boundary of the global-motion branch: mav_motion_result's layout against include/mavflow.h (CPU), and the argument checks
of the new entry points (GPU: they need a context)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_motion_result_layout_matches_the_header(mav, tmp_path):
    from mavflow import _lib
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc is not None, "a C compiler is needed to read the header's layout"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mavflow.h"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(mav_motion_result));']
    for name, _ in _lib.MotionResult._fields_:
        lines.append(f'  printf("{name} %zu\\n", offsetof(mav_motion_result, {name}));')
    lines.append('  printf("iters %d\\n", MAV_HOMOGRAPHY_LM_ITERATIONS); printf("pairs %d\\n", MAV_HOMOGRAPHY_MAX_PAIRS);')
    lines.append("  return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = {k: int(v) for k, v in (line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())}
    assert got["size"] == C.sizeof(_lib.MotionResult) == _lib.MOTION_DTYPE.itemsize == 88
    for name, _ in _lib.MotionResult._fields_:
        assert got[name] == getattr(_lib.MotionResult, name).offset == _lib.MOTION_DTYPE.fields[name][1], name
    assert got["pairs"] == _lib.HOMOGRAPHY_MAX_PAIRS
    import global_motion_ref as R
    assert got["iters"] == R.LM_ITERATIONS


@pytest.mark.gpu
def test_bad_arguments():
    from mavflow import _lib
    W, H = 96, 80
    lib = _lib.load()
    flow = np.zeros((1, H, W, 2), np.float32)
    M = np.array([[[1.0, 0, 0], [0, 1.0, 0]]])
    res = np.empty(1, _lib.MOTION_DTYPE)
    Hm, ok = np.empty(9), np.empty(1, np.int32)
    pts = np.arange(16.0).reshape(8, 2) ** 2
    coords = np.array([[5, 5], [90, 7], [50, 70], [8, 60]], np.int32)
    p = _lib._ptr
    with _lib.Context(W, H, 1) as ctx:
        h = ctx.h
        A = _lib.MAV_ERR_ARG
        assert lib.mav_global_motion(None, p(flow), p(M), 1, 1.5, 0, None, None, None, p(res)) == A
        assert lib.mav_global_motion(h, None, p(M), 1, 1.5, 0, None, None, None, p(res)) == A
        assert lib.mav_global_motion(h, p(flow), None, 1, 1.5, 0, None, None, None, p(res)) == A
        assert lib.mav_global_motion(h, p(flow), p(M), 1, 1.5, 0, None, None, None, None) == A
        assert lib.mav_global_motion(h, p(flow), p(M), 2, 1.5, 0, None, None, None, p(res)) == A          # batch > max_batch
        assert lib.mav_global_motion(h, p(flow), p(M), 1, 1.0, 0, None, None, None, p(res)) == A          # scale <= 1
        assert lib.mav_global_motion(h, p(flow), p(M), 1, 2.0, 0, None, None, None, p(res)) == A          # 96x80 -> 48x40: integer ratio
        assert b"integer ratio" in lib.mav_last_error()
        assert lib.mav_find_homography(h, p(pts), p(pts), 3, 1, p(Hm), p(ok)) == A                            # fewer than 4 pairs
        assert lib.mav_find_homography(h, p(pts), p(pts), _lib.HOMOGRAPHY_MAX_PAIRS + 1, 1, p(Hm), p(ok)) == A
        assert lib.mav_find_homography(h, None, p(pts), 8, 1, p(Hm), p(ok)) == A
        assert lib.mav_find_homography(h, p(pts), p(pts), 8, 1, p(Hm), None) == A
        assert lib.mav_flow_homography(h, p(flow), None, 4, 1, p(Hm), p(ok), None) == A
        outside = coords.copy()
        outside[2] = (W, 3)
        assert lib.mav_flow_homography(h, p(flow), p(outside), 4, 1, p(Hm), p(ok), None) == A and b"outside" in lib.mav_last_error()
        assert lib.mav_global_motion_step_dev(h, None, p(coords), 4, 1, 1.5, 0, None, None, None, None) == A
        # nothing resident yet / a batch that differs / after another host call
        assert lib.mav_last_global_motion_render(None, 1, None, None) == A
        img = np.empty((1, H, W, 3), np.uint8)
        assert lib.mav_last_global_motion_render(ctx.h, 1, p(img), None) == _lib.MAV_ERR_STATE
        ctx.global_motion(flow, M)
        assert lib.mav_last_global_motion_render(ctx.h, 2, p(img), None) == _lib.MAV_ERR_STATE
        assert lib.mav_last_global_motion_render(ctx.h, 1, p(img), None) == _lib.MAV_OK
        assert lib.mav_last_global_motion_render(ctx.h, 1, None, None) == _lib.MAV_OK
        ctx.bbox(np.zeros((H, W), np.uint8))
        assert lib.mav_last_global_motion_render(ctx.h, 1, p(img), None) == _lib.MAV_ERR_STATE
        with pytest.raises(ValueError):
            ctx.global_motion(flow, M, outputs=("nope",))
        with pytest.raises(ValueError):
            ctx.flow_homography(flow, coords.astype(np.float64))
