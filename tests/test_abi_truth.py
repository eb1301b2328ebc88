"""The C boundary of include/mavflow_truth.h: the header declares and the cross-compiled library exports every entry point of
mavflow._truth.EXPORTS, the layout of mav_gt_flow_params matches its Python mirrors (a small C program compiled against the header, here
and now), and calls that must be refused are refused with MAV_ERR_ARG, the function's name in the message and the outputs untouched --
whatever the arguments alone decide, before the context is looked at.  Runs without a GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mavflow_truth.h")
CANARY = 0x5A5A5A5A5A5A5A5A


def test_header_declares_and_library_exports_the_symbols(mav):
    from mavflow import _lib, _truth
    raw = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = re.findall(r"\b(mav_[a-z0-9_]+)\s*\(", txt)
    assert sorted(declared) == sorted(_truth.EXPORTS)
    lib = _truth.load()
    for s in _truth.EXPORTS:
        assert hasattr(lib, s), f"libmavflow.so does not export {s}"
        assert s not in _lib.EXPORTS                       # include/mavflow.h's list stays what it was
    main = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mavflow.h")).read(), flags=re.S)
    assert not any(re.search(rf"\b{s}\s*\(", main) for s in _truth.EXPORTS)
    for phrase in ('#include "mavflow.h"', "true division", "the product in float32", "0x7FF8000000000000", "numpy.histogram2d's rule",
                   "ADDS into it", "inverted by the caller"):
        assert phrase in raw, phrase
    for member in ("gt_flow", "gt_flow_enqueue", "radial_error_hist", "radial_error_accumulator"):
        assert hasattr(_lib.Context, member), member
    for member in ("add", "add_enqueue", "counts", "reset", "close"):
        assert hasattr(_truth.RadialErrorAccumulator, member), member


def test_layout_and_constants_match_the_header(mav, tmp_path):
    from mavflow import _lib, _truth
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc is not None, "a C compiler is needed to read the header's layout"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mavflow_truth.h"', "int main(void) {",
             '  printf("mav_gt_flow_params %zu\\n", sizeof(mav_gt_flow_params));']
    for name, _ in _truth.GtFlowParams._fields_:
        lines.append(f'  printf("mav_gt_flow_params.{name} %zu\\n", offsetof(mav_gt_flow_params, {name}));')
    for macro in ("MAV_RADIAL_MAX_EDGES", "MAV_RADIAL_MAX_CELLS", "MAV_RADIAL_TABLE_WORDS(159, 159)", "MAV_DEPTH_32F", "MAV_DEPTH_64F"):
        lines.append(f'  printf("{macro.replace(" ", "")} %d\\n", (int)({macro}));')
    lines.append('  printf("step %zu\\n", sizeof(mav_frame_step));')
    lines.append("  return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = {k: int(v) for k, v in (line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())}
    assert got["mav_gt_flow_params"] == C.sizeof(_truth.GtFlowParams) == _truth.GT_FLOW_PARAMS_DTYPE.itemsize == 288
    for name, _ in _truth.GtFlowParams._fields_:
        assert got[f"mav_gt_flow_params.{name}"] == getattr(_truth.GtFlowParams, name).offset == _truth.GT_FLOW_PARAMS_DTYPE.fields[name][1], name
    assert (got["MAV_RADIAL_MAX_EDGES"], got["MAV_RADIAL_MAX_CELLS"]) == (_truth.RADIAL_MAX_EDGES, _truth.RADIAL_MAX_CELLS) == (257, 65536)
    assert got["MAV_RADIAL_TABLE_WORDS(159,159)"] == _truth.table_words(159, 159) == 25283
    assert (got["MAV_DEPTH_32F"], got["MAV_DEPTH_64F"]) == (_lib.DEPTH_32F, _lib.DEPTH_64F) == (5, 6)
    assert got["step"] == C.sizeof(_lib.FrameStep) == 488                   # nothing was added to the loop's struct
    internal = open(os.path.join(ROOT, "mav-detection_amd", "csrc", "mavflow_internal.h")).read()
    assert "struct RadialEdges { int n, pad; double e[257]; };" in internal       # the by-value list holds MAV_RADIAL_MAX_EDGES


def _params(flags=0):
    from mavflow import _truth
    p = _truth.gt_flow_params(np.eye(4), np.eye(4), (0.0, 0.0, 0.0), 1.0, 1)
    p["flags"] = flags
    return p


def test_refused_gt_flow_calls_leave_the_output_untouched(mav):
    from mavflow import _lib, _truth
    lib, ptr = _truth.load(), _lib._ptr
    depth, seg = np.ones((4, 4), np.float32), np.zeros((4, 4), np.uint8)
    out = np.full(4 * 4 * 2 + 8, CANARY, np.uint64)
    fake_ctx = C.c_void_p(C.addressof(C.create_string_buffer(64)))          # a handle that must never be dereferenced
    good = _params()
    d, s, p, o = ptr(depth), ptr(seg), ptr(good), ptr(out)
    off = lambda v, n: C.c_void_p(v.value + n)
    for name in ("mav_gt_flow", "mav_gt_flow_dev"):
        fn = getattr(lib, name)
        calls = {"NULL context": (None, d, s, p, 1, _lib.DEPTH_32F, o), "NULL depth": (fake_ctx, None, s, p, 1, _lib.DEPTH_32F, o),
                 "NULL params": (fake_ctx, d, s, None, 1, _lib.DEPTH_32F, o), "NULL flow": (fake_ctx, d, s, p, 1, _lib.DEPTH_32F, None),
                 "out_depth": (fake_ctx, d, s, p, 1, _lib.DEPTH_8U, o), "batch 0": (fake_ctx, d, s, p, 0, _lib.DEPTH_64F, o),
                 "batch -3": (fake_ctx, d, s, p, -3, _lib.DEPTH_64F, o)}
        if name.endswith("_dev"):
            calls.update({"depth is not aligned": (fake_ctx, off(d, 2), s, p, 1, _lib.DEPTH_32F, o),
                          "params is not aligned": (fake_ctx, d, s, off(p, 4), 1, _lib.DEPTH_32F, o),
                          "flow is not aligned": (fake_ctx, d, s, p, 1, _lib.DEPTH_32F, off(o, 4)),
                          "flow is not aligned to its 16": (fake_ctx, d, s, p, 1, _lib.DEPTH_64F, off(o, 8))})
        else:
            calls["flags"] = (fake_ctx, d, s, ptr(_params(flags=1)), 1, _lib.DEPTH_32F, o)
        for what, args in calls.items():
            assert fn(*args) == _lib.MAV_ERR_ARG, (name, what)
            msg = lib.mav_last_error()
            assert name.encode() + b":" in msg and what.split(" ")[0].encode() in msg, (name, what, msg)
    assert np.all(out == CANARY)


def test_refused_histogram_calls_leave_the_table_untouched(mav):
    from mavflow import _lib, _truth
    lib, ptr = _truth.load(), _lib._ptr
    flow, gt, sky = np.ones((4, 4, 2), np.float32), np.ones((4, 4, 2), np.float32), np.zeros((4, 4), np.uint8)
    table = np.full(_truth.table_words(256, 256) + 8, CANARY, np.uint64)
    fake_ctx = C.c_void_p(C.addressof(C.create_string_buffer(64)))
    em, ee = np.linspace(0, 10, 160), np.linspace(-20, 20, 160)
    f, g, s, t = ptr(flow), ptr(gt), ptr(sky), ptr(table)
    off = lambda v, n: C.c_void_p(v.value + n)
    bad_lists = {"not strictly increasing": np.array([0.0, 2.0, 1.0, 3.0]), "strictly increasing at [2]": np.array([0.0, 1.0, 1.0, 3.0]),
                 "not finite": np.array([0.0, np.nan, 2.0]), "is not finite": np.array([0.0, 1.0, np.inf]), "outside [2, 257]": np.array([1.0]),
                 "258": np.linspace(0, 1, 258)}
    for name in ("mav_radial_error_hist", "mav_radial_error_hist_dev"):
        fn = getattr(lib, name)
        ok = (fake_ctx, f, g, s, 1, ptr(em), em.size, ptr(ee), ee.size, t)
        calls = {"NULL context": (None,) + ok[1:], "NULL flow": ok[:1] + (None,) + ok[2:], "NULL gt_flow": ok[:2] + (None,) + ok[3:],
                 "NULL table": ok[:9] + (None,), "NULL mag_edges": ok[:5] + (None,) + ok[6:], "NULL err_edges": ok[:7] + (None,) + ok[8:],
                 "batch 0": ok[:4] + (0,) + ok[5:], "batch -1": ok[:4] + (-1,) + ok[5:],
                 "0 mag_edges": ok[:6] + (0,) + ok[7:], "1 err_edges": ok[:8] + (1,) + ok[9:]}
        for what, lst in bad_lists.items():
            calls[f"mag {what}"] = ok[:5] + (ptr(lst), lst.size) + ok[7:]
            calls[f"err {what}"] = ok[:7] + (ptr(lst), lst.size) + ok[9:]
        if name.endswith("_dev"):
            calls.update({"flow is not aligned": ok[:1] + (off(f, 4),) + ok[2:], "gt_flow is not aligned": ok[:2] + (off(g, 4),) + ok[3:],
                          "table is not aligned": ok[:9] + (off(t, 4),)})
        for what, args in calls.items():
            assert fn(*args) == _lib.MAV_ERR_ARG, (name, what)
            msg = lib.mav_last_error()
            assert name.encode() + b":" in msg, (name, what, msg)
    assert np.all(table == CANARY)
    # (more than MAV_RADIAL_MAX_CELLS cells cannot be reached by two accepted lists -- 257 edges each give exactly 256 x 256 -- so that
    # refusal has no case here; tests/test_gpu_radial_hist.py runs lists of 257 and 256 edges)


def test_python_layer_refuses_what_would_round(mav):
    from mavflow import _lib, _truth
    import pytest
    ctx = object.__new__(_lib.Context)                                      # no device: the checks come before any call
    ctx.W, ctx.H = 4, 4
    with pytest.raises(TypeError):
        _lib.Context.gt_flow(ctx, np.ones((4, 4), np.float64), None, np.eye(4), np.eye(4), (0, 0, 0))
    with pytest.raises(ValueError):
        _lib.Context.gt_flow(ctx, np.ones((4, 4), np.float32), None, np.eye(4), np.eye(4), (0, 0, 0), dtype=np.float16)
    with pytest.raises(TypeError):
        _lib.Context.radial_error_hist(ctx, np.ones((4, 4, 2), np.float64), np.ones((4, 4, 2), np.float32), None)
    p = _truth.gt_flow_params(np.arange(16.0).reshape(4, 4), np.eye(4), (1, 2, 3), 100.0, 2)
    assert p.shape == (2,) and p["view_proj_prev"][1][6] == 6.0 and p["depth_scale"][0] == np.float32(100) and not p["flags"].any()
