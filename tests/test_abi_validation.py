"""The C boundary of include/mavflow_validation.h: the header declares and the cross-compiled library exports every entry point of
mavflow._validation.EXPORTS (none of them in include/mavflow.h or _lib.EXPORTS), the layouts of mav_gt_stats_params and
mav_gt_stats_record match their Python mirrors (a small C program compiled against the header, here and now), and calls that must be
refused are refused with MAV_ERR_ARG, the function's name in the message and the outputs untouched -- whatever the arguments alone
decide, before the context is looked at.  Runs without a GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mavflow_validation.h")
CANARY = 0x5A5A5A5A5A5A5A5A


def test_header_declares_and_library_exports_the_symbols(mav):
    from mavflow import _lib, _validation
    raw = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = re.findall(r"\b(mav_gt_[a-z0-9_]+)\s*\(", txt)
    assert sorted(declared) == sorted(_validation.EXPORTS)
    lib = _validation.load()
    for s in _validation.EXPORTS:
        assert hasattr(lib, s), f"libmavflow.so does not export {s}"
        assert s not in _lib.EXPORTS                       # include/mavflow.h's list stays what it was
    main = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mavflow.h")).read(), flags=re.S)
    assert not any(re.search(rf"\b{s}\s*\(", main) for s in _validation.EXPORTS)
    for phrase in ('#include "mavflow.h"', "in raster order", "accumulated SEQUENTIALLY from 0.0", "value-based casting", "0x7FC00000",
                   "Only integer atomics are used"):
        assert phrase in raw, phrase
    for member in ("gt_stats", "gt_stats_enqueue"):
        assert hasattr(_lib.Context, member), member
    mk = open(os.path.join(ROOT, "mav-detection_amd", "csrc", "Makefile")).read()
    assert mk.count("$(BUILD)/kernels_validation.o") == 4          # its own rule, libmavflow.so, the diag and variant link lines
    rule = mk[mk.index("$(BUILD)/kernels_validation.o:"):]
    assert "-ffp-contract=off" in rule.split("\n")[2]


def test_layout_and_constants_match_the_header(mav, tmp_path):
    from mavflow import _lib, _validation as V
    import validation_ref as R
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc is not None, "a C compiler is needed to read the header's layout"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mavflow_validation.h"', "int main(void) {",
             '  printf("mav_gt_stats_params %zu\\n", sizeof(mav_gt_stats_params));', '  printf("mav_gt_stats_record %zu\\n", sizeof(mav_gt_stats_record));']
    for struct, mirror in (("mav_gt_stats_params", V.GtStatsParams), ("mav_gt_stats_record", V.GtStatsRecord)):
        for name, _ in mirror._fields_:
            lines.append(f'  printf("{struct}.{name} %zu\\n", offsetof({struct}, {name}));')
    for macro in ("MAV_GT_STATS_FRAME0", "MAV_GT_STATS_THR_F64", "MAV_GT_STATS_TRUNCATED", "MAV_GT_STATS_DEPTH_NAN", "MAV_GT_STATS_MAX_PIXELS"):
        lines.append(f'  printf("{macro} %d\\n", (int)({macro}));')
    lines.append('  printf("step %zu\\n", sizeof(mav_frame_step));')
    lines.append("  return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = {k: int(v) for k, v in (line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())}
    assert got["mav_gt_stats_params"] == C.sizeof(V.GtStatsParams) == V.PARAMS_DTYPE.itemsize == 56
    assert got["mav_gt_stats_record"] == C.sizeof(V.GtStatsRecord) == V.RECORD_DTYPE.itemsize == 96 and 96 % 16 == 0
    for struct, mirror, dtype in (("mav_gt_stats_params", V.GtStatsParams, V.PARAMS_DTYPE), ("mav_gt_stats_record", V.GtStatsRecord, V.RECORD_DTYPE)):
        for name, _ in mirror._fields_:
            assert got[f"{struct}.{name}"] == getattr(mirror, name).offset == dtype.fields[name][1], (struct, name)
    assert V.RECORD_DTYPE == R.RECORD_DTYPE                                  # the restatement's records are the library's
    end = max(off + dt.itemsize for dt, off in (V.RECORD_DTYPE.fields[n][:2] for n in V.RECORD_DTYPE.names))
    assert end == 96 and sum(V.RECORD_DTYPE.fields[n][0].itemsize for n in V.RECORD_DTYPE.names) == 96       # no padding inside or behind
    assert (got["MAV_GT_STATS_FRAME0"], got["MAV_GT_STATS_THR_F64"]) == (V.GT_STATS_FRAME0, V.GT_STATS_THR_F64) == (R.FRAME0, R.THR_F64) == (1, 2)
    assert (got["MAV_GT_STATS_TRUNCATED"], got["MAV_GT_STATS_DEPTH_NAN"]) == (V.GT_STATS_TRUNCATED, V.GT_STATS_DEPTH_NAN) == (R.TRUNCATED, R.DEPTH_NAN) == (1, 2)
    assert got["MAV_GT_STATS_MAX_PIXELS"] == V.GT_STATS_MAX_PIXELS == 1 << 20
    assert got["step"] == C.sizeof(_lib.FrameStep) == 488                   # nothing was added to the loop's struct


def test_defaults(mav):
    from mavflow import _validation as V
    p = V.GtStatsParams()
    p.pad = 7
    V.load().mav_gt_stats_defaults(C.byref(p))
    assert (list(p.omega), p.dt, p.box_fraction, p.seg_threshold, p.flags, p.pad) == ([0.0, 0.0, 0.0], 1.0, 0.1, 127, 0, 0)
    assert np.float32(p.depth_fraction) == np.float32(0.8)
    V.load().mav_gt_stats_defaults(None)                                    # harmless
    q = V.gt_stats_params(np.arange(6.0).reshape(2, 3), dt=(0.5, 0.25), frame0=(True, False), legacy_threshold=True)
    assert q.shape == (2,) and q["omega"][1][2] == 5.0 and list(q["dt"]) == [0.5, 0.25] and list(q["flags"]) == [3, 2]
    assert (q["box_fraction"] == 0.1).all() and (q["depth_fraction"] == np.float32(0.8)).all() and (q["seg_threshold"] == 127).all()


def test_refused_calls_leave_the_outputs_untouched(mav):
    from mavflow import _lib, _validation as V
    lib, ptr = V.load(), _lib._ptr
    seg, sky = np.zeros((4, 4), np.uint8), np.zeros((4, 4), np.uint8)
    gt, depth = np.ones((4, 4, 2), np.float32), np.ones((4, 4), np.float32)
    rec = np.full(96 // 8 * 2 + 8, CANARY, np.uint64)
    idx = np.full(64, CANARY, np.uint64)
    fake_ctx = C.c_void_p(C.addressof(C.create_string_buffer(64)))          # a handle that must never be dereferenced
    good = V.gt_stats_params()
    s, g, k, d, p, r, i = ptr(seg), ptr(gt), ptr(sky), ptr(depth), ptr(good), ptr(rec), ptr(idx)
    assert r.value % 16 == 0 and g.value % 8 == 0
    off = lambda v, n: C.c_void_p(v.value + n)

    def bad(**kw):
        q = V.gt_stats_params()
        for key, v in kw.items():
            q[key] = v
        return q

    for name in ("mav_gt_stats", "mav_gt_stats_dev"):
        fn = getattr(lib, name)
        ok = (fake_ctx, s, g, k, d, p, 1, 8, r, i)
        calls = {"NULL context": (None,) + ok[1:], "NULL seg": ok[:1] + (None,) + ok[2:], "NULL params": ok[:5] + (None,) + ok[6:],
                 "NULL records": ok[:8] + (None,) + ok[9:], "batch 0": ok[:6] + (0,) + ok[7:], "batch -2": ok[:6] + (-2,) + ok[7:],
                 "max_pixels 0": ok[:7] + (0,) + ok[8:], "max_pixels -1": ok[:7] + (-1,) + ok[8:], "max_pixels 1048577": ok[:7] + ((1 << 20) + 1,) + ok[8:]}
        keep = []
        if name.endswith("_dev"):
            calls.update({"depth is not aligned": ok[:4] + (off(d, 2),) + ok[5:], "gt_flow is not aligned": ok[:2] + (off(g, 4),) + ok[3:],
                          "params is not aligned": ok[:5] + (off(p, 4),) + ok[6:], "records is not aligned": ok[:8] + (off(r, 8),) + ok[9:],
                          "indices is not aligned": ok[:9] + (off(i, 2),)})
        else:
            for what, q in {"omega[1] is not finite": bad(omega=(0.0, np.nan, 0.0)), "omega[2] is not finite": bad(omega=(0.0, 0.0, np.inf)),
                            "dt is not finite": bad(dt=np.inf), "dt is 0": bad(dt=0.0), "flags 0x4": bad(flags=4), "flags 0x80000001": bad(flags=-0x7FFFFFFF)}.items():
                keep.append(q)
                calls[what] = ok[:5] + (ptr(q),) + ok[6:]
        for what, args in calls.items():
            assert fn(*args) == _lib.MAV_ERR_ARG, (name, what)
            msg = lib.mav_last_error()
            assert name.encode() + b":" in msg and what.split(" ")[0].encode() in msg, (name, what, msg)
    assert np.all(rec == CANARY) and np.all(idx == CANARY)
    # dt == 0 is what frame 0 passes: accepted with MAV_GT_STATS_FRAME0 (the next check is the context, which a NULL one fails)
    q = bad(dt=0.0, flags=V.GT_STATS_FRAME0)
    assert lib.mav_gt_stats(None, s, g, k, d, ptr(q), 1, 8, r, i) == _lib.MAV_ERR_ARG and b"NULL context" in lib.mav_last_error()


def test_python_layer_refuses_what_would_round(mav):
    from mavflow import _lib
    ctx = object.__new__(_lib.Context)                                      # no device: the checks come before any call
    ctx.W, ctx.H = 4, 4
    seg = np.zeros((4, 4), np.uint8)
    with pytest.raises(TypeError):
        _lib.Context.gt_stats(ctx, seg, gt_flow=np.ones((4, 4, 2), np.float64))
    with pytest.raises(TypeError):
        _lib.Context.gt_stats(ctx, seg, depth=np.ones((4, 4), np.float64))
    with pytest.raises(ValueError):
        _lib.Context.gt_stats(ctx, np.zeros((5, 4), np.uint8))
    with pytest.raises(ValueError):
        _lib.Context.gt_stats(ctx, np.zeros((2, 4, 4), np.uint8), depth=np.ones((3, 4, 4), np.float32))


def test_processor_validation_keyword(mav):
    import inspect
    from mavflow.processor import Processor
    params = list(inspect.signature(Processor.__init__).parameters.values())
    assert params[-1].name == "validation" and params[-1].default == "host"
    with pytest.raises(ValueError):
        Processor(None, validation="gpu")
