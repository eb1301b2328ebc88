"""The C boundary of the threshold sweep: the header declares and the cross-compiled library exports the four entry points, the layout
of mav_roc_params matches its Python mirror (a small C program compiled against include/mavflow.h, here and now), mav_frame_step is
what it was, and calls that must be refused are refused with the table untouched.  Runs without a GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np

import roc_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mav_roc_sweep", "mav_roc_sweep_dev", "mav_last_roc_sweep", "mav_roc_arm")
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
    for phrase in ("phi * gate > t equals gate && phi > t", "ROUNDED TO FLOAT32", "A NaN magnitude passes no gate", "are ignored"):
        assert phrase in raw, phrase


def test_layouts_match_the_header(mav, tmp_path):
    from mavflow import _lib
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc is not None, "a C compiler is needed to read the header's layout"
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mavflow.h"', "int main(void) {",
             '  printf("mav_roc_params %zu\\n", sizeof(mav_roc_params));']
    for name, _ in _lib.RocParams._fields_:
        lines.append(f'  printf("mav_roc_params.{name} %zu\\n", offsetof(mav_roc_params, {name}));')
    lines.append('  printf("step %zu\\n", sizeof(mav_frame_step)); printf("step.off_cc_blobs %zu\\n", offsetof(mav_frame_step, off_cc_blobs));')
    lines.append('  printf("max_angles %d\\n", MAV_ROC_MAX_ANGLES); printf("max_mags %d\\n", MAV_ROC_MAX_MAGS);')
    lines.append('  printf("words_1_1 %zu\\n", MAV_ROC_TABLE_WORDS(1, 1)); printf("words_max %zu\\n", MAV_ROC_TABLE_WORDS(64, 16));')
    lines.append("  return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = {k: int(v) for k, v in (line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())}
    assert got["mav_roc_params"] == C.sizeof(_lib.RocParams)
    for name, _ in _lib.RocParams._fields_:
        assert got[f"mav_roc_params.{name}"] == getattr(_lib.RocParams, name).offset, name
    assert (got["max_angles"], got["max_mags"]) == (_lib.ROC_MAX_ANGLES, _lib.ROC_MAX_MAGS) == (rc.MAX_ANGLES, rc.MAX_MAGS)
    assert got["words_1_1"] == _lib.roc_table_words(1, 1) == 4 and got["words_max"] == _lib.roc_table_words(64, 16) == 2050
    # mav_frame_step is what it was: the sweep is armed on the context, the struct is not extended
    assert got["step"] == C.sizeof(_lib.FrameStep) == 488
    assert got["step.off_cc_blobs"] + C.sizeof(C.c_size_t) == got["step"]
    assert [n for n, _ in _lib.FrameStep._fields_][-1] == "off_cc_blobs"


def test_expand_orders_the_table_as_tpr_fpr_counts():
    from mavflow import _lib
    ka, km = 3, 2
    t = np.arange(2 * _lib.roc_table_words(ka, km), dtype=np.int64).reshape(2, -1)
    e = _lib.roc_expand(t, ka, km)
    assert e.shape == (2, ka, km, 4)
    for b in range(2):
        for i in range(ka):
            for j in range(km):
                assert e[b, i, j].tolist() == [t[b, 0], t[b, 1], t[b, 2 + 2 * (i * km + j)], t[b, 3 + 2 * (i * km + j)]]


def test_refused_calls_leave_the_table_untouched(mav):
    from mavflow import _lib
    lib, ptr = _lib.load(), _lib._ptr
    W, H = 4, 4
    flow, foe, gt = np.zeros((1, H, W, 2), np.float32), np.zeros((1, 2)), np.zeros((1, H, W), np.uint8)
    table = np.full(_lib.roc_table_words(64, 16) + 8, CANARY, np.uint64)
    good, ga, gm = _lib.roc_params(rc.ANG, rc.MAG)

    def calls(ctx, p, arm=True):
        yield "mav_roc_sweep", lib.mav_roc_sweep(ctx, ptr(flow), ptr(foe), None, None, None, None, ptr(gt), 1, 1, None, p, ptr(table))
        yield "mav_roc_sweep_dev", lib.mav_roc_sweep_dev(ctx, ptr(flow), ptr(foe), None, None, None, None, ptr(gt), 1, 1, None, p, ptr(table))
        yield "mav_last_roc_sweep", lib.mav_last_roc_sweep(ctx, ptr(gt), 1, 1, p, ptr(table))
        if arm:
            yield "mav_roc_arm", lib.mav_roc_arm(ctx, p, 0)

    for name, rcode in calls(None, C.byref(good)):                                  # a NULL context
        assert rcode == _lib.MAV_ERR_ARG, name
        assert b"NULL" in lib.mav_last_error()
    assert lib.mav_roc_arm(None, None, 0) == _lib.MAV_ERR_ARG
    # a refused list is refused before the context is looked at: a (never dereferenced) non-NULL handle shows the order of the checks
    fake = C.c_void_p(C.addressof(C.create_string_buffer(64)))
    for bad, (a, m) in rc.BAD_LISTS.items():
        p, ka_, km_ = _lib.roc_params(a, m)
        for name, rcode in calls(fake, C.byref(p)):
            assert rcode == _lib.MAV_ERR_ARG, (bad, name)
            assert name.encode() in lib.mav_last_error(), (bad, name, lib.mav_last_error())
    for name, rcode in calls(fake, None, arm=False):                                # NULL parameters (for mav_roc_arm NULL means disarm)
        assert rcode == _lib.MAV_ERR_ARG, name
    nul = _lib.RocParams(2, 1, None, good.mags)                                     # a list pointer missing
    for name, rcode in calls(fake, C.byref(nul)):
        assert rcode == _lib.MAV_ERR_ARG, name
    assert np.all(table == CANARY)
