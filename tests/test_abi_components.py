"""The C boundary of the connected components: the header declares and the cross-compiled library exports the new symbols, the
layouts of mav_blob / mav_cc_params / mav_cc_counts and the tile size match their Python mirrors (a small C program compiled against
include/mavflow.h, here and now), and calls without a context are refused.  Runs without a GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mav_cc_defaults", "mav_components", "mav_components_dev", "mav_last_masks_components")


def test_header_declares_and_library_exports_the_symbols(mav):
    from mavflow import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mavflow.h")).read(), flags=re.S)
    lib = _lib.load()
    for s in SYMBOLS:
        assert re.search(rf"\b{s}\s*\(", txt), f"include/mavflow.h does not declare {s}"
        assert hasattr(lib, s), f"libmavflow.so does not export {s}"
        assert s in _lib.EXPORTS
    assert "NOT promised to be cv2's" in open(os.path.join(ROOT, "include", "mavflow.h")).read()


def test_layouts_match_the_header(mav, tmp_path):
    from mavflow import _lib
    import components_ref as R
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc is not None, "a C compiler is needed to read the header's layout"
    mirrors = (("mav_blob", _lib.Blob), ("mav_cc_params", _lib.CcParams), ("mav_cc_counts", _lib.CcCounts))
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "mavflow.h"', "int main(void) {"]
    for cname, cls in mirrors:
        lines.append(f'  printf("{cname} %zu\\n", sizeof({cname}));')
        for name, _ in cls._fields_:
            lines.append(f'  printf("{cname}.{name} %zu\\n", offsetof({cname}, {name}));')
    for name in ("cc", "off_cc_counts", "off_cc_blobs", "record_done"):
        lines.append(f'  printf("step.{name} %zu\\n", offsetof(mav_frame_step, {name}));')
    lines.append('  printf("step %zu\\n", sizeof(mav_frame_step));')
    lines.append('  printf("tile_w %d\\n", MAV_CC_TILE_W); printf("tile_h %d\\n", MAV_CC_TILE_H); printf("max_blobs %d\\n", MAV_CC_MAX_BLOBS);')
    lines.append("  return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = {k: int(v) for k, v in (line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())}
    for cname, cls in mirrors:
        assert got[cname] == C.sizeof(cls), cname
        for name, _ in cls._fields_:
            assert got[f"{cname}.{name}"] == getattr(cls, name).offset, (cname, name)
    assert got["mav_blob"] == _lib.BLOB_DTYPE.itemsize == R.BLOB_DTYPE.itemsize == 40
    assert got["mav_cc_counts"] == _lib.CC_COUNTS_DTYPE.itemsize == R.COUNTS_DTYPE.itemsize == 8
    for name, _ in _lib.Blob._fields_:
        assert got[f"mav_blob.{name}"] == _lib.BLOB_DTYPE.fields[name][1] == R.BLOB_DTYPE.fields[name][1], name
    assert (got["tile_w"], got["tile_h"], got["max_blobs"]) == (_lib.CC_TILE_W, _lib.CC_TILE_H, _lib.CC_MAX_BLOBS)
    # the new step fields are the LAST ones, behind everything the struct had
    assert got["step.record_done"] < got["step.cc"] < got["step.off_cc_counts"] < got["step.off_cc_blobs"]
    assert got["step.off_cc_blobs"] + C.sizeof(C.c_size_t) == got["step"] == C.sizeof(_lib.FrameStep)
    assert [n for n, _ in _lib.FrameStep._fields_][-3:] == ["cc", "off_cc_counts", "off_cc_blobs"]
    assert bytes(_lib.FrameStep())[got["step.cc"]:] == bytes(got["step"] - got["step.cc"])       # a zeroed struct: cc off


def test_defaults_and_calls_without_a_context(mav):
    from mavflow import _lib
    lib = _lib.load()
    p = _lib.cc_defaults()
    assert (p.connectivity, p.min_area, p.max_blobs) == (8, 1, 256)
    lib.mav_cc_defaults(None)                                          # a NULL pointer is ignored, as the other *_defaults
    mask = np.ones((1, 4, 4), np.uint8)
    counts, table = np.zeros(1, _lib.CC_COUNTS_DTYPE), np.zeros((1, 256), _lib.BLOB_DTYPE)
    ptr = _lib._ptr
    for fn in (lib.mav_components, lib.mav_components_dev):
        assert fn(None, ptr(mask), 1, None, None, ptr(counts), ptr(table)) == _lib.MAV_ERR_ARG
        assert b"NULL" in lib.mav_last_error()
    assert lib.mav_last_masks_components(None, 0, 1, None, None, ptr(counts), ptr(table)) == _lib.MAV_ERR_ARG
    for bad in (dict(connectivity=6), dict(min_area=0), dict(max_blobs=0), dict(max_blobs=65536)):
        q = _lib.cc_defaults(**bad)
        assert lib.mav_components(None, ptr(mask), 1, C.byref(q), None, ptr(counts), ptr(table)) == _lib.MAV_ERR_ARG
    assert not table.view(np.uint8).any() and not counts.view(np.uint8).any()             # nothing was written
    import pytest
    with pytest.raises(ValueError):
        _lib.cc_defaults(nope=1)
