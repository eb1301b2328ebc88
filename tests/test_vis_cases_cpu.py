"""The case table of the flow pictures (tests/vis_cases.py) held to the library: mav_vis_form, a pure host function, gives the form the
table names for every case, and every form and feature of the pixel passes is reached by some case.  And the C boundary of
include/mavflow_vis.h: the header declares and the cross-compiled library exports exactly mavflow.vis.EXPORTS, none of them in another
header; the build rule keeps the float32 arithmetic the header promises.  No GPU."""
import os
import re

import numpy as np
import pytest

import vis_cases as vc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mavflow_vis.h")
BASE = 0x7F0000001000                              # a 16-aligned address no call dereferences


@pytest.mark.parametrize("case", vc.CASES, ids=vc.case_id)
def test_mav_vis_form_follows_the_table(mav, case):
    from mavflow import vis
    flow, bgr, hsv = BASE, BASE + 0x100000 + case.offset, BASE + 0x200000 + case.offset
    assert vis.vis_form(case.W, case.H, case.batch, flow, bgr, hsv) == case.form
    assert vis.vis_form(case.W, case.H, case.batch, flow, bgr, None) == case.form          # a NULL hsv constrains nothing
    assert vc.form_of(case.W, case.H, case.batch, flow, bgr, hsv) == case.form
    if case.form == vc.FORM_FAST:
        assert vis.vis_form(case.W, case.H, case.batch, flow + 4, bgr, None) == vc.FORM_BYTES     # a flow aligned to its floats alone
        assert vis.vis_form(case.W, case.H, case.batch, None, bgr, hsv + 8) == vc.FORM_BYTES


def test_every_form_and_feature_is_reached_by_a_case():
    for name, holds in vc.FEATURES.items():
        assert any(holds(c) for c in vc.CASES), f"no case reaches: {name}"
    assert {(c.W, c.H) for c in vc.CASES} == set(vc.FRAMES) and {c.batch for c in vc.CASES} == {1, 3}
    assert (131 * 3) % 2 == 1                      # the rows of the 131-wide pictures start at odd addresses


def test_mav_vis_form_of_degenerate_sizes(mav):
    from mavflow import vis
    assert vis.vis_form(0, 5, 1) == -1 and vis.vis_form(5, 5, 0) == -1
    assert vis.vis_form(4, 4, 1) == vc.FORM_FAST and vis.vis_form(5, 3, 1) == vc.FORM_BYTES            # 16 and 15 pixels
    assert vis.FORM_FAST == vc.FORM_FAST and vis.FORM_BYTES == vc.FORM_BYTES


def test_header_and_library_agree(mav):
    from mavflow import _lib, vis
    txt = open(HEADER).read()
    declared = re.findall(r"\bint\s+(mav_\w+)\s*\(", txt)
    assert sorted(declared) == sorted(vis.EXPORTS) and len(declared) == 7
    lib = vis.load()
    for s in vis.EXPORTS:
        assert hasattr(lib, s), s
        assert s not in _lib.EXPORTS
    for s in vis.EXPORTS[:6]:
        assert (s + "_dev" in vis.EXPORTS) != s.endswith("_dev")            # a host form and a _dev form each
    inc = os.path.join(ROOT, "include")
    for other in sorted(os.listdir(inc)):
        if other != "mavflow_vis.h":
            assert not re.search(r"mav_flow_hsv|mav_cvt_color|mav_draw_flow|mav_vis_form|MAV_HSV_|MAV_COLOR_", open(os.path.join(inc, other)).read()), other
    for name, value in (("MAV_HSV_PROCESS", vis.HSV_PROCESS), ("MAV_HSV_DRAW", vis.HSV_DRAW), ("MAV_COLOR_BGR2HSV", 40), ("MAV_COLOR_HSV2BGR", 54),
                        ("MAV_COLOR_BGR2RADIAL", vis.COLOR_BGR2RADIAL), ("MAV_VIS_FORM_BYTES", 0), ("MAV_VIS_FORM_FAST", 1)):
        assert re.search(rf"#define\s+{name}\s+{value}\b", txt), name
    assert vis.RECORD_DTYPE.names == ("mag_min", "mag_max", "nonzero", "invalid") and vis.RECORD_DTYPE.itemsize == 16


def test_the_build_rule_keeps_ieee_float32():
    mk = open(os.path.join(ROOT, "mav-detection_amd", "csrc", "Makefile")).read()
    rule = mk[mk.index("$(BUILD)/kernels_vis.o:"):].split("\n")
    assert "kernels_vis.hip" in rule[0] and "-ffp-contract=off" in rule[2]
    assert "fast-math" not in mk and "-fno-hip-fp32-correctly-rounded-divide-sqrt" not in mk
    assert mk.count("$(BUILD)/kernels_vis.o") == 4                  # its own rule, libmavflow.so, the diag and variant link lines


def test_python_refusals_without_a_device():
    from mavflow import vis
    with pytest.raises(NotImplementedError, match="COLOR_BGR2HSV"):
        vis.cvtColor(np.zeros((4, 4, 3), np.uint8), 4)                       # COLOR_BGR2RGB: not built, named before any context is made
    with pytest.raises(NotImplementedError):
        vis.cvtColor(np.zeros((4, 4), np.uint8), vis.COLOR_HSV2BGR)
    with pytest.raises(ValueError):
        vis._mode("hsv")
