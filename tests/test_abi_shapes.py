"""The C boundary of include/mavflow_shapes.h: the header declares and the cross-compiled library exports every entry point of
_lib.SHAPES_EXPORTS, each is bound in _lib.py, the record is 32 bytes, the pure functions answer without a GPU, and the shims refuse from
their arguments alone what is not built.  Runs without a GPU."""
import ctypes as C
import logging
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mavflow_shapes.h")


def test_header_declares_library_exports_and_lib_binds_the_symbols(mav):
    from mavflow import _lib, shapes
    raw = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = re.findall(r"\b(mav_[a-z0-9_]+)\s*\(", txt)
    assert sorted(declared) == sorted(_lib.SHAPES_EXPORTS) and len(declared) == 11 and shapes.EXPORTS is _lib.SHAPES_EXPORTS
    lib = _lib.load()
    for s in _lib.SHAPES_EXPORTS:
        assert hasattr(lib, s), f"libmavflow.so does not export {s}"
        assert s not in _lib.EXPORTS                                   # include/mavflow.h's list stays what it was
        assert getattr(lib, s).argtypes is not None, f"{s} is not bound in _lib.py"
    for s in ("mav_draw_shapes", "mav_add_saturate", "mav_mosaic"):
        assert s + "_dev" in _lib.SHAPES_EXPORTS
    for other in os.listdir(os.path.join(ROOT, "include")):
        if other != "mavflow_shapes.h":
            main = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", other)).read(), flags=re.S)
            assert not re.search(r"mav_draw_shapes|mav_mosaic|mav_add_saturate|mav_shape\b", main), other
    for phrase in ('#include "mavflow.h"', "pinned to no cv2 build", "What to re-check first against a cv2 build", "odd-thickness half-width",
                   "outline pass", "three\n *   pixels wide", "A refused call has enqueued and written nothing", "is SKIPPED", "truncated toward zero"):
        assert phrase in raw, phrase
    for member in ("draw_shapes", "draw_shapes_enqueue", "draw_blob_boxes", "mosaic", "mosaic_enqueue", "add_saturate", "add_saturate_enqueue"):
        assert hasattr(_lib.Context, member), member
    mk = open(os.path.join(ROOT, "mav-detection_amd", "csrc", "Makefile")).read()
    assert mk.count("$(BUILD)/kernels_shapes.o") == 4                  # its own rule, libmavflow.so, the diag and variant link lines
    assert shapes.SHAPE_DTYPE.itemsize == 32 and [shapes.SHAPE_DTYPE.fields[k][1] for k in ("kind", "image", "x0", "y0", "x1", "y1", "thickness", "colour")] \
        == [0, 4, 8, 12, 16, 20, 24, 28]
    import mavflow
    assert mavflow.shapes is shapes


def test_null_context_calls_are_refused_by_name(mav):
    from mavflow import _lib
    lib = _lib.load()
    buf = np.zeros(64, np.uint8)
    p = buf.ctypes.data_as(C.c_void_p)
    calls = (("mav_draw_shapes", lambda: lib.mav_draw_shapes(None, p, 3, 1, p, 1)),
             ("mav_draw_shapes_dev", lambda: lib.mav_draw_shapes_dev(None, p, 3, 1, p, 1, None, None)),
             ("mav_add_saturate", lambda: lib.mav_add_saturate(None, p, p, 3, 1, p)),
             ("mav_add_saturate_dev", lambda: lib.mav_add_saturate_dev(None, p, p, 3, 1, p)),
             ("mav_mosaic", lambda: lib.mav_mosaic(None, p, p, 1, 1, 1, p)), ("mav_mosaic_dev", lambda: lib.mav_mosaic_dev(None, p, p, 1, 1, 1, p)),
             ("mav_shapes_from_blobs_dev", lambda: lib.mav_shapes_from_blobs_dev(None, p, p, 1, 1, 1, p, p, p)),
             ("mav_motion_pictures_dev", lambda: lib.mav_motion_pictures_dev(None, p, 1, p, p, p, p)))
    for name, call in calls:
        assert call() == _lib.MAV_ERR_ARG and lib.mav_last_error().decode().startswith(name + ":"), name
    assert not buf.any()


def test_cv2_signatures_refuse_what_is_not_built():
    from mavflow import shapes
    img = np.zeros((33, 66, 3), np.uint8)
    with pytest.raises(NotImplementedError, match="LINE_AA"):
        shapes.line(img, (1, 1), (9, 9), (0, 0, 255), 2, shapes.LINE_AA)
    with pytest.raises(NotImplementedError, match="LINE_AA"):
        shapes.rectangle(img, (1, 1), (9, 9), (0, 0, 255), 2, lineType=shapes.LINE_AA)
    with pytest.raises(NotImplementedError, match="shift"):
        shapes.line(img, (1, 1), (9, 9), (0, 0, 255), 2, shapes.LINE_8, 3)
    with pytest.raises(NotImplementedError, match="outlined circle"):
        shapes.circle(img, (9, 9), 4, (0, 0, 255), 1)
    with pytest.raises(NotImplementedError, match="outlined circle"):
        shapes.circle(img, (9, 9), 4, (0, 0, 255))
    with pytest.raises(ValueError, match="thickness"):
        shapes.line(img, (1, 1), (9, 9), (0, 0, 255), 0)
    with pytest.raises(ValueError, match="thickness"):
        shapes.rectangle(img, (1, 1), (9, 9), (0, 0, 255), 256)
    with pytest.raises(ValueError, match="radius"):
        shapes.circle(img, (9, 9), -1, (0, 0, 255), -1)
    with pytest.raises(TypeError, match="pt2"):
        shapes.line(img, (1, 1), (9.5, 9), (0, 0, 255), 2)
    with pytest.raises(NotImplementedError, match="uint8"):
        shapes.line(img.astype(np.float32), (1, 1), (9, 9), (0, 0, 255), 2)
    with pytest.raises(NotImplementedError, match="mask"):
        shapes.add(img, img, mask=img[..., 0])
    with pytest.raises(NotImplementedError, match="one shape"):
        shapes.add(img, img[:-1])
    with pytest.raises(ValueError, match="color"):
        shapes.line(img, (1, 1), (9, 9), (0, 0, float("nan")), 2)
    assert not img.any()
    assert shapes.shape(shapes.LINE, 1, 2, 3, 4, 5, (300, -4, 7.6))[-1] == (255, 0, 8, 0)      # cv2's saturation of a scalar


def _processor(**kw):
    from mavflow.detector import Detector
    from mavflow.processor import Processor, SyntheticDataset
    from mavflow.run_config import RunConfig
    ds = SyntheticDataset(W=96, H=80, N=3, use_farneback=False)
    cfg = RunConfig(logging.getLogger("t"), ds, "", False, False, False, True, False, False, "FLOW_FOE_CLUSTERING")
    return Processor(cfg, algorithm=Detector.Algorithm.HOMOGRAPHY, **kw)


def test_debug_mode_alone_still_raises_and_debug_path_refuses_the_batched_loop(mav, tmp_path):
    p = _processor()
    assert p.debug_path is None
    p.debug_mode = True
    with pytest.raises(NotImplementedError, match="debug"):
        p.run_detection()
    with pytest.raises(NotImplementedError, match="debug"):
        p.run_detection_batched(2)
    p = _processor(debug_path=str(tmp_path / "dbg"))
    with pytest.raises(NotImplementedError, match="debug_path"):
        p.run_detection_batched(2)
    assert p.detection_results == {} and not os.path.exists(str(tmp_path / "dbg"))


def test_line_colours_follow_the_reference_arithmetic_on_zero_denominators():
    from mavflow.focus_of_expansion import FocusOfExpansion
    t = np.cos(np.deg2rad(15))
    G, R = [0, 255, 0], [0, 0, 255]
    i32, u16 = np.int32, np.uint16
    lines = [((i32(50), i32(40)), (u16(40), u16(40))),      # points away from the FoE along the ray: cosine 1 -> green
             ((i32(50), i32(40)), (u16(60), u16(40))),      # toward it: cosine -1 -> red
             ((i32(50), i32(40)), (u16(50), u16(30))),      # across: cosine 0 -> red
             ((i32(50), i32(40)), (u16(50), u16(40))),      # zero-length line: 0 / 0 -> NaN -> green
             ((i32(30), i32(40)), (u16(20), u16(40))),      # newest point ON the FoE: 0 / 0 -> green
             ((i32(30), i32(40)), (u16(30), u16(40))),      # both
             ((i32(5), i32(40)), (u16(65535), u16(40)))]    # a wrapped end (the reference's uint16): int32 - uint16 stays exact
    got = FocusOfExpansion.line_colours(lines, (30.0, 40.0), t)
    assert got == [G, R, R, G, G, G, G]
    # the same decisions from the formula written out in float64
    for (p, q), c in zip(lines, got):
        d1 = np.array([float(p[0]) - float(q[0]), float(p[1]) - float(q[1])])
        d2 = np.array([float(p[0]) - 30.0, float(p[1]) - 40.0])
        den = np.hypot(*d1) * np.hypot(*d2)
        cos = np.nan if den == 0 else d1.dot(d2) / den
        assert c == (R if cos < t else G)
    assert FocusOfExpansion.line_colours([], (1.0, 2.0), t) == []
