"""The processed.mp4 frame at the drop-in boundary (no GPU): include/mavflow.h declares mav_overlay / mav_overlay_dev /
mav_last_overlay, libmavflow.so exports them, the binding lists them, and the Python surface carries them."""
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mav_overlay", "mav_overlay_dev", "mav_last_overlay")


def test_overlay_symbols_are_declared_exported_and_bound(mav):
    from mavflow import _lib
    txt = open(os.path.join(ROOT, "include", "mavflow.h")).read()
    assert "#define MAV_OVERLAY_MAX_RADIUS 4096" in txt
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(mav_[a-z0-9_]+)\s*\(", code))
    lib = _lib.load()
    for name in NAMES:
        assert name in declared, name
        assert name in _lib.EXPORTS, name
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes, name


def test_python_surface(mav):
    from mavflow import _lib
    from mavflow.focus_of_expansion import FocusOfExpansion
    from mavflow.processor import Processor
    for name in ("overlay", "overlay_last", "overlay_dev"):
        assert callable(getattr(_lib.Context, name)), name
    sig = inspect.signature(FocusOfExpansion.draw_FoE).parameters
    assert sig["color"].default == [0, 42, 255] and sig["radius"].default == 10
    assert inspect.signature(Processor).parameters["processed_path"].default is None
