"""TEST INFRASTRUCTURE -- the case table of the image resize (include/mavflow_resize.h, csrc/kernels_resize.hip): the shapes, the inputs
and, for every kernel form (pixel format x form of cv::resize's dispatch x aligned or scalar store path, and the fused sky mask), the
smallest shapes that reach it.  tests/test_resize_cases_cpu.py holds the table to the forms the kernel file names and to a pure-Python
mirror of the host's dispatch (resize_ref.form_of / vector_stores), and fails when a form is no longer reached; tests/test_gpu_resize.py
runs the device on every run of the table."""
from __future__ import annotations

import os
import re
from collections import namedtuple

import numpy as np

import resize_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = os.path.join(ROOT, "mav-detection_amd", "csrc", "kernels_resize.hip")
INTERNAL = os.path.join(ROOT, "mav-detection_amd", "csrc", "mavflow_internal.h")
B = 3                                                      # max_batch of every context here; calls run at batch 1 and 3
FORMATS = {"U8C1": R.U8C1, "U8C3": R.U8C3, "F32C1": R.F32C1, "F32C2": R.F32C2}
INTERPS = {"nearest": R.NEAREST, "linear": R.LINEAR, "area": R.AREA}

Shape = namedtuple("Shape", "src dst why")                 # (sw, sh), (dw, dh)
SHAPES = [
    Shape((1, 1), (5, 3), "one-tap region everywhere"),
    Shape((2, 2), (7, 5), "smallest with two taps"),
    Shape((1, 9), (3, 30), "one source column"),
    Shape((13, 1), (40, 6), "one source row; a destination width that is a multiple of 4"),
    Shape((5, 3), (67, 4), "crosses a 64-lane row boundary with a ragged tail"),
    Shape((9, 2), (263, 3), "crosses the 64-lane row boundary of this kernel (4 or 2 pixels a lane) with a ragged tail"),
    Shape((33, 17), (65, 70), "general enlarging; more than one workgroup of rows; a zero weight inside the picture (column 32)"),
    Shape((64, 48), (37, 29), "linear shrink that is not 2x; general area"),
    Shape((64, 48), (32, 24), "linear to area; uint8 2 x 2; float32 fast 2 x 2"),
    Shape((63, 48), (21, 16), "area fast 3 x 3"),
    Shape((48, 20), (12, 10), "area fast 4 x 2 at a width that is a multiple of 4"),
    Shape((60, 45), (40, 30), "area general 1.5"),
    Shape((20, 12), (20, 12), "copy"),
]
FORMS = ("copy", "nearest", "linear", "area_2x2", "area_fast", "area_general")     # RS_* of mavflow_internal.h, in its order
SKY_FORMS = ("copy", "linear", "area_2x2")                                         # what INTER_LINEAR of a uint8 picture can become


def kernel_forms() -> set:
    """every (format, form, vector stores?, sky?) k_resize can be instantiated as"""
    out = set()
    for f, fmt in FORMATS.items():
        for form in FORMS:
            if form == "area_2x2" and R.FORMATS[fmt][0] != np.uint8:
                continue
            out |= {(f, form, v, False) for v in (False, True)}
    out |= {("U8C3", form, v, True) for form in SKY_FORMS for v in (False, True)}
    return out


def source_forms() -> dict:
    """what the sources name, read as text"""
    with open(KERNELS) as f:
        src = f.read()
    with open(INTERNAL) as f:
        internal = f.read()
    enum = re.search(r"enum \{ (RS_COPY[^}]*) \};", internal).group(1)
    return dict(enum=[e.strip()[3:].lower() for e in enum.split(",")], formats=set(re.findall(r"struct RsFmt<MAV_WARP_(\w+)>", src)),
                dispatched=set(re.findall(r"RS_GO\(RS_(\w+)\);", src)), text=src)


Run = namedtuple("Run", "fmt interp shape batch shifted")   # shifted: every device pointer one element into its block


def interps_of(shape: Shape) -> list:
    (sw, sh), (dw, dh) = shape.src, shape.dst
    return [i for i in INTERPS if i != "area" or (dw <= sw and dh <= sh)]


def runs(shape: Shape) -> list:
    return [Run(f, i, shape, n, s) for f in FORMATS for i in interps_of(shape) for n in (1, B) for s in (False, True)]


def form_reached(run: Run, sky: bool = False) -> tuple:
    """the kernel form a _dev run lands in: blocks are aligned to at least 16, a shifted pointer is one element past that"""
    fmt = FORMATS[run.fmt]
    (sw, sh), (dw, dh) = run.shape.src, run.shape.dst
    esize = np.dtype(R.FORMATS[fmt][0]).itemsize
    address = 1 if (run.shifted and sky) else (esize if run.shifted else 0)
    return (run.fmt, R.form_of(fmt, sw, sh, dw, dh, INTERPS[run.interp]), R.vector_stores(fmt, dw, address, sky), sky)


def sky_runs() -> list:
    return [Run("U8C3", "linear", s, n, sh) for s in SHAPES for n in (1, B) for sh in (False, True)]


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------------
def nan_pixel(sw: int, sh: int) -> tuple:
    """(row, column) of the NaN of item 0, channel 0: column 1 is the tap under a zero weight left of the first source column's centre"""
    return sh // 2, min(1, sw - 1)


def inf_pixel(sw: int, sh: int) -> tuple:
    """(row, column) of the +inf of item 0, last channel: row 1 is the tap under a zero weight above the first source row's centre"""
    return min(1, sh - 1), sw // 2


def images(fmt: int, sw: int, sh: int, special: bool = True) -> np.ndarray:
    """(B, sh, sw[, C]): item 0 a 0 / 255 checkerboard (uint8) or noise with one NaN and one +inf planted (float32), items 1.. full-range
    noise"""
    dt, ch = R.FORMATS[fmt]
    rng = np.random.default_rng(1000 * fmt + 7 * sw + sh)
    shape = (B,) + R.image_shape(fmt, sh, sw)
    if dt == np.uint8:
        a = rng.integers(0, 256, shape, dtype=np.uint8)
        board = ((np.arange(sh)[:, None] + np.arange(sw)[None, :]) % 2 * 255).astype(np.uint8)
        a[0] = board if ch == 1 else np.repeat(board[..., None], ch, axis=2)
        return a
    a = rng.normal(0, 40, shape).astype(np.float32)
    if special:
        v = a[0].reshape(sh, sw, ch)
        v[nan_pixel(sw, sh) + (0,)] = np.nan
        v[inf_pixel(sw, sh) + (ch - 1,)] = np.inf
    return a


SKY, OTHER = (180, 130), (0, 0)
STRIPES = [(180, 130, 70), (180, 10, 70), (200, 130, 0), (160, 130, 255), (200, 110, 9), (160, 150, 9), (180, 130, 1), (0, 0, 0)]


def prediction(sw: int, sh: int) -> np.ndarray:
    """(B, sh, sw, 3) uint8: flat vertical stripes -- the sky colour (180, 130, x), neighbours that share one of its two key channels, and
    pairs whose blend passes through 180 or 130 in one channel alone or in both at once -- shifted by one stripe in the lower half, so the
    blends occur along both axes.  Item 2 is noise in which the key is rare."""
    n = len(STRIPES)
    width = max(1, sw // n)
    col = (np.arange(sw) // width) % n
    a = np.empty((B, sh, sw, 3), np.uint8)
    for b in range(2):
        for y in range(sh):
            a[b, y] = np.array(STRIPES, np.uint8)[(col + b + (1 if y >= sh // 2 else 0)) % n]
    a[2] = np.random.default_rng(sw + 31 * sh).integers(120, 200, (sh, sw, 3), dtype=np.uint8)
    return a
