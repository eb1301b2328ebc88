"""Flow pictures on the device (include/mavflow_vis.h): the ctypes binding as methods of _lib.Context (flow_hsv, cvt_color, draw_flow,
each with an *_enqueue twin that takes device pointers) and `cvtColor` with cv2's signature for the two codes that are built.  The
library is _lib's (same loader, no CPU fallback); the entry points here are not in _lib.EXPORTS, which lists include/mavflow.h alone.

MAV_HSV_PROCESS is mavflow.farneback.flow_to_hsv + hsv_to_bgr on the device (bit for bit up to atan2f), MAV_HSV_DRAW the reference's
Farneback.draw_hsv; BGR -> HSV, the line clip and the line stepping are OpenCV 4.x as remembered and pinned to no cv2 build (the header
lists what to re-check first)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import Context, _dev_ptr, _ptr, check

# every symbol include/mavflow_vis.h declares (tests check the library exports each of them)
EXPORTS = ("mav_flow_hsv", "mav_flow_hsv_dev", "mav_cvt_color", "mav_cvt_color_dev", "mav_draw_flow", "mav_draw_flow_dev", "mav_vis_form")

HSV_PROCESS, HSV_DRAW = 0, 1                                        # MAV_HSV_*
COLOR_BGR2HSV, COLOR_HSV2BGR = 40, 54                               # cv2's values, and MAV_COLOR_*'s
COLOR_BGR2RADIAL = 1040                                             # MAV_COLOR_BGR2RADIAL: im_helpers.get_flow_radial in one pass
FORM_BYTES, FORM_FAST = 0, 1                                        # MAV_VIS_FORM_*
_MODES = {"process": HSV_PROCESS, "draw": HSV_DRAW, HSV_PROCESS: HSV_PROCESS, HSV_DRAW: HSV_DRAW}
_CODES = (COLOR_BGR2HSV, COLOR_HSV2BGR, COLOR_BGR2RADIAL)

RECORD_DTYPE = np.dtype([("mag_min", np.float32), ("mag_max", np.float32), ("nonzero", np.int32), ("invalid", np.int32)])
assert RECORD_DTYPE.itemsize == 16

_ready = False


def load() -> C.CDLL:
    """_lib.load() with this header's prototypes attached."""
    global _ready
    lib = _lib.load()
    if not _ready:
        vp, i = C.c_void_p, C.c_int
        for fn in (lib.mav_flow_hsv, lib.mav_flow_hsv_dev):               # ctx, flow, batch, mode, bgr, hsv, records
            fn.restype, fn.argtypes = i, [vp, vp, i, i, vp, vp, vp]
        for fn in (lib.mav_cvt_color, lib.mav_cvt_color_dev):             # ctx, src, code, batch, dst
            fn.restype, fn.argtypes = i, [vp, vp, i, i, vp]
        for fn in (lib.mav_draw_flow, lib.mav_draw_flow_dev):             # ctx, img, flow, batch, step, threshold, bgr_colour
            fn.restype, fn.argtypes = i, [vp, vp, vp, i, i, C.c_float, vp]
        lib.mav_vis_form.restype, lib.mav_vis_form.argtypes = i, [i, i, i, vp, vp, vp]
        _ready = True
    return lib


def vis_form(W: int, H: int, batch: int, flow=None, bgr=None, hsv=None) -> int:
    """mav_vis_form: the form (FORM_FAST / FORM_BYTES) a call of these sizes and pointers (ints, or None) takes"""
    return int(load().mav_vis_form(int(W), int(H), int(batch), flow, bgr, hsv))


def _on_device(ctx, a) -> bool:
    return hasattr(a, "ptr") and getattr(a, "on_device", True) and getattr(a, "ctx", ctx) is ctx


def _mode(mode) -> int:
    if mode not in _MODES:
        raise ValueError(f"mode must be 'process' or 'draw', got {mode!r}")
    return _MODES[mode]


def _code(code) -> int:
    if int(code) not in _CODES:
        raise NotImplementedError(f"cvtColor code {code} is not built: COLOR_BGR2HSV ({COLOR_BGR2HSV}) and COLOR_HSV2BGR ({COLOR_HSV2BGR}) are")
    return int(code)


def _fields(self, flow, what="flow"):
    """flow (H, W, 2) or (B, H, W, 2) float32 of this context's frame -> (contiguous array, batch, single)"""
    a = np.asarray(flow)
    if a.dtype == np.float64:
        raise TypeError(f"a float64 {what} would be rounded to float32: convert it yourself if that is meant")
    if a.dtype != np.float32:
        raise TypeError(f"{what} must be float32, got {a.dtype}")
    H, W = self.H, self.W
    if a.shape == (H, W, 2):
        return np.ascontiguousarray(a), 1, True
    if a.ndim == 4 and a.shape[1:] == (H, W, 2):
        return np.ascontiguousarray(a), int(a.shape[0]), False
    raise ValueError(f"{what} has shape {a.shape}; this context's frame is {W} x {H}: (H, W, 2) or (B, H, W, 2)")


def _pictures(self, img, what="img"):
    """img (H, W, 3) or (B, H, W, 3) uint8 of this context's frame -> (the array, batch, single)"""
    a = np.asarray(img)
    H, W = self.H, self.W
    if a.dtype != np.uint8:
        raise TypeError(f"{what} must be uint8 with 3 channels, got {a.dtype}")
    if a.shape == (H, W, 3):
        return a, 1, True
    if a.ndim == 4 and a.shape[1:] == (H, W, 3):
        return a, int(a.shape[0]), False
    raise ValueError(f"{what} has shape {a.shape}; this context's frame is {W} x {H}: (H, W, 3) or (B, H, W, 3)")


def _flow_hsv(self, flow, mode="process", hsv: bool = False, batch: int = 1) -> dict:
    """The picture of a flow field: mode "process" is Farneback.process()'s (flow_to_hsv + hsv_to_bgr: hue from the angle, value from the
    min-max-normalised magnitude), "draw" is Farneback.draw_hsv's.  flow (H, W, 2) or (B, H, W, 2) float32 on the host, or a device handle
    of this context (.ptr) holding `batch` fields.  Returns bgr, hsv (with hsv=True) and record (a RECORD_DTYPE array (B,), or the one
    record of a single field): mag_min, mag_max, nonzero, invalid ("process"; zeros for "draw")."""
    lib, m = load(), _mode(mode)
    H, W = self.H, self.W
    if _on_device(self, flow):
        B, single = int(batch), int(batch) == 1 and len(getattr(flow, "shape", (0, 0, 0))) == 3
        n = B * H * W
        ob = 16 * B                                                    # the records, then each picture at a multiple of 16
        oh = ob + (n * 3 + 15) // 16 * 16
        blk = self.alloc(oh + (n * 3 if hsv else 0))                   # the call's own block, freed below
        try:
            check(lib.mav_flow_hsv_dev(self.h, _dev_ptr(flow), B, m, blk.ptr + ob, blk.ptr + oh if hsv else None, blk.ptr))
            raw = blk.download(np.uint8, (blk.nbytes,))
        finally:
            blk.free()
        out = dict(bgr=raw[ob:ob + n * 3].reshape(B, H, W, 3), record=raw[:ob].view(RECORD_DTYPE))
        if hsv:
            out["hsv"] = raw[oh:oh + n * 3].reshape(B, H, W, 3)
    else:
        a, B, single = _fields(self, flow)
        bgr = np.empty((B, H, W, 3), np.uint8)
        hs = np.empty((B, H, W, 3), np.uint8) if hsv else None
        rec = np.empty(B, RECORD_DTYPE)
        check(lib.mav_flow_hsv(self.h, _ptr(a), B, m, _ptr(bgr), _ptr(hs) if hsv else None, _ptr(rec)))
        out = dict(bgr=bgr, record=rec)
        if hsv:
            out["hsv"] = hs
    if single:
        out = {k: v[0] for k, v in out.items()}
    return out


def _flow_hsv_enqueue(self, flow_ptr, bgr_ptr, records_ptr, mode="process", hsv_ptr=None, batch: int = 1) -> None:
    """mav_flow_hsv_dev: flow (batch, H, W, 2) float32, bgr and (unless None) hsv (batch, H, W, 3) uint8, records (batch) of 16 bytes, all
    in device memory; enqueue only"""
    check(load().mav_flow_hsv_dev(self.h, _dev_ptr(flow_ptr), int(batch), _mode(mode), _dev_ptr(bgr_ptr),
                                  None if hsv_ptr is None else _dev_ptr(hsv_ptr), _dev_ptr(records_ptr)))


def _cvt_color(self, img, code) -> np.ndarray:
    """cv2.cvtColor(img, code) for COLOR_HSV2BGR and COLOR_BGR2HSV (and COLOR_BGR2RADIAL) on (H, W, 3) or (B, H, W, 3) uint8"""
    lib, code = load(), _code(code)
    a, B, _ = _pictures(self, img)
    a = np.ascontiguousarray(a)
    dst = np.empty_like(a)
    check(lib.mav_cvt_color(self.h, _ptr(a), code, B, _ptr(dst)))
    return dst


def _cvt_color_enqueue(self, src_ptr, code, dst_ptr, batch: int = 1) -> None:
    """mav_cvt_color_dev: src, dst (batch, H, W, 3) uint8 in device memory; enqueue only"""
    check(load().mav_cvt_color_dev(self.h, _dev_ptr(src_ptr), _code(code), int(batch), _dev_ptr(dst_ptr)))


def _colour(color):
    c = np.asarray(color)
    if c.shape != (3,) or np.any(c < 0) or np.any(c > 255):
        raise ValueError(f"color must be three values in [0, 255] (B, G, R), got {color!r}")
    return np.ascontiguousarray(c, np.uint8)


def _draw_flow(self, img, flow, step: int = 8, threshold: float = 1.0, color=(0, 255, 0)) -> np.ndarray:
    """Farneback.draw_flow (src/farneback.py:28-48): from every step-th pixel whose flow is longer than `threshold` a line to where the
    flow points (cv2.polylines, thickness 1) and a dot of radius 1 at the pixel, all in `color` (B, G, R).  img (H, W, 3) or
    (B, H, W, 3) uint8 is drawn into and returned, as cv2.polylines does; flow the float32 field(s) of the same batch."""
    lib = load()
    a, B, _ = _pictures(self, img)
    f, Bf, _ = _fields(self, flow)
    if Bf != B:
        raise ValueError(f"img holds {B} pictures and flow {Bf} fields")
    if int(step) < 1:
        raise ValueError(f"step must be at least 1, got {step}")
    if not (isinstance(img, np.ndarray) and img.flags.writeable):
        raise TypeError("img must be a writeable numpy array: it is drawn into")
    work = a if a.flags.c_contiguous else np.ascontiguousarray(a)
    check(lib.mav_draw_flow(self.h, _ptr(work), _ptr(f), B, int(step), float(threshold), _ptr(_colour(color))))
    if work is not a:
        img[...] = work
    return img


def _draw_flow_enqueue(self, img_ptr, flow_ptr, step: int = 8, threshold: float = 1.0, color=(0, 255, 0), batch: int = 1) -> None:
    """mav_draw_flow_dev: img (batch, H, W, 3) uint8 drawn into, flow (batch, H, W, 2) float32, in device memory; enqueue only"""
    check(load().mav_draw_flow_dev(self.h, _dev_ptr(img_ptr), _dev_ptr(flow_ptr), int(batch), int(step), float(threshold), _ptr(_colour(color))))


Context.flow_hsv = _flow_hsv
Context.flow_hsv_enqueue = _flow_hsv_enqueue
Context.cvt_color = _cvt_color
Context.cvt_color_enqueue = _cvt_color_enqueue
Context.draw_flow = _draw_flow
Context.draw_flow_enqueue = _draw_flow_enqueue


def cvtColor(src, code, dst=None):
    """cv2.cvtColor's signature for COLOR_HSV2BGR (54) and COLOR_BGR2HSV (40) on an (H, W, 3) uint8 image; NotImplementedError names what
    is built for any other code."""
    code = _code(code)
    a = np.asarray(src)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        raise NotImplementedError(f"cvtColor of {a.dtype} {a.shape} is not built: (H, W, 3) uint8 is")
    from . import im_helpers
    res = im_helpers._ctx(a.shape[1], a.shape[0]).cvt_color(a, code)
    if dst is None:
        return res
    dst[...] = res
    return dst
