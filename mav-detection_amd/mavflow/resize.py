"""Image resize on the device (include/mavflow_resize.h): the ctypes binding as methods of _lib.Context (resize, sky_mask, each with an
*_enqueue twin that takes device pointers), `resize` with cv2's literal signature, and the reference's resize call sites by name:
sky_segmentation (src/datasets/dataset.py:153-158) and gt_of_resized (src/datasets/sim_data.py:78-79); im_helpers.resize_percent
(src/im_helpers.py:254-260) lives with the other image helpers.  The library is _lib's (same loader, no CPU fallback); the entry points
here are not in _lib.EXPORTS, which lists include/mavflow.h alone.

INTER_NEAREST, INTER_LINEAR and INTER_AREA (shrinking) on uint8 with 1 or 3 channels and float32 with 1 or 2; the arithmetic is OpenCV
4.x resize.cpp as remembered and is pinned to no cv2 build (the header lists what to re-check first)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import Context, _dev_ptr, _ptr, check
from .warp import WARP_F32C1, WARP_F32C2, WARP_U8C1, WARP_U8C3, _FORMATS, _deliver, _on_device, format_of

# every symbol include/mavflow_resize.h declares (tests check the library exports each of them)
EXPORTS = ("mav_resize", "mav_resize_dev", "mav_sky_mask", "mav_sky_mask_dev")

# cv2's constants
INTER_NEAREST, INTER_LINEAR, INTER_CUBIC, INTER_AREA, INTER_LANCZOS4, INTER_LINEAR_EXACT, INTER_NEAREST_EXACT = 0, 1, 2, 3, 4, 5, 6
MAX_SIDE = 32767                                                    # MAV_RESIZE_MAX_SIDE
SKY_KEY = (180, 130)                                                # channels 0 and 1 of the sky colour of the HRNet prediction (dataset.py:157)
_BUILT = (INTER_NEAREST, INTER_LINEAR, INTER_AREA)
_NAMES = {INTER_CUBIC: "INTER_CUBIC", INTER_LANCZOS4: "INTER_LANCZOS4", INTER_LINEAR_EXACT: "INTER_LINEAR_EXACT", INTER_NEAREST_EXACT: "INTER_NEAREST_EXACT"}

_ready = False


def load() -> C.CDLL:
    """_lib.load() with this header's prototypes attached."""
    global _ready
    lib = _lib.load()
    if not _ready:
        vp, i = C.c_void_p, C.c_int
        for fn in (lib.mav_resize, lib.mav_resize_dev):               # ctx, src, format, sw, sh, dw, dh, interpolation, batch, dst
            fn.restype, fn.argtypes = i, [vp, vp, i, i, i, i, i, i, i, vp]
        for fn in (lib.mav_sky_mask, lib.mav_sky_mask_dev):           # ctx, pred_bgr, sw, sh, dw, dh, key0, key1, batch, sky
            fn.restype, fn.argtypes = i, [vp, vp, i, i, i, i, i, i, i, vp]
        _ready = True
    return lib


def _round_half_even(v: float) -> int:
    return int(np.rint(v))


def dsize_of(w: int, h: int, dsize=None, fx: float = 0, fy: float = 0) -> tuple:
    """cv2.resize's destination size: dsize, or where it is None or (0, 0), (round_half_even(fx * w), round_half_even(fy * h))"""
    if dsize is not None and tuple(int(v) for v in dsize) != (0, 0):
        dw, dh = (int(v) for v in dsize)
    else:
        if not (fx > 0 and fy > 0):
            raise ValueError("resize: either dsize or both fx and fy must be positive")
        dw, dh = _round_half_even(fx * w), _round_half_even(fy * h)
    if not (1 <= dw <= MAX_SIDE and 1 <= dh <= MAX_SIDE):
        raise ValueError(f"resize: destination {dw} x {dh}: every side is in [1, {MAX_SIDE}]")
    return dw, dh


def _interpolation_checked(interpolation, sw, sh, dw, dh) -> int:
    interpolation = int(interpolation)
    if interpolation not in _BUILT:
        raise NotImplementedError(f"interpolation {_NAMES.get(interpolation, interpolation)} is not built: INTER_NEAREST, INTER_LINEAR and INTER_AREA are")
    if interpolation == INTER_AREA and (dw > sw or dh > sh):
        raise NotImplementedError(f"INTER_AREA enlarging ({sw} x {sh} -> {dw} x {dh}) is not built: OpenCV takes another coefficient scheme there")
    return interpolation


def _image(src, batched: bool, what="src"):
    """src (H, W[, C]), or with `batched` (B, H, W[, C]) -> (contiguous array, format, B, sw, sh, trailing channel axis?)"""
    a = np.asarray(src)
    if a.dtype == np.float64:
        raise TypeError(f"a float64 {what} would be rounded to float32: convert it yourself if that is meant")
    lead = 1 if batched else 0
    if a.ndim not in (lead + 2, lead + 3):
        raise ValueError(f"{what} has shape {a.shape}; expected {'(B, H, W[, C])' if batched else '(H, W[, C])'}")
    ch = 1 if a.ndim == lead + 2 else a.shape[-1]
    if a.dtype not in (np.uint8, np.float32):
        raise NotImplementedError(f"{what} of {a.dtype} is not built: uint8 (1 or 3 channels) and float32 (1 or 2 channels) are")
    if (a.dtype == np.uint8 and ch not in (1, 3)) or (a.dtype == np.float32 and ch not in (1, 2)):
        raise NotImplementedError(f"{what} of {a.dtype} with {ch} channels is not built: uint8 with 1 or 3 channels and float32 with 1 or 2 are")
    sh, sw = a.shape[lead], a.shape[lead + 1]
    if sw < 1 or sh < 1 or sw > MAX_SIDE or sh > MAX_SIDE:
        raise ValueError(f"{what} is {sw} x {sh}: every side is in [1, {MAX_SIDE}]")
    return np.ascontiguousarray(a), format_of((a.dtype, ch)), (a.shape[0] if batched else 1), sw, sh, a.ndim == lead + 3


def _resize(self, src, dsize=None, fx=0, fy=0, interpolation=INTER_LINEAR, batched: bool = False, format=None, ssize=None, batch: int = 1, dst=None):
    """cv2.resize(src, dsize, fx=fx, fy=fy, interpolation=interpolation) on this context's stream; the sizes are independent of the
    context's frame.  src: a host array (H, W[, C]), or with batched=True (B, H, W[, C]) -- the resized array(s) come back; or a device
    handle of this context (.ptr) with format= (WARP_*), ssize=(sw, sh) and batch= -- the result stays on the device, in dst (a handle)
    or in a new DeviceBuffer the caller frees, which is returned."""
    lib = load()
    if _on_device(self, src):
        if format is None or ssize is None:
            raise ValueError("resize of a device handle needs format= and ssize=(sw, sh)")
        sw, sh = (int(v) for v in ssize)
        dw, dh = dsize_of(sw, sh, dsize, fx, fy)
        interpolation = _interpolation_checked(interpolation, sw, sh, dw, dh)
        dt, ch = _FORMATS[int(format)]
        out = self.alloc(int(batch) * dw * dh * ch * dt.itemsize) if dst is None else dst
        check(lib.mav_resize_dev(self.h, _dev_ptr(src), int(format), sw, sh, dw, dh, interpolation, int(batch), _dev_ptr(out)))
        return out
    a, fmt, B, sw, sh, has_c = _image(src, batched)
    dw, dh = dsize_of(sw, sh, dsize, fx, fy)
    interpolation = _interpolation_checked(interpolation, sw, sh, dw, dh)
    ch = _FORMATS[fmt][1]
    out = np.empty(((B,) if batched else ()) + (dh, dw) + ((ch,) if has_c else ()), a.dtype)
    check(lib.mav_resize(self.h, _ptr(a), fmt, sw, sh, dw, dh, interpolation, B, _ptr(out)))
    return out


def _resize_enqueue(self, src_ptr, fmt: int, sw: int, sh: int, dw: int, dh: int, interp: int, batch: int, dst_ptr) -> None:
    """mav_resize_dev: src (batch, sh, sw, C) and dst (batch, dh, dw, C) of format `fmt` in device memory; enqueue only"""
    check(load().mav_resize_dev(self.h, _dev_ptr(src_ptr), int(fmt), int(sw), int(sh), int(dw), int(dh), int(interp), int(batch), _dev_ptr(dst_ptr)))


def _sky_mask(self, pred_bgr, dsize=None, key=SKY_KEY, ssize=None, batch: int = 1, dst=None):
    """The sky mask of a prediction picture (Dataset.get_sky_segmentation, dataset.py:153-158): cv2.resize(pred_bgr, dsize) with
    INTER_LINEAR, then (c0 == key[0]) * (c1 == key[1]), in one pass.  dsize defaults to the context's (W, H).  pred_bgr: a host array
    (h, w, 3) or (B, h, w, 3) uint8 -- a bool array (H, W) or (B, H, W) comes back; or a device handle with ssize=(sw, sh) and batch= --
    the uint8 mask stays on the device, in dst or in a new DeviceBuffer, which is returned (what detect's sky_dev takes)."""
    lib = load()
    dw, dh = (self.W, self.H) if dsize is None else (int(v) for v in dsize)
    k0, k1 = (int(v) for v in key)
    if _on_device(self, pred_bgr):
        if ssize is None:
            raise ValueError("sky_mask of a device handle needs ssize=(sw, sh)")
        sw, sh = (int(v) for v in ssize)
        out = self.alloc(int(batch) * dw * dh) if dst is None else dst
        check(lib.mav_sky_mask_dev(self.h, _dev_ptr(pred_bgr), sw, sh, dw, dh, k0, k1, int(batch), _dev_ptr(out)))
        return out
    a = np.asarray(pred_bgr)
    if a.dtype != np.uint8 or a.ndim not in (3, 4) or a.shape[-1] != 3:
        raise TypeError(f"sky_mask takes a uint8 picture (h, w, 3) or (B, h, w, 3), got {a.dtype} {a.shape}")
    a = np.ascontiguousarray(a)
    single = a.ndim == 3
    B, sh, sw = (1 if single else a.shape[0]), a.shape[-3], a.shape[-2]
    out = np.empty((dh, dw) if single else (B, dh, dw), np.uint8)
    check(lib.mav_sky_mask(self.h, _ptr(a), sw, sh, dw, dh, k0, k1, B, _ptr(out)))
    return out.view(np.bool_)


def _sky_mask_enqueue(self, pred_ptr, sw: int, sh: int, dw: int, dh: int, sky_ptr, key=SKY_KEY, batch: int = 1) -> None:
    """mav_sky_mask_dev: pred (batch, sh, sw, 3) uint8 and sky (batch, dh, dw) uint8 in device memory; enqueue only"""
    check(load().mav_sky_mask_dev(self.h, _dev_ptr(pred_ptr), int(sw), int(sh), int(dw), int(dh), int(key[0]), int(key[1]), int(batch), _dev_ptr(sky_ptr)))


Context.resize = _resize
Context.resize_enqueue = _resize_enqueue
Context.sky_mask = _sky_mask
Context.sky_mask_enqueue = _sky_mask_enqueue


# ---- cv2's signature, and the reference's call sites ------------------------------------------------------------------------------------------
def _ctx_of(w: int, h: int, batch: int = 1) -> Context:
    """im_helpers' cached context of this size (the sizes of a resize are its own: any context serves, this one holds no more than its
    staging blocks)"""
    from . import im_helpers
    return im_helpers._ctx(int(w), int(h), batch)


def resize(src, dsize, dst=None, fx=0, fy=0, interpolation=INTER_LINEAR, batched: bool = False):
    """cv2.resize's signature.  src uint8 (H, W), (H, W, 1 | 3) or float32 (H, W), (H, W, 1 | 2); dsize (w, h), or None / (0, 0) with
    fx, fy.  NotImplementedError names what is not built: other interpolations, 4 channels, uint16, INTER_AREA enlarging; TypeError
    for a float64 source (it would round).  batched=True: src carries a leading batch axis."""
    a, _, B, sw, sh, _ = _image(src, batched)                   # what is not built is refused before a context is made
    _interpolation_checked(interpolation, sw, sh, *dsize_of(sw, sh, dsize, fx, fy))
    return _deliver(_ctx_of(sw, sh, B).resize(a, dsize, fx, fy, interpolation, batched=batched), dst)


def sky_segmentation(prediction_bgr, size=(1920, 1024)) -> np.ndarray:
    """The body of Dataset.get_sky_segmentation after imread (dataset.py:153-158): the prediction resized to `size` (INTER_LINEAR) and
    keyed on (180, 130) in channels 0 and 1; a bool (H, W)."""
    return _ctx_of(size[0], size[1]).sky_mask(prediction_bgr, size, SKY_KEY)


def gt_of_resized(flow, capture_size):
    """sim_data.py:78-79: the .flo field resized to capture_size (INTER_LINEAR; the vectors are not rescaled, as in the reference);
    the input itself when the sizes agree."""
    if tuple(int(v) for v in capture_size) == (flow.shape[1], flow.shape[0]):
        return flow
    return resize(flow, tuple(int(v) for v in capture_size))
