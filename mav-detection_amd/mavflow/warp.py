"""Image warps on the device (include/mavflow_warp.h): the ctypes binding as methods of _lib.Context (remap, warp_flow, warp_affine,
warp_perspective, warp_method, each with an *_enqueue twin that takes device pointers) and `remap`, `warpAffine`, `warpPerspective`
with cv2's literal signatures.  The library is _lib's (same loader, no CPU fallback); the entry points here are not in _lib.EXPORTS,
which lists include/mavflow.h alone.

INTER_LINEAR and BORDER_CONSTANT with value 0 only, source and destination of one size; the arithmetic is OpenCV 4.x imgwarp.cpp as
remembered and is pinned to no cv2 build (the header lists what to re-check first)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import Context, _dev_ptr, _ptr, check

# every symbol include/mavflow_warp.h declares (tests check the library exports each of them)
EXPORTS = ("mav_remap", "mav_remap_dev", "mav_remap_planes", "mav_remap_planes_dev", "mav_warp_flow", "mav_warp_flow_dev", "mav_warp_affine",
           "mav_warp_affine_dev", "mav_warp_perspective", "mav_warp_perspective_dev", "mav_warp_method", "mav_warp_method_dev")

WARP_U8C1, WARP_U8C3, WARP_F32C1, WARP_F32C2 = 0, 1, 2, 3           # MAV_WARP_*
WARP_INVERSE_MAP_FLAG = 16                                          # MAV_WARP_INVERSE_MAP
WARP_AFFINE, WARP_PERSPECTIVE = 0, 1
# cv2's constants, for the functions with cv2's signatures below
INTER_NEAREST, INTER_LINEAR, INTER_CUBIC, INTER_AREA, INTER_LANCZOS4 = 0, 1, 2, 3, 4
WARP_INVERSE_MAP = 16
BORDER_CONSTANT, BORDER_REPLICATE, BORDER_REFLECT, BORDER_WRAP, BORDER_REFLECT_101, BORDER_TRANSPARENT = 0, 1, 2, 3, 4, 5
_INTER_MASK = 7

_FORMATS = {WARP_U8C1: (np.dtype(np.uint8), 1), WARP_U8C3: (np.dtype(np.uint8), 3), WARP_F32C1: (np.dtype(np.float32), 1),
            WARP_F32C2: (np.dtype(np.float32), 2)}


class WarpRecord(C.Structure):
    """mav_warp_record"""
    _fields_ = [("max_mag", C.c_float), ("row", C.c_int32), ("col", C.c_int32), ("pad", C.c_int32)]


RECORD_DTYPE = np.dtype([("max_mag", np.float32), ("row", np.int32), ("col", np.int32), ("pad", np.int32)])
assert RECORD_DTYPE.itemsize == C.sizeof(WarpRecord) == 16

_ready = False


def load() -> C.CDLL:
    """_lib.load() with this header's prototypes attached."""
    global _ready
    lib = _lib.load()
    if not _ready:
        vp, i = C.c_void_p, C.c_int
        for name in ("mav_remap", "mav_warp_flow"):                       # ctx, src, format, map_xy | flow, batch, dst
            for fn in (getattr(lib, name), getattr(lib, name + "_dev")):
                fn.restype, fn.argtypes = i, [vp, vp, i, vp, i, vp]
        for fn in (lib.mav_remap_planes, lib.mav_remap_planes_dev):       # ctx, src, format, map_x, map_y, batch, dst
            fn.restype, fn.argtypes = i, [vp, vp, i, vp, vp, i, vp]
        for name in ("mav_warp_affine", "mav_warp_perspective"):          # ctx, src, format, M, flags, batch, dst
            for fn in (getattr(lib, name), getattr(lib, name + "_dev")):
                fn.restype, fn.argtypes = i, [vp, vp, i, vp, i, i, vp]
        for fn in (lib.mav_warp_method, lib.mav_warp_method_dev):         # ctx, flow, M, kind, batch, diff, mag, records
            fn.restype, fn.argtypes = i, [vp, vp, vp, i, i, vp, vp, vp]
        _ready = True
    return lib


def format_of(img) -> int:
    """The MAV_WARP_* format of a (dtype, channels) pair; TypeError for any other, float64 (which would round) among them."""
    dt, ch = img
    for fmt, (d, c) in _FORMATS.items():
        if d == np.dtype(dt) and c == ch:
            return fmt
    if np.dtype(dt) == np.float64:
        raise TypeError("a float64 image would be rounded to float32: convert it yourself if that is meant")
    raise TypeError(f"images are uint8 with 1 or 3 channels or float32 with 1 or 2 channels, got {np.dtype(dt)} with {ch}")


def _images(self, src, what="src"):
    """src of this context's frame, one image or a batch -> (contiguous (B, H, W, C) view's array, format, single, its shape)"""
    a = np.asarray(src)
    H, W = self.H, self.W
    if a.dtype == np.float64:
        format_of((a.dtype, 1))
    if a.shape in ((H, W), (H, W, 2), (H, W, 3)):
        single, ch = True, 1 if a.ndim == 2 else a.shape[2]
    elif a.ndim >= 3 and a.shape[1:] in ((H, W), (H, W, 2), (H, W, 3)):
        single, ch = False, 1 if a.ndim == 3 else a.shape[3]
    else:
        raise ValueError(f"{what} has shape {a.shape}; this context's frame is {W} x {H}: (H, W[, C]) or (B, H, W[, C])")
    fmt = format_of((a.dtype, ch))
    return np.ascontiguousarray(a), fmt, single, a.shape


def _batch_of(single, shape) -> int:
    return 1 if single else int(shape[0])


def _operand(a, dtype, shape, what):
    a = np.ascontiguousarray(a, dtype)
    if a.shape != shape:
        raise ValueError(f"{what} has shape {a.shape}; expected {shape}")
    return a


def _remap(self, src, map1, map2=None) -> np.ndarray:
    """cv2.remap(src, map1, map2, INTER_LINEAR) with BORDER_CONSTANT 0: src (H, W[, C]) or a batch (B, H, W[, C]), uint8 with 1 or 3
    channels or float32 with 1 or 2; map1 (.., H, W, 2) float32 absolute source coordinates with map2 None, or map1 / map2 (.., H, W)
    float32 planes.  Returns the warped image(s), same shape and dtype."""
    lib = load()
    a, fmt, single, shape = _images(self, src)
    B = _batch_of(single, shape)
    dst = np.empty_like(a)
    lead = () if single else (B,)
    if map2 is None:
        m = _operand(map1, np.float32, lead + (self.H, self.W, 2), "map1")
        check(lib.mav_remap(self.h, _ptr(a), fmt, _ptr(m), B, _ptr(dst)))
    else:
        mx = _operand(map1, np.float32, lead + (self.H, self.W), "map1")
        my = _operand(map2, np.float32, lead + (self.H, self.W), "map2")
        check(lib.mav_remap_planes(self.h, _ptr(a), fmt, _ptr(mx), _ptr(my), B, _ptr(dst)))
    return dst


def _warp_flow(self, img, flow) -> np.ndarray:
    """Farneback.warp_flow (src/farneback.py:63-69) fused: img sampled at grid - flow, the map generated in the kernel.  img as in remap,
    flow (.., H, W, 2) float32 (not written)."""
    a, fmt, single, shape = _images(self, img, "img")
    B = _batch_of(single, shape)
    f = _operand(flow, np.float32, (() if single else (B,)) + (self.H, self.W, 2), "flow")
    dst = np.empty_like(a)
    check(load().mav_warp_flow(self.h, _ptr(a), fmt, _ptr(f), B, _ptr(dst)))
    return dst


def _matrix_warp(self, name, rows, src, M, inverse_map):
    a, fmt, single, shape = _images(self, src)
    B = _batch_of(single, shape)
    M = np.asarray(M, np.float64)
    if M.shape == (rows, 3) and not single:
        M = np.broadcast_to(M, (B, rows, 3))
    M = _operand(M, np.float64, (() if single else (B,)) + (rows, 3), "M")
    dst = np.empty_like(a)
    check(getattr(load(), name)(self.h, _ptr(a), fmt, _ptr(M), WARP_INVERSE_MAP_FLAG if inverse_map else 0, B, _ptr(dst)))
    return dst


def _warp_affine(self, src, M, inverse_map: bool = False) -> np.ndarray:
    """cv2.warpAffine(src, M, (W, H), flags=INTER_LINEAR [| WARP_INVERSE_MAP]) with BORDER_CONSTANT 0.  M (2, 3), or (B, 2, 3) for a
    batch.  Without inverse_map M is inverted on the device; a singular or non-finite matrix is refused (ValueError)."""
    return _matrix_warp(self, "mav_warp_affine", 2, src, M, inverse_map)


def _warp_perspective(self, src, M, inverse_map: bool = False) -> np.ndarray:
    """cv2.warpPerspective likewise, M (3, 3) or (B, 3, 3)."""
    return _matrix_warp(self, "mav_warp_perspective", 3, src, M, inverse_map)


def _on_device(ctx, a) -> bool:
    return hasattr(a, "ptr") and getattr(a, "on_device", True) and getattr(a, "ctx", ctx) is ctx


def _warp_method(self, flow, M, kind=None) -> dict:
    """Detector.warp_method's arithmetic (src/detector.py:213-224) in one pass: the float32 field warped by M (inverted, as cv2 does),
    subtracted, its magnitude and the first position of the largest.  flow (H, W, 2) or (B, H, W, 2) float32 on the host, or a device
    handle of this context (.ptr; one field); M (2, 3) / (3, 3) or a batch of them; kind: WARP_AFFINE / WARP_PERSPECTIVE, by default
    from M's shape.  Returns diff, mag, max_mag, flow_max (row, col) and records."""
    lib = load()
    M = np.asarray(M, np.float64)
    if kind is None:
        kind = WARP_PERSPECTIVE if M.shape[-2:] == (3, 3) else WARP_AFFINE
    rows = 3 if kind == WARP_PERSPECTIVE else 2
    H, W = self.H, self.W
    if _on_device(self, flow):
        if getattr(flow, "_deferred", None) is not None:
            flow._deferred.flush()
        M = _operand(M, np.float64, (rows, 3), "M")
        bufs = []
        try:
            for nbytes in (M.nbytes, 8 * H * W, 4 * H * W, 16):
                bufs.append(self.alloc(nbytes))
            dm, dd, dg, dr = bufs
            dm.upload(M)
            check(lib.mav_warp_method_dev(self.h, _dev_ptr(flow), dm.ptr, kind, 1, dd.ptr, dg.ptr, dr.ptr))
            diff, mag, rec = dd.download(np.float32, (H, W, 2)), dg.download(np.float32, (H, W)), dr.download(RECORD_DTYPE, (1,))
        finally:
            for b in bufs:
                b.free()
        single = True
    else:
        f = np.ascontiguousarray(flow)
        if f.dtype != np.float32:
            raise TypeError(f"warp_method takes a float32 field, got {f.dtype}")
        single = f.shape == (H, W, 2)
        B = 1 if single else f.shape[0]
        f = _operand(f, np.float32, (() if single else (B,)) + (H, W, 2), "flow")
        if M.shape == (rows, 3) and not single:
            M = np.broadcast_to(M, (B, rows, 3))
        M = _operand(M, np.float64, (() if single else (B,)) + (rows, 3), "M")
        diff, mag, rec = np.empty_like(f), np.empty(f.shape[:-1], np.float32), np.zeros(B, RECORD_DTYPE)
        check(lib.mav_warp_method(self.h, _ptr(f), _ptr(M), kind, B, _ptr(diff), _ptr(mag), _ptr(rec)))
    out = dict(diff=diff, mag=mag, max_mag=rec["max_mag"].copy(), flow_max=np.stack([rec["row"], rec["col"]], axis=-1), records=rec)
    if single:
        out.update(max_mag=float(rec["max_mag"][0]), flow_max=(int(rec["row"][0]), int(rec["col"][0])), records=rec[0])
    return out


# ---- the *_enqueue twins: device pointers (ints, or objects with a .ptr), enqueue only ----------------------------------------------------
def _remap_enqueue(self, src_ptr, format: int, map1_ptr, dst_ptr, batch: int = 1, map2_ptr=None) -> None:
    """mav_remap_dev, or mav_remap_planes_dev with map2_ptr: src / dst (batch, H, W, C) of `format`, maps float32."""
    if map2_ptr is None:
        check(load().mav_remap_dev(self.h, _dev_ptr(src_ptr), int(format), _dev_ptr(map1_ptr), int(batch), _dev_ptr(dst_ptr)))
    else:
        check(load().mav_remap_planes_dev(self.h, _dev_ptr(src_ptr), int(format), _dev_ptr(map1_ptr), _dev_ptr(map2_ptr), int(batch), _dev_ptr(dst_ptr)))


def _warp_flow_enqueue(self, img_ptr, format: int, flow_ptr, dst_ptr, batch: int = 1) -> None:
    """mav_warp_flow_dev"""
    check(load().mav_warp_flow_dev(self.h, _dev_ptr(img_ptr), int(format), _dev_ptr(flow_ptr), int(batch), _dev_ptr(dst_ptr)))


def _warp_affine_enqueue(self, src_ptr, format: int, M_ptr, dst_ptr, batch: int = 1, inverse_map: bool = False) -> None:
    """mav_warp_affine_dev: M (batch, 2, 3) double in device memory"""
    check(load().mav_warp_affine_dev(self.h, _dev_ptr(src_ptr), int(format), _dev_ptr(M_ptr), WARP_INVERSE_MAP_FLAG if inverse_map else 0, int(batch),
                                     _dev_ptr(dst_ptr)))


def _warp_perspective_enqueue(self, src_ptr, format: int, M_ptr, dst_ptr, batch: int = 1, inverse_map: bool = False) -> None:
    """mav_warp_perspective_dev: M (batch, 3, 3) double in device memory -- what mav_flow_homography_dev leaves, with no host round trip"""
    check(load().mav_warp_perspective_dev(self.h, _dev_ptr(src_ptr), int(format), _dev_ptr(M_ptr), WARP_INVERSE_MAP_FLAG if inverse_map else 0, int(batch),
                                          _dev_ptr(dst_ptr)))


def _warp_method_enqueue(self, flow_ptr, M_ptr, kind: int, records_ptr, batch: int = 1, diff_ptr=None, mag_ptr=None) -> None:
    """mav_warp_method_dev: records `batch` RECORD_DTYPE blocks aligned to 16; diff and mag optional"""
    check(load().mav_warp_method_dev(self.h, _dev_ptr(flow_ptr), _dev_ptr(M_ptr), int(kind), int(batch), None if diff_ptr is None else _dev_ptr(diff_ptr),
                                     None if mag_ptr is None else _dev_ptr(mag_ptr), _dev_ptr(records_ptr)))


Context.remap = _remap
Context.warp_flow = _warp_flow
Context.warp_affine = _warp_affine
Context.warp_perspective = _warp_perspective
Context.warp_method = _warp_method
Context.remap_enqueue = _remap_enqueue
Context.warp_flow_enqueue = _warp_flow_enqueue
Context.warp_affine_enqueue = _warp_affine_enqueue
Context.warp_perspective_enqueue = _warp_perspective_enqueue
Context.warp_method_enqueue = _warp_method_enqueue


# ---- cv2's signatures ------------------------------------------------------------------------------------------------------------------------
def _ctx_for(src):
    from . import im_helpers
    a = np.asarray(src)
    if a.ndim not in (2, 3):
        raise ValueError(f"src has shape {a.shape}; expected (H, W) or (H, W, C)")
    return im_helpers._ctx(a.shape[1], a.shape[0])


def _border_checked(borderMode, borderValue):
    if int(borderMode) != BORDER_CONSTANT:
        raise NotImplementedError(f"borderMode {borderMode}: BORDER_CONSTANT alone is built")
    if np.any(np.asarray(borderValue) != 0):
        raise NotImplementedError(f"borderValue {borderValue}: the constant border is 0")


def _deliver(res, dst):
    if dst is None:
        return res
    dst[...] = res
    return dst


def remap(src, map1, map2, interpolation, dst=None, borderMode=BORDER_CONSTANT, borderValue=0):
    """cv2.remap's signature: map1 (H, W, 2) float32 with map2 None, or map1 / map2 (H, W) float32 planes; interpolation INTER_LINEAR.
    NotImplementedError for any other interpolation or border, a non-zero borderValue and fixed-point (CV_16SC2) maps; TypeError for a
    float64 source (it would round)."""
    if int(interpolation) != INTER_LINEAR:
        raise NotImplementedError(f"interpolation {interpolation}: INTER_LINEAR alone is built")
    _border_checked(borderMode, borderValue)
    m1 = np.asarray(map1)
    if m1.dtype == np.int16 or (map2 is not None and np.asarray(map2).dtype in (np.int16, np.uint16)):
        raise NotImplementedError("fixed-point (CV_16SC2) maps are not built: pass float32 coordinates")
    return _deliver(_ctx_for(src).remap(src, map1, map2), dst)


def _matrix_call(method, src, M, dsize, dst, flags, borderMode, borderValue):
    a = np.asarray(src)
    if tuple(int(v) for v in dsize) != (a.shape[1], a.shape[0]):
        raise NotImplementedError(f"dsize {tuple(dsize)}: a destination of another size than the source's {(a.shape[1], a.shape[0])} is not built")
    if int(flags) & _INTER_MASK != INTER_LINEAR or int(flags) & ~(_INTER_MASK | WARP_INVERSE_MAP):
        raise NotImplementedError(f"flags {flags}: INTER_LINEAR, with or without WARP_INVERSE_MAP, alone is built")
    _border_checked(borderMode, borderValue)
    return _deliver(getattr(_ctx_for(src), method)(src, M, inverse_map=bool(int(flags) & WARP_INVERSE_MAP)), dst)


def warpAffine(src, M, dsize, dst=None, flags=INTER_LINEAR, borderMode=BORDER_CONSTANT, borderValue=0):
    """cv2.warpAffine's signature; dsize must be the source's (W, H)."""
    return _matrix_call("warp_affine", src, M, dsize, dst, flags, borderMode, borderValue)


def warpPerspective(src, M, dsize, dst=None, flags=INTER_LINEAR, borderMode=BORDER_CONSTANT, borderValue=0):
    """cv2.warpPerspective's signature; dsize must be the source's (W, H)."""
    return _matrix_call("warp_perspective", src, M, dsize, dst, flags, borderMode, borderValue)
