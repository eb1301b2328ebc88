"""Shapes on the device (include/mavflow_shapes.h): a table of lines, rectangles and filled circles drawn in table order, cv2.add, blob
boxes and the tile mosaic, as methods of _lib.Context (draw_shapes, draw_shapes_enqueue, draw_blob_boxes, add_saturate,
add_saturate_enqueue, mosaic, mosaic_enqueue) and `line`, `rectangle`, `circle`, `add` with cv2's signatures.  The library is _lib's
(same loader, no CPU fallback).  The thick line is OpenCV 4.x ThickLine as remembered and pinned to no cv2 build: the header is the
definition and lists what to re-check first."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import Context, _dev_ptr, _ptr, check

EXPORTS = _lib.SHAPES_EXPORTS

LINE, RECT, CIRCLE = 0, 1, 2                                        # MAV_SHAPE_*
FILLED = -1
MAX_THICKNESS = 255
MAX_COORD = 1 << 20
FORM_ORDERED, FORM_DIRECT = 0, 1                                    # MAV_SHAPES_FORM_*
FORM_BYTES, FORM_WORDS = 0, 1
MOSAIC_MAX_TILES = 16
LINE_4, LINE_8, LINE_AA = 4, 8, 16                                  # cv2's values

SHAPE_DTYPE = np.dtype([("kind", np.int32), ("image", np.int32), ("x0", np.int32), ("y0", np.int32), ("x1", np.int32), ("y1", np.int32),
                        ("thickness", np.int32), ("colour", np.uint8, (4,))])
assert SHAPE_DTYPE.itemsize == 32


def _colour4(color, channels=3):
    """cv2's scalar: a number or up to four of them, saturated to uint8 -> four bytes"""
    c = np.atleast_1d(np.asarray(color, np.float64)).reshape(-1)
    if c.size < 1 or c.size > 4 or not np.all(np.isfinite(c)):
        raise ValueError(f"color must be one to four finite numbers, got {color!r}")
    out = np.zeros(4, np.uint8)
    out[:c.size] = np.clip(np.rint(c), 0, 255).astype(np.uint8)
    return out


def shape(kind, x0, y0, x1, y1, thickness, color, image: int = 0):
    """one record of a table (a tuple np.array(.., SHAPE_DTYPE) takes)"""
    return (int(kind), int(image), int(x0), int(y0), int(x1), int(y1), int(thickness), tuple(int(v) for v in _colour4(color)))


def table(records) -> np.ndarray:
    """records (tuples of shape(), or a SHAPE_DTYPE array) -> a contiguous SHAPE_DTYPE array"""
    if isinstance(records, np.ndarray) and records.dtype == SHAPE_DTYPE:
        return np.ascontiguousarray(records.reshape(-1))
    return np.array(list(records), dtype=SHAPE_DTYPE).reshape(-1)


def shapes_form(shapes, channels: int = 3) -> int:
    """mav_shapes_form: FORM_DIRECT when every record carries the same colour, else FORM_ORDERED"""
    t = table(shapes)
    return int(_lib.load().mav_shapes_form(_ptr(t) if len(t) else None, len(t), int(channels)))


def bytes_form(n: int, a=None, b=None, dst=None) -> int:
    """mav_bytes_form: FORM_WORDS / FORM_BYTES of an add or a mosaic of n bytes with these pointers (ints, or None)"""
    return int(_lib.load().mav_bytes_form(int(n), a, b, dst))


def scratch_bytes(W: int, H: int, batch: int) -> int:
    return int(_lib.load().mav_shapes_scratch_bytes(int(W), int(H), int(batch)))


def _images(self, img, what="img"):
    """img (H, W), (H, W, C) or (B, H, W, C) uint8 of this context's frame, C 1 or 3 -> (array, batch, channels)"""
    a = np.asarray(img)
    H, W = self.H, self.W
    if a.dtype != np.uint8:
        raise TypeError(f"{what} must be uint8, got {a.dtype}")
    if a.shape == (H, W):
        return a, 1, 1
    if a.ndim == 3 and a.shape[:2] == (H, W) and a.shape[2] in (1, 3):
        return a, 1, int(a.shape[2])
    if a.ndim == 4 and a.shape[1:3] == (H, W) and a.shape[3] in (1, 3):
        return a, int(a.shape[0]), int(a.shape[3])
    raise ValueError(f"{what} has shape {a.shape}; this context's frame is {W} x {H}: (H, W), (H, W, C) or (B, H, W, C), C 1 or 3")


def _draw_shapes(self, img, shapes) -> np.ndarray:
    """Draw the table (shape() records or a SHAPE_DTYPE array) into img in table order, as the same cv2 calls in that order would: a
    pixel several records reach carries the last one's colour.  img (H, W[, C]) or (B, H, W, C) uint8 is drawn into and returned.  A
    record the library would skip (include/mavflow_shapes.h) is a ValueError naming it."""
    a, B, ch = _images(self, img)
    if not (isinstance(img, np.ndarray) and img.flags.writeable):
        raise TypeError("img must be a writeable numpy array: it is drawn into")
    t = table(shapes)
    work = a if a.flags.c_contiguous else np.ascontiguousarray(a)
    check(self.lib.mav_draw_shapes(self.h, _ptr(work), ch, B, _ptr(t) if len(t) else None, len(t)))
    if work is not a:
        img[...] = work
    return img


def _draw_shapes_enqueue(self, img_ptr, shapes_ptr, n_max: int, channels: int = 3, batch: int = 1, n_ptr=None, scratch_ptr=None) -> None:
    """mav_draw_shapes_dev: img (batch, H, W, channels) uint8 and n_max records in device memory; n_ptr: None or the device's int32
    count; scratch_ptr: scratch_bytes(W, H, batch) bytes for the ordered form, or None -- the promise that overlapping records share a
    colour.  Enqueue only."""
    check(self.lib.mav_draw_shapes_dev(self.h, _dev_ptr(img_ptr), int(channels), int(batch), _dev_ptr(shapes_ptr), int(n_max),
                                       None if n_ptr is None else _dev_ptr(n_ptr), None if scratch_ptr is None else _dev_ptr(scratch_ptr)))


def _shapes_from_blobs_enqueue(self, blobs_ptr, counts_ptr, batch: int, max_blobs: int, out_ptr, n_out_ptr, thickness: int = 2,
                               color=(0, 0, 255)) -> None:
    """mav_shapes_from_blobs_dev: the blob tables of components_dev -> RECT records in out (batch * max_blobs of them) and their count"""
    check(self.lib.mav_shapes_from_blobs_dev(self.h, _dev_ptr(blobs_ptr), _dev_ptr(counts_ptr), int(batch), int(max_blobs), int(thickness),
                                             _ptr(_colour4(color)), _dev_ptr(out_ptr), _dev_ptr(n_out_ptr)))


def _draw_blob_boxes(self, img, cc=None, thickness: int = 2, color=(0, 0, 255), connectivity: int = 8, min_area: int = 1,
                     max_blobs: int = 256, mask=None) -> np.ndarray:
    """The boxes of the blobs of `mask` ((B, H, W) or (H, W), any non-zero byte set) drawn onto img ((B, H, W, C) or (H, W[, C]), drawn
    into and returned): components, blob records -> rectangles and the drawing are enqueued back to back and no table visits the host.
    `cc` may be given instead of mask: the dict Context.components returned for the same batch (its records go up once)."""
    a, B, ch = _images(self, img)
    if not (isinstance(img, np.ndarray) and img.flags.writeable):
        raise TypeError("img must be a writeable numpy array: it is drawn into")
    if (cc is None) == (mask is None):
        raise ValueError("give either cc (the result of Context.components) or mask")
    work = np.ascontiguousarray(a)
    cb, bb = _lib.CC_COUNTS_DTYPE.itemsize, _lib.BLOB_DTYPE.itemsize
    if cc is not None:
        blobs = cc["blobs"]
        if len(blobs) != B:
            raise ValueError(f"cc holds {len(blobs)} images and img {B}")
        max_blobs = max(1, max(len(b) for b in blobs))
        counts = np.zeros(B, _lib.CC_COUNTS_DTYPE)
        tab = np.zeros((B, max_blobs), _lib.BLOB_DTYPE)
        for i, b in enumerate(blobs):
            counts["n_blobs"][i] = counts["n_components"][i] = len(b)
            tab[i, :len(b)] = b
    o_counts = 0
    o_blobs = (cb * B + 15) // 16 * 16
    o_shapes = o_blobs + (bb * B * max_blobs + 15) // 16 * 16
    o_n = o_shapes + 32 * B * max_blobs
    o_img = o_n + 16
    o_mask = o_img + (work.nbytes + 15) // 16 * 16
    blk = self.alloc(o_mask + (B * self.H * self.W if mask is not None else 0))
    try:
        check(self.lib.mav_memcpy_h2d(self.h, blk.ptr + o_img, _ptr(work), work.nbytes))
        if cc is not None:
            check(self.lib.mav_memcpy_h2d(self.h, blk.ptr + o_counts, _ptr(counts), counts.nbytes))
            check(self.lib.mav_memcpy_h2d(self.h, blk.ptr + o_blobs, _ptr(tab), tab.nbytes))
        else:
            m = np.asarray(mask)
            m = np.ascontiguousarray(m.view(np.uint8) if m.dtype == np.bool_ else m).reshape(B, self.H, self.W)
            if m.dtype != np.uint8:
                raise TypeError(f"mask must be bool or uint8, got {m.dtype}")
            check(self.lib.mav_memcpy_h2d(self.h, blk.ptr + o_mask, _ptr(m), m.nbytes))
            self.components_dev(blk.ptr + o_mask, B, blk.ptr + o_counts, blk.ptr + o_blobs, connectivity=connectivity, min_area=min_area,
                                max_blobs=max_blobs)
        _shapes_from_blobs_enqueue(self, blk.ptr + o_blobs, blk.ptr + o_counts, B, max_blobs, blk.ptr + o_shapes, blk.ptr + o_n, thickness, color)
        _draw_shapes_enqueue(self, blk.ptr + o_img, blk.ptr + o_shapes, B * max_blobs, ch, B, n_ptr=blk.ptr + o_n)
        check(self.lib.mav_memcpy_d2h(self.h, _ptr(work), blk.ptr + o_img, work.nbytes))
    finally:
        blk.free()
    if work is not a:
        img[...] = work
    return img


def _add_saturate(self, a, b) -> np.ndarray:
    """cv2.add(a, b) of two uint8 images of this context's frame, (H, W[, C]) or (B, H, W, C), C <= 4"""
    x, y = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if x.dtype != np.uint8 or y.dtype != np.uint8:
        raise TypeError(f"add takes uint8 images, got {x.dtype} and {y.dtype}")
    if x.shape != y.shape:
        raise ValueError(f"add of shapes {x.shape} and {y.shape}")
    H, W = self.H, self.W
    if x.shape[:2] == (H, W) and x.ndim in (2, 3):
        B, ch = 1, 1 if x.ndim == 2 else int(x.shape[2])
    elif x.ndim == 4 and x.shape[1:3] == (H, W):
        B, ch = int(x.shape[0]), int(x.shape[3])
    else:
        raise ValueError(f"images of shape {x.shape}; this context's frame is {W} x {H}")
    dst = np.empty_like(x)
    check(self.lib.mav_add_saturate(self.h, _ptr(x), _ptr(y), ch, B, _ptr(dst)))
    return dst


def _add_saturate_enqueue(self, a_ptr, b_ptr, dst_ptr, channels: int = 3, batch: int = 1) -> None:
    """mav_add_saturate_dev: a, b, dst (batch, H, W, channels) uint8 in device memory (dst may be a or b); enqueue only"""
    check(self.lib.mav_add_saturate_dev(self.h, _dev_ptr(a_ptr), _dev_ptr(b_ptr), int(channels), int(batch), _dev_ptr(dst_ptr)))


def _tile_args(tiles, rows, cols, channels):
    if rows < 1 or cols < 1 or rows * cols > MOSAIC_MAX_TILES or len(tiles) != rows * cols:
        raise ValueError(f"{len(tiles)} tiles for {rows} x {cols}; at most {MOSAIC_MAX_TILES} in all")
    ptrs = (C.c_void_p * (rows * cols))(*[None if t is None else t for t in tiles])
    chs = (C.c_int * (rows * cols))(*[int(c) for c in channels])
    return ptrs, chs


def _mosaic(self, tiles, rows: int, cols: int) -> np.ndarray:
    """np.vstack of the rows' np.hstack of rows * cols tiles of this context's frame, row after row: each (H, W), (H, W, C) or
    (B, H, W, C) uint8 with C 1 (replicated, GRAY2RGB) or 3, or None (black) -> (B, rows * H, cols * W, 3), or (rows * H, cols * W, 3)
    when no tile has a batch axis."""
    arrs, B, single = [], None, True
    for t in tiles:
        if t is None:
            arrs.append((None, 3))
            continue
        a, b, ch = _images(self, t, "tile")
        single = single and np.asarray(t).ndim < 4
        if B not in (None, b):
            raise ValueError(f"tiles of {B} and of {b} images")
        B = b
        arrs.append((np.ascontiguousarray(a), ch))
    if B is None:
        raise ValueError("every tile is None")
    ptrs, chs = _tile_args([None if a is None else a.ctypes.data for a, _ in arrs], int(rows), int(cols), [c for _, c in arrs])
    out = np.empty((B, rows * self.H, cols * self.W, 3), np.uint8)
    check(self.lib.mav_mosaic(self.h, ptrs, chs, int(rows), int(cols), B, _ptr(out)))
    return out[0] if single else out


def _mosaic_enqueue(self, tile_ptrs, tile_channels, rows: int, cols: int, out_ptr, batch: int = 1) -> None:
    """mav_mosaic_dev: tile_ptrs: rows * cols device pointers (or None: black) of (batch, H, W, tile_channels[i]) uint8; out
    (batch, rows * H, cols * W, 3) in device memory; enqueue only"""
    ptrs, chs = _tile_args([None if t is None else _dev_ptr(t) for t in tile_ptrs], int(rows), int(cols), tile_channels)
    check(self.lib.mav_mosaic_dev(self.h, ptrs, chs, int(rows), int(cols), int(batch), _dev_ptr(out_ptr)))


def _motion_pictures_enqueue(self, batch: int = 1, flow_ptr=None, field_ptr=None, img_flow_ptr=None, img_warped_ptr=None, img_global_ptr=None) -> None:
    """mav_motion_pictures_dev: get_flow_vis of the device flow and of the resident global-motion call's warped and global fields, into
    (batch, H, W, 3) device pictures (each optional); field_ptr: batch * H * W * 2 floats of scratch for the latter two"""
    o = [None if p is None else _dev_ptr(p) for p in (flow_ptr, field_ptr, img_flow_ptr, img_warped_ptr, img_global_ptr)]
    check(self.lib.mav_motion_pictures_dev(self.h, o[0], int(batch), o[1], o[2], o[3], o[4]))


Context.motion_pictures_enqueue = _motion_pictures_enqueue
Context.draw_shapes = _draw_shapes
Context.draw_shapes_enqueue = _draw_shapes_enqueue
Context.shapes_from_blobs_enqueue = _shapes_from_blobs_enqueue
Context.draw_blob_boxes = _draw_blob_boxes
Context.add_saturate = _add_saturate
Context.add_saturate_enqueue = _add_saturate_enqueue
Context.mosaic = _mosaic
Context.mosaic_enqueue = _mosaic_enqueue


# ---- cv2's signatures ----------------------------------------------------------------------------------------------------------------------
def _point(pt, what):
    p = tuple(pt)
    if len(p) != 2 or any(isinstance(v, float) and not float(v).is_integer() for v in p):
        raise TypeError(f"{what} must be a pair of integers, got {pt!r}")
    return int(p[0]), int(p[1])


def _cv_args(img, thickness, lineType, shift, what):
    if lineType == LINE_AA:
        raise NotImplementedError(f"{what} with LINE_AA is not built: LINE_8 (the default) is")
    if lineType not in (LINE_8, None):
        raise NotImplementedError(f"{what} with lineType {lineType} is not built: LINE_8 (the default) is")
    if shift:
        raise NotImplementedError(f"{what} with shift {shift} is not built: shift 0 is")
    a = np.asarray(img)
    if not isinstance(img, np.ndarray) or a.dtype != np.uint8 or a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] not in (1, 3)):
        raise NotImplementedError(f"{what} into {type(img).__name__} {getattr(a, 'dtype', '')} {getattr(a, 'shape', '')} is not built: "
                                  "an (H, W), (H, W, 1) or (H, W, 3) uint8 array is")
    return int(thickness)


def _draw_one(img, record):
    from . import im_helpers
    return im_helpers._ctx(img.shape[1], img.shape[0]).draw_shapes(img, [record])


def line(img, pt1, pt2, color, thickness=1, lineType=LINE_8, shift=0):
    """cv2.line: drawn into img and returned.  LINE_8 and shift 0 are built, thickness 1 .. 255."""
    t = _cv_args(img, thickness, lineType, shift, "line")
    if not 1 <= t <= MAX_THICKNESS:
        raise ValueError(f"line: thickness {thickness} outside [1, {MAX_THICKNESS}]")
    return _draw_one(img, shape(LINE, *_point(pt1, "pt1"), *_point(pt2, "pt2"), t, color))


def rectangle(img, pt1, pt2, color, thickness=1, lineType=LINE_8, shift=0):
    """cv2.rectangle(img, pt1, pt2, ...): thickness 1 .. 255, or any negative one (cv2.FILLED) for the filled box"""
    t = _cv_args(img, thickness, lineType, shift, "rectangle")
    if t < 0:
        t = FILLED
    elif not 1 <= t <= MAX_THICKNESS:
        raise ValueError(f"rectangle: thickness {thickness} outside [1, {MAX_THICKNESS}] and not negative (filled)")
    return _draw_one(img, shape(RECT, *_point(pt1, "pt1"), *_point(pt2, "pt2"), t, color))


def circle(img, center, radius, color, thickness=1, lineType=LINE_8, shift=0):
    """cv2.circle for the filled disc (a negative thickness); an outlined circle is not built"""
    t = _cv_args(img, thickness, lineType, shift, "circle")
    if t >= 0:
        raise NotImplementedError("an outlined circle (thickness >= 0) is not built: the filled one (thickness -1) is")
    if int(radius) < 0:
        raise ValueError(f"circle: radius {radius} < 0")
    cx, cy = _point(center, "center")
    return _draw_one(img, shape(CIRCLE, cx, cy, int(radius), 0, FILLED, color))


def add(src1, src2, dst=None, mask=None, dtype=None):
    """cv2.add of two uint8 images of one shape (saturating); mask and dtype are not built"""
    if mask is not None or dtype not in (None, -1):
        raise NotImplementedError("add with a mask or a dtype is not built: two uint8 images of one shape are")
    a, b = np.asarray(src1), np.asarray(src2)
    if a.dtype != np.uint8 or b.dtype != np.uint8 or a.shape != b.shape or a.ndim not in (2, 3):
        raise NotImplementedError(f"add of {a.dtype} {a.shape} and {b.dtype} {b.shape} is not built: two uint8 images of one shape are")
    from . import im_helpers
    res = im_helpers._ctx(a.shape[1], a.shape[0]).add_saturate(a, b)
    if dst is None:
        return res
    dst[...] = res
    return dst
