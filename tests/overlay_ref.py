"""Numpy restatement of the frame the reference's detection loop writes to processed.mp4 (src/processor.py:376-392), the bar that
mav_overlay / Processor(processed_path=...) are held to.

Per frame, with orig_frame the BGR u8 frame, estimate_fixed the fixed mask, FoE_dense and FoE_gt:
  1. draw_FoE(orig_frame, FoE_dense, [0, 255, 0]), then draw_FoE(orig_frame, FoE_gt, [255, 255, 255]) -- white over green.
     draw_FoE (src/focus_of_expansion.py:186-201) is cv2.circle(frame, (int(x), int(y)), 10, color, -1): a filled disc, LINE_8,
     shift 0, drawn in place.  int() truncates toward zero.  The disc is skipped when |x| > 1e9 or |y| > 1e9, or when a coordinate IS
     the np.nan object; any other NaN makes int() raise ValueError.
  2. The same two discs on result_img = to_rgb(255 * estimate_fixed), after that image was written: it only decides step 3.
  3. The frame is written only if np.sum(result_img) > 0: the mask is non-empty or a disc has a pixel inside the image.
  4. mask_rgb = copy(orig_frame) (discs included), mask_rgb[estimate_fixed] = (150, 0, 150).
  5. mask_vis = cv2.addWeighted(orig_frame, 0.2, mask_rgb, 0.8, 0.0): the frame that goes to the video.

The blend.  cv2.addWeighted on u8 computes p * 0.2f + q * 0.8f (+ 0.0f) in float32 and rounds to the nearest byte.  The exact value
0.2 p + 0.8 q = (p + 4 q) / 5 has a fractional part in {0, .2, .4, .6, .8}: never near .5, so float32 rounding, FMA against separate
multiply-add and SIMD lane order cannot move the rounded byte, which is round((p + 4 q) / 5) = (p + 4 q + 2) // 5 (no ties).  Outside
the mask q == p and the byte is p.  tests/test_overlay_cpu.py checks this over all 65 536 (p, q) pairs.

The disc.  cv2.circle with thickness -1, LINE_8 and shift 0 takes OpenCV's integer midpoint routine Circle(..., fill=1)
(drawing.cpp): from err = 0, dx = r, dy = 0, plus = 1, minus = 2r - 1 it emits horizontal spans [cx +- dx] on rows cy +- dy and
[cx +- dy] on rows cy +- dx while dx >= dy; spans are clipped to the image and rows outside it are skipped (a span that lies wholly
outside is skipped too, which removes no pixel of the image).  A row is therefore the widest span emitted on it.  For r = 10 the
half-widths by row offset 0..10 are 10 9 9 9 9 8 8 7 6 4 0 (317 pixels).  This routine is restated from memory of the published
source: NO image the reference wrote pins it (like JET entries 200-255).  HALF_WIDTHS_R10 pins this restatement's own
table so that a later edit cannot change it silently."""
from __future__ import annotations

import numpy as np

HALF_WIDTHS_R10 = (10, 9, 9, 9, 9, 8, 8, 7, 6, 4, 0)
GREEN, WHITE, PURPLE = (0, 255, 0), (255, 255, 255), (150, 0, 150)       # BGR
GUARD = 1e9


def half_widths(r: int) -> list:
    """Half-width of each row offset 0..r of the filled midpoint disc of radius r."""
    if r < 0:
        raise ValueError("radius must be >= 0")
    h = [-1] * (r + 1)
    err, dx, dy, plus, minus = 0, r, 0, 1, 2 * r - 1
    while dx >= dy:
        h[dy] = max(h[dy], dx)                   # spans [cx +- dx] on rows cy +- dy
        h[dx] = max(h[dx], dy)                   # spans [cx +- dy] on rows cy +- dx
        dy += 1
        err += plus
        plus += 2
        if err > 0:
            err -= minus
            dx -= 1
            minus -= 2
    assert min(h) >= 0
    return h


def centre(foe):
    """(cx, cy) draw_FoE draws at, or None when it draws nothing.  Raises ValueError for a NaN that is not the np.nan object."""
    x, y = foe[0], foe[1]
    if x is np.nan or y is np.nan or np.abs(x) > GUARD or np.abs(y) > GUARD:
        return None
    return int(x), int(y)


def disc(H: int, W: int, cx: int, cy: int, r: int) -> np.ndarray:
    """(H, W) bool: the pixels of the clipped filled disc."""
    out = np.zeros((H, W), bool)
    for k, h in enumerate(half_widths(r)):
        for y in {cy - k, cy + k}:
            if 0 <= y < H:
                x0, x1 = max(cx - h, 0), min(cx + h, W - 1)
                if x0 <= x1:
                    out[y, x0:x1 + 1] = True
    return out


def disc_of(H: int, W: int, foe, r: int = 10) -> np.ndarray:
    c = centre(foe)
    return np.zeros((H, W), bool) if c is None else disc(H, W, c[0], c[1], r)


def draw(frame: np.ndarray, foe, color, r: int = 10) -> np.ndarray:
    """draw_FoE in place on an (H, W, 3) u8 array."""
    frame[disc_of(frame.shape[0], frame.shape[1], foe, r)] = color
    return frame


def blend(p: np.ndarray, q: np.ndarray) -> np.ndarray:
    """cv2.addWeighted(p, 0.2, q, 0.8, 0.0) of u8 arrays (see the module docstring)."""
    return ((p.astype(np.int32) + 4 * q.astype(np.int32) + 2) // 5).astype(np.uint8)


def overlay(frame: np.ndarray, mask: np.ndarray, foe, foe_gt, r: int = 10):
    """(mask_vis (H, W, 3) u8, written) of one frame; `frame` is not modified."""
    orig = np.array(frame, np.uint8, copy=True)
    mask = np.asarray(mask).astype(bool)
    H, W = mask.shape
    g, w = disc_of(H, W, foe, r), disc_of(H, W, foe_gt, r)
    orig[g] = GREEN
    orig[w] = WHITE
    written = bool(mask.any() or g.any() or w.any())          # np.sum(to_rgb(255 * mask) with both discs) > 0
    mask_rgb = orig.copy()
    mask_rgb[mask] = PURPLE
    return blend(orig, mask_rgb), written


def overlay_batch(frames, masks, foes, foe_gts, r: int = 10):
    outs = [overlay(f, m, a, b, r) for f, m, a, b in zip(frames, masks, foes, foe_gts)]
    return np.stack([o for o, _ in outs]), np.array([w for _, w in outs])
