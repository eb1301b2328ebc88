"""include/mavflow_shapes.h in plain scalar Python / numpy: what the device's shapes are compared with, byte for byte.  Every record is
restated as the header states it -- row spans as a closed form of the row -- and nothing is shared with the library.  The thickness-1
line is restated BY ROWS here (the header's closed form) and held to tests/vis_ref.py's pixel-by-pixel iterator by a CPU test."""
import math
import sys

import numpy as np

LINE, RECT, CIRCLE = 0, 1, 2
FILLED = -1
MAX_THICKNESS = 255
MAX_COORD = 1 << 20
XY_ONE = 1 << 16
HALF = XY_ONE >> 1
DBL_EPSILON = sys.float_info.epsilon

SHAPE_DTYPE = np.dtype([("kind", np.int32), ("image", np.int32), ("x0", np.int32), ("y0", np.int32), ("x1", np.int32), ("y1", np.int32),
                        ("thickness", np.int32), ("colour", np.uint8, (4,))])
assert SHAPE_DTYPE.itemsize == 32


def shape(kind, image, x0, y0, x1, y1, thickness, colour):
    c = tuple(int(v) for v in colour) + (0,) * (4 - len(colour))
    return (int(kind), int(image), int(x0), int(y0), int(x1), int(y1), int(thickness), c)


def table(records) -> np.ndarray:
    return np.array(list(records), dtype=SHAPE_DTYPE).reshape(-1)


def valid(s, batch: int) -> bool:
    """the records the header says are drawn (the others are skipped by the device form and refused by the host form)"""
    if not 0 <= int(s["image"]) < batch:
        return False
    if any(abs(int(s[k])) > MAX_COORD for k in ("x0", "y0", "x1", "y1")):
        return False
    t, kind = int(s["thickness"]), int(s["kind"])
    thick = 1 <= t <= MAX_THICKNESS
    if kind == LINE:
        return thick
    if kind == RECT:
        return thick or t == FILLED
    if kind == CIRCLE:
        return t == FILLED and int(s["x1"]) >= 0
    return False


def _tdiv(a: int, b: int) -> int:
    """the int64 quotient truncated toward zero"""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def clip_line(W, H, x1, y1, x2, y2):
    """cv::clipLine as include/mavflow_vis.h states it"""
    right, bottom = W - 1, H - 1
    c1 = (x1 < 0) + (x1 > right) * 2 + (y1 < 0) * 4 + (y1 > bottom) * 8
    c2 = (x2 < 0) + (x2 > right) * 2 + (y2 < 0) * 4 + (y2 > bottom) * 8
    if (c1 & c2) == 0 and (c1 | c2) != 0:
        if c1 & 12:
            a = 0 if c1 < 8 else bottom
            x1 += int(float(a - y1) * float(x2 - x1) / float(y2 - y1))
            y1 = a
            c1 = (x1 < 0) + (x1 > right) * 2
        if c2 & 12:
            a = 0 if c2 < 8 else bottom
            x2 += int(float(a - y2) * float(x2 - x1) / float(y2 - y1))
            y2 = a
            c2 = (x2 < 0) + (x2 > right) * 2
        if (c1 & c2) == 0 and (c1 | c2) != 0:
            if c1:
                a = 0 if c1 == 1 else right
                y1 += int(float(a - x1) * float(y2 - y1) / float(x2 - x1))
                x1 = a
                c1 = 0
            if c2:
                a = 0 if c2 == 1 else right
                y2 += int(float(a - x2) * float(y2 - y1) / float(x2 - x1))
                x2 = a
                c2 = 0
    return (c1 | c2) == 0, x1, y1, x2, y2


def thin_line_spans(W, H, x1, y1, x2, y2):
    """thickness 1, by rows: {y: [(xa, xb)]}"""
    ok, x1, y1, x2, y2 = clip_line(W, H, x1, y1, x2, y2)
    out = {}
    if not ok:
        return out
    dx, dy = x2 - x1, y2 - y1
    if dx < 0:
        dx, dy, x1, y1 = -dx, -dy, x2, y2
    sy = -1 if dy < 0 else 1
    dy = abs(dy)
    if dy > dx:
        for i in range(dy + 1):
            x = x1 + (2 * dx * i + dy - 1) // (2 * dy)
            out[y1 + sy * i] = [(x, x)]
    elif dy == 0:
        out[y1] = [(x1, x1 + dx)]
    else:
        for d in range(dy + 1):
            lo = 0 if d == 0 else (2 * dx * (d - 1) + dx) // (2 * dy) + 1
            hi = min((2 * dx * d + dx) // (2 * dy), dx)
            if lo <= hi:
                out[y1 + sy * d] = [(x1 + lo, x1 + hi)]
    return out


def disc_half_widths(r: int):
    h = [-1] * (r + 1)
    err, dx, dy, plus, minus = 0, r, 0, 1, 2 * r - 1
    while dx >= dy:
        h[dy] = max(h[dy], dx)
        h[dx] = max(h[dx], dy)
        dy += 1
        err += plus
        plus += 2
        if err > 0:
            err -= minus
            dx -= 1
            minus -= 2
    return h


def _add(out, y, span):
    out.setdefault(y, []).append(span)


def disc_spans(out, cx, cy, r, H):
    h = disc_half_widths(r)
    for y in range(max(cy - r, 0), min(cy + r, H - 1) + 1):
        k = abs(y - cy)
        if h[k] >= 0:
            _add(out, y, (cx - h[k], cx + h[k]))


def half_width_vector(x0, y0, x1, y1, t):
    """dp of the header, or None where the quadrilateral does not exist"""
    dx, dy = float(x0 - x1), float(y1 - y0)
    r = dx * dx + dy * dy
    if not r > DBL_EPSILON:
        return None
    s = (float(t << 15) + float((t & 1) << 15)) / math.sqrt(r)
    return int(np.rint(dy * s)), int(np.rint(dx * s))


def _chain_x(vx, rw, m, di, ymin, y):
    X, D, Y, ys, c = -XY_ONE, 0, ymin, ymin, 0
    while True:
        k = c + 1
        while k <= 3 and rw[(m + k * di) % 4] <= ys:
            k += 1
        if k > 3:
            break
        ty, xs, xe = rw[(m + k * di) % 4], vx[(m + (k - 1) * di) % 4], vx[(m + k * di) % 4]
        D = _tdiv((xe - xs) * 2 + (ty - ys), 2 * (ty - ys))
        X, Y, c = xs, ys, k
        if y < ty:
            break
        ys = ty
    return X + (y - Y) * D


def poly_spans(out, vx, vy, H):
    """the convex fill of four 16.16 vertices, rows ymin .. ymax"""
    rw = [(v + HALF) >> 16 for v in vy]
    m = 0
    for i in range(4):
        if vy[i] < vy[m]:
            m = i
    ymin, ymax = rw[m], max(rw)
    for y in range(max(ymin, 0), min(ymax, H - 1) + 1):
        xa, xb = _chain_x(vx, rw, m, 1, ymin, y), _chain_x(vx, rw, m, 3, ymin, y)
        if xa > xb:
            xa, xb = xb, xa
        _add(out, y, ((xa + HALF) >> 16, (xb + HALF) >> 16))


def line_spans(out, W, H, x0, y0, x1, y1, t):
    if t <= 1:
        for y, spans in thin_line_spans(W, H, x0, y0, x1, y1).items():
            for s in spans:
                _add(out, y, s)
        return
    dp = half_width_vector(x0, y0, x1, y1, t)
    if dp is not None:
        X0, Y0, X1, Y1 = x0 * XY_ONE, y0 * XY_ONE, x1 * XY_ONE, y1 * XY_ONE
        vx = [X0 + dp[0], X0 - dp[0], X1 - dp[0], X1 + dp[0]]
        vy = [Y0 + dp[1], Y0 - dp[1], Y1 - dp[1], Y1 + dp[1]]
        poly_spans(out, vx, vy, H)
    cap = (t * HALF + HALF) >> 16
    disc_spans(out, x0, y0, cap, H)
    disc_spans(out, x1, y1, cap, H)


def record_spans(s, W, H):
    """{row: [(xa, xb), ...]} of one valid record, rows inside the image, spans not yet clipped"""
    out = {}
    kind, t = int(s["kind"]), int(s["thickness"])
    x0, y0, x1, y1 = (int(s[k]) for k in ("x0", "y0", "x1", "y1"))
    if kind == LINE:
        line_spans(out, W, H, x0, y0, x1, y1, t)
    elif kind == RECT and t == FILLED:
        for y in range(max(min(y0, y1), 0), min(max(y0, y1), H - 1) + 1):
            _add(out, y, (min(x0, x1), max(x0, x1)))
    elif kind == RECT:
        for a, b in (((x0, y1), (x0, y0)), ((x0, y0), (x1, y0)), ((x1, y0), (x1, y1)), ((x1, y1), (x0, y1))):
            line_spans(out, W, H, a[0], a[1], b[0], b[1], t)
    elif kind == CIRCLE:
        disc_spans(out, x0, y0, x1, H)
    return out


def record_mask(s, W, H) -> np.ndarray:
    """(H, W) bool: the pixels of one valid record"""
    m = np.zeros((H, W), bool)
    for y, spans in record_spans(s, W, H).items():
        if 0 <= y < H:
            for xa, xb in spans:
                xa, xb = max(xa, 0), min(xb, W - 1)
                if xa <= xb:
                    m[y, xa:xb + 1] = True
    return m


def draw_shapes(img: np.ndarray, shapes: np.ndarray, n=None) -> np.ndarray:
    """a copy of img (batch, H, W, C) with records 0 .. n - 1 drawn in table order; n None: all; n < 0 or above len: none"""
    out = img.copy()
    B, H, W, C = out.shape
    n = len(shapes) if n is None else n
    if n < 0 or n > len(shapes):
        n = 0
    for s in shapes[:n]:
        if valid(s, B):
            out[int(s["image"])][record_mask(s, W, H)] = s["colour"][:C]
    return out


def owner_plane(shapes: np.ndarray, B, H, W) -> np.ndarray:
    """(B, H, W) int32: index + 1 of the last record that reaches a pixel, 0 where none does; and how many records reach it"""
    own, cnt = np.zeros((B, H, W), np.int32), np.zeros((B, H, W), np.int32)
    for i, s in enumerate(shapes):
        if valid(s, B):
            m = record_mask(s, W, H)
            own[int(s["image"])][m] = i + 1
            cnt[int(s["image"])][m] += 1
    return own, cnt


def add_saturate(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    return np.minimum(a.astype(np.int32) + b.astype(np.int32), 255).astype(np.uint8)


def mosaic(tiles, rows, cols, B, H, W) -> np.ndarray:
    """tiles: rows * cols entries, (B, H, W), (B, H, W, 1), (B, H, W, 3) or None -> (B, rows * H, cols * W, 3)"""
    def rgb(t):
        if t is None:
            return np.zeros((B, H, W, 3), np.uint8)
        t = t.reshape(B, H, W, -1)
        return np.repeat(t, 3, axis=3) if t.shape[3] == 1 else t
    return np.stack([np.vstack([np.hstack([rgb(tiles[r * cols + c])[b] for c in range(cols)]) for r in range(rows)]) for b in range(B)])


def shapes_from_blobs(blobs, counts, max_blobs, thickness, colour) -> np.ndarray:
    """blobs: per image a list of (x, y, w, h); counts: n_blobs per image"""
    recs = []
    for b, (bl, n) in enumerate(zip(blobs, counts)):
        for x, y, w, h in list(bl)[:min(max(int(n), 0), max_blobs)]:
            recs.append(shape(RECT, b, x, y, x + w - 1, y + h - 1, thickness, colour))
    return table(recs) if recs else np.zeros(0, SHAPE_DTYPE)
