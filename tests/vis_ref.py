"""include/mavflow_vis.h in numpy: what the device's flow pictures are compared with, byte for byte.  MAV_HSV_PROCESS and HSV -> BGR are
defined by mavflow.farneback.flow_to_hsv / hsv_to_bgr themselves and are not restated here; this file has draw_hsv's HSV stage,
BGR -> HSV, clip_line, line_pixels and draw_flow.  tests/golden/vis.npz (tools/gen_vis_fixtures.py) holds what the reference's own lines
give for draw_hsv's HSV image and draw_flow's line and centre lists."""
import numpy as np

HSV_SHIFT = 12
CLAMP = float(1 << 30)


def draw_hsv_stage(flow: np.ndarray) -> np.ndarray:
    """Farneback.draw_hsv (src/farneback.py:50-58) up to the colour conversion: the HSV image of a float32 field"""
    fx, fy = flow[..., 0], flow[..., 1]
    assert fx.dtype == np.float32
    ang = np.arctan2(fy, fx) + np.float32(np.pi)
    v = np.sqrt(fx * fx + fy * fy)
    hsv = np.zeros(flow.shape[:-1] + (3,), np.uint8)
    hsv[..., 0] = (ang * np.float32(180 / np.pi / 2)).astype(np.int32) & 255
    hsv[..., 1] = 255
    hsv[..., 2] = np.minimum(v * np.float32(4), np.float32(255)).astype(np.int32) & 255
    return hsv


def draw_hue_float(flow: np.ndarray) -> np.ndarray:
    """the hue of draw_hsv_stage before it is cut to a whole number (the tests' margin is taken on it)"""
    return (np.arctan2(flow[..., 1], flow[..., 0]) + np.float32(np.pi)) * np.float32(180 / np.pi / 2)


def process_hue_float(flow: np.ndarray) -> np.ndarray:
    """the hue of mavflow.farneback.flow_to_hsv before it is cut to a whole number"""
    ang = np.arctan2(flow[..., 1], flow[..., 0]).astype(np.float32)
    ang = np.where(ang < 0, ang + np.float32(2 * np.pi), ang)
    return ang * 180 / np.pi / 2


def div_tables():
    """sdiv[i] = rint((255 << 12) / i), hdiv[i] = rint((180 << 12) / (6 i)) in double, entry 0 = 0"""
    i = np.arange(1, 256, dtype=np.float64)
    sdiv, hdiv = np.zeros(256, np.int64), np.zeros(256, np.int64)
    sdiv[1:] = np.rint((255 << HSV_SHIFT) / i).astype(np.int64)
    hdiv[1:] = np.rint((180 << HSV_SHIFT) / (6.0 * i)).astype(np.int64)
    return sdiv, hdiv


def bgr2hsv(bgr: np.ndarray) -> np.ndarray:
    """COLOR_BGR2HSV on uint8 (.., 3): OpenCV's integer path as include/mavflow_vis.h states it"""
    sdiv, hdiv = div_tables()
    b, g, r = (bgr[..., k].astype(np.int64) for k in range(3))
    v = np.maximum(b, np.maximum(g, r))
    d = v - np.minimum(b, np.minimum(g, r))
    s = (d * sdiv[v] + (1 << (HSV_SHIFT - 1))) >> HSV_SHIFT
    h = np.where(v == r, g - b, np.where(v == g, b - r + 2 * d, r - g + 4 * d))
    h = (h * hdiv[d] + (1 << (HSV_SHIFT - 1))) >> HSV_SHIFT               # numpy's >> on int64 is arithmetic
    h = np.where(h < 0, h + 180, h)
    return np.stack([h, s, v], -1).astype(np.uint8)


def flow_radial(bgr: np.ndarray, hsv_to_bgr) -> np.ndarray:
    """im_helpers.get_flow_radial: the composition the fused launch must equal"""
    hsv = bgr2hsv(bgr)
    hsv[..., 1] = 255
    hsv[..., 2] = 255
    return hsv_to_bgr(hsv)


def _trunc(x: float) -> int:
    return int(x)                                                         # toward zero, as (int64) of a double


def clip_line(W: int, H: int, p1, p2):
    """cv::clipLine on integer points -> (accepted, (x1, y1), (x2, y2))"""
    x1, y1, x2, y2 = int(p1[0]), int(p1[1]), int(p2[0]), int(p2[1])
    right, bottom = W - 1, H - 1
    c1 = (x1 < 0) + (x1 > right) * 2 + (y1 < 0) * 4 + (y1 > bottom) * 8
    c2 = (x2 < 0) + (x2 > right) * 2 + (y2 < 0) * 4 + (y2 > bottom) * 8
    if (c1 & c2) == 0 and (c1 | c2) != 0:
        if c1 & 12:
            a = 0 if c1 < 8 else bottom
            x1 += _trunc(float(a - y1) * float(x2 - x1) / float(y2 - y1))
            y1 = a
            c1 = (x1 < 0) + (x1 > right) * 2
        if c2 & 12:
            a = 0 if c2 < 8 else bottom
            x2 += _trunc(float(a - y2) * float(x2 - x1) / float(y2 - y1))
            y2 = a
            c2 = (x2 < 0) + (x2 > right) * 2
        if (c1 & c2) == 0 and (c1 | c2) != 0:
            if c1:
                a = 0 if c1 == 1 else right
                y1 += _trunc(float(a - x1) * float(y2 - y1) / float(x2 - x1))
                x1 = a
                c1 = 0
            if c2:
                a = 0 if c2 == 1 else right
                y2 += _trunc(float(a - x2) * float(y2 - y1) / float(x2 - x1))
                x2 = a
                c2 = 0
    return (c1 | c2) == 0, (x1, y1), (x2, y2)


def line_pixels(p1, p2):
    """cv::LineIterator, 8-connected, left to right, on a segment inside the image: the list of (x, y)"""
    x1, y1, x2, y2 = int(p1[0]), int(p1[1]), int(p2[0]), int(p2[1])
    dx, dy = x2 - x1, y2 - y1
    if dx < 0:
        dx, dy, x1, y1 = -dx, -dy, x2, y2
    sy = -1 if dy < 0 else 1
    dy = abs(dy)
    steep = dy > dx
    major, minor = (dy, dx) if steep else (dx, dy)
    err, x, y, out = major - 2 * minor, x1, y1, []
    for _ in range(major + 1):
        out.append((x, y))
        diag = err < 0
        err += -2 * minor + (2 * major if diag else 0)
        if steep:
            y += sy
            x += 1 if diag else 0
        else:
            x += 1
            y += sy if diag else 0
    return out


def grid_points(W: int, H: int, step: int):
    """np.mgrid[step//2:h:step, step//2:w:step] as (y, x) int32 lists in the reference's order"""
    y, x = np.mgrid[step // 2:H:step, step // 2:W:step].reshape(2, -1).astype(np.int32)
    return y, x


def flow_lines(flow: np.ndarray, step: int, threshold):
    """draw_flow's `lines` array (src/farneback.py:29-42) with the header's clamp: (n, 2, 2) int32 [[x, y], [x + fx, y + fy]]"""
    H, W = flow.shape[:2]
    y, x = grid_points(W, H, step)
    fx, fy = flow[y, x].T
    mask = np.sqrt(fx * fx + fy * fy) > np.float32(threshold)
    x, y, fx, fy = x[mask], y[mask], fx[mask], fy[mask]
    lines = np.vstack([x, y, x + fx.astype(np.float64), y + fy.astype(np.float64)]).T.reshape(-1, 2, 2)
    return np.clip(lines + 0.5, -CLAMP, CLAMP).astype(np.int32)


def draw_flow(img: np.ndarray, flow: np.ndarray, step: int = 8, threshold=1.0, colour=(0, 255, 0)) -> np.ndarray:
    """Farneback.draw_flow on a copy of img: cv2.polylines of every line (clip_line, line_pixels), then cv2.circle(.., 1, .., -1)"""
    out = img.copy()
    H, W = out.shape[:2]
    col = np.asarray(colour, np.uint8)
    for (xa, ya), (xb, yb) in flow_lines(flow, step, threshold):
        ok, q1, q2 = clip_line(W, H, (xa, ya), (xb, yb))
        if ok:
            for px, py in line_pixels(q1, q2):
                out[py, px] = col
        for px, py in ((xa - 1, ya), (xa, ya), (xa + 1, ya), (xa, ya - 1), (xa, ya + 1)):
            if 0 <= px < W and 0 <= py < H:
                out[py, px] = col
    return out
