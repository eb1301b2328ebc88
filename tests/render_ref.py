"""numpy restatement of the three images Processor.run_detection writes per frame (src/processor.py:364-374 of the reference):

    result   im_helpers.to_rgb(255 * estimate_fixed)                   (im_helpers.py:162-200)
    flow     im_helpers.get_flow_vis(flow) = flow_vis.flow_to_color(flow, convert_to_bgr=True)
    phi      im_helpers.apply_colormap(to_rgb(phi, max_value=180.0)) = cv2.applyColorMap(..., COLORMAP_JET)

All three are (H, W, 3) u8 BGR, what the reference hands to cv2.imwrite.  Every expression keeps numpy 2's dtype rules: a float32
field (frame index 0, detector.py:80-81) stays float32 up to the wheel coordinate, `fk - k0` (float32 - int32) is float64.

flow_vis and cv2 are not installed here; the two images the reference wrote with them (media/colorwheel.png, media/colorbar.png,
copied to tests/golden/) pin this restatement: test_render_cpu.py.
"""
from __future__ import annotations

import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
COLORWHEEL_PNG = os.path.join(GOLDEN, "colorwheel.png")
COLORBAR_PNG = os.path.join(GOLDEN, "colorbar.png")


def decode_rgb(path: str) -> np.ndarray:
    """(H, W, 3) u8 RGB of an 8-bit RGB PNG (mavflow.frame_source.decode_png)."""
    from mavflow.frame_source import decode_png
    with open(path, "rb") as f:
        px, ctype = decode_png(f.read())
    assert ctype == 2 and px.ndim == 3 and px.shape[2] == 3, (ctype, px.shape)
    return px


def make_colorwheel() -> np.ndarray:
    """flow_vis.make_colorwheel: (55, 3) float64 RGB, the Middlebury wheel."""
    RY, YG, GC, CB, BM, MR = 15, 6, 4, 11, 13, 6
    wheel = np.zeros((RY + YG + GC + CB + BM + MR, 3))
    c = 0
    wheel[0:RY, 0] = 255
    wheel[0:RY, 1] = np.floor(255 * np.arange(0, RY) / RY)
    c += RY
    wheel[c:c + YG, 0] = 255 - np.floor(255 * np.arange(0, YG) / YG)
    wheel[c:c + YG, 1] = 255
    c += YG
    wheel[c:c + GC, 1] = 255
    wheel[c:c + GC, 2] = np.floor(255 * np.arange(0, GC) / GC)
    c += GC
    wheel[c:c + CB, 1] = 255 - np.floor(255 * np.arange(CB) / CB)
    wheel[c:c + CB, 2] = 255
    c += CB
    wheel[c:c + BM, 2] = 255
    wheel[c:c + BM, 0] = np.floor(255 * np.arange(0, BM) / BM)
    c += BM
    wheel[c:c + MR, 2] = 255 - np.floor(255 * np.arange(MR) / MR)
    wheel[c:c + MR, 0] = 255
    return wheel


def _nudge(a: np.ndarray, ulps: int) -> np.ndarray:
    """a moved by `ulps` units in the last place of its own type (negative: towards -inf)."""
    if ulps == 0:
        return a
    to = np.array(np.inf if ulps > 0 else -np.inf, a.dtype)
    for _ in range(abs(ulps)):
        a = np.nextafter(a, to)
    return a


def flow_to_color(flow: np.ndarray, atan2_ulps: int = 0) -> np.ndarray:
    """flow_vis.flow_to_color(flow, convert_to_bgr=True) of one (H, W, 2) field in its own float type.  atan2_ulps moves every
    arctan2 result by that many ulps (finds the pixels whose byte depends on the last bits of arctan2)."""
    u, v = flow[:, :, 0], flow[:, :, 1]
    rad = np.sqrt(np.square(u) + np.square(v))
    rad_max = np.max(rad)
    epsilon = 1e-5
    u = u / (rad_max + epsilon)
    v = v / (rad_max + epsilon)
    img = np.zeros((u.shape[0], u.shape[1], 3), np.uint8)
    wheel = make_colorwheel()
    ncols = wheel.shape[0]
    rad = np.sqrt(np.square(u) + np.square(v))
    a = _nudge(np.arctan2(-v, -u), atan2_ulps) / np.pi
    fk = (a + 1) / 2 * (ncols - 1)
    k0 = np.floor(fk).astype(np.int32)
    k1 = k0 + 1
    k1[k1 == ncols] = 0
    f = fk - k0
    for i in range(3):
        tmp = wheel[:, i]
        col0 = tmp[k0] / 255.0
        col1 = tmp[k1] / 255.0
        col = (1 - f) * col0 + f * col1
        idx = rad <= 1
        col[idx] = 1 - rad[idx] * (1 - col[idx])
        col[~idx] = col[~idx] * 0.75
        img[:, :, 2 - i] = np.floor(255 * col)
    return img


# cv2.COLORMAP_JET, BGR, entries 200..255: NOT pinned by any image the reference wrote.  Restated from OpenCV's Jet: red holds 255
# through entry 223 and then falls by 4 per entry to 128; green falls by 4 per entry from 92 to 0 at 223; blue is 0.
JET_TAIL = np.array([(0, max(0, 92 - 4 * (i - 200)), 255 if i < 224 else 252 - 4 * (i - 224)) for i in range(200, 256)], np.uint8)


def jet_head() -> np.ndarray:
    """JET entries 0..199 (BGR) from colorbar.png: cv2.applyColorMap(JET) of the rows 0..199 (im_helpers.py:212-222)."""
    rgb = decode_rgb(COLORBAR_PNG)
    assert rgb.shape == (200, 30, 3) and (rgb == rgb[:, :1]).all()
    return np.ascontiguousarray(rgb[:, 0, ::-1])


def jet_lut(tail: np.ndarray = JET_TAIL) -> np.ndarray:
    """(256, 3) u8 BGR: the pinned head and the given tail."""
    return np.concatenate([jet_head(), np.asarray(tail, np.uint8).reshape(56, 3)])


def to_int(img: np.ndarray, max_value=None) -> np.ndarray:
    """im_helpers.to_int(img, np.uint8, normalize=True, max_value)."""
    if max_value is None:
        max_value = np.max(img)
    elif max_value <= 0.0:
        max_value = 1.0
    with np.errstate(all="ignore"):
        return np.around(np.abs(img) * 255 / max_value).astype(np.uint8)


def result_image(estimate_fixed: np.ndarray) -> np.ndarray:
    """to_rgb(255 * estimate_fixed): GRAY2RGB of to_int(normalize=True); an empty mask is 0 / 0 -> NaN -> 0."""
    g = to_int(255 * np.asarray(estimate_fixed, bool))
    return np.repeat(g[:, :, None], 3, axis=2)


def phi_image(phi: np.ndarray, lut: np.ndarray | None = None) -> np.ndarray:
    """apply_colormap(to_rgb(phi, max_value=180.0)): phi in its own float type, then the JET LUT of the (equal) channels."""
    lut = jet_lut() if lut is None else lut
    return lut[to_int(phi, max_value=180.0)]


def colorwheel_field() -> np.ndarray:
    """The float64 disk im_helpers.get_colorwheel (:225-242) renders: (x - 125, y - 125) inside radius 125, zero outside."""
    diameter = 250
    radius = diameter / 2
    ys, xs = np.mgrid[0:diameter, 0:diameter]
    img = np.stack([xs - radius, ys - radius], axis=-1).astype(np.float64)
    img[np.sqrt((xs - radius) ** 2 + (ys - radius) ** 2) > radius] = 0
    return img


def atan2_sensitive(flow: np.ndarray, ulps: int = 2) -> np.ndarray:
    """(H, W) bool: pixels whose flow image changes when arctan2 moves by up to +-ulps."""
    base = flow_to_color(flow)
    out = np.zeros(base.shape[:2], bool)
    for k in range(1, ulps + 1):
        for s in (k, -k):
            out |= (flow_to_color(flow, s) != base).any(axis=2)
    return out
