"""TEST INFRASTRUCTURE -- include/mavflow_resize.h in numpy: the dispatch of cv::resize, the per-axis tables and every form (copy,
nearest, linear for float32 and uint8, the area forms), one image at a time, and the sky mask.  The text of the header is the
definition; this file is that text and nothing else (it shares no code with the library, and tests/test_resize_ref_cpu.py holds it to
definitions it shares no code with).  The device equals it byte for byte (tests/test_gpu_resize.py)."""
from __future__ import annotations

import numpy as np

U8C1, U8C3, F32C1, F32C2 = 0, 1, 2, 3                                 # MAV_WARP_*
NEAREST, LINEAR, AREA = 0, 1, 3                                       # MAV_INTER_*
FORMATS = {U8C1: (np.uint8, 1), U8C3: (np.uint8, 3), F32C1: (np.float32, 1), F32C2: (np.float32, 2)}
PX = {U8C1: 4, U8C3: 4, F32C1: 4, F32C2: 2}                           # consecutive destination pixels of one thread
DBL_EPS = float(np.finfo(np.float64).eps)
MAX_SIDE = 32767
QNAN = np.uint32(0x7FC00000)
f32 = np.float32


def bits(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def canon(a: np.ndarray) -> np.ndarray:
    """a NaN result is stored as 0x7FC00000"""
    a = np.ascontiguousarray(a, np.float32).copy()
    a.view(np.uint32)[np.isnan(a)] = QNAN
    return a


def image_shape(fmt: int, h: int, w: int) -> tuple:
    ch = FORMATS[fmt][1]
    return (h, w) if ch == 1 else (h, w, ch)


def scales(sw: int, sh: int, dw: int, dh: int) -> tuple:
    return sw / dw, sh / dh                                           # (double)sw / dw: one correctly rounded division


# ---- dispatch --------------------------------------------------------------------------------------------------------------------------------
def form_of(fmt: int, sw: int, sh: int, dw: int, dh: int, interp: int) -> str:
    """the form cv::resize's dispatch picks, in the header's order: copy | nearest | linear | area_2x2 (uint8) | area_fast | area_general"""
    scale_x, scale_y = scales(sw, sh, dw, dh)
    if (dw, dh) == (sw, sh):
        return "copy"
    if interp == LINEAR and abs(scale_x - 2) < DBL_EPS and abs(scale_y - 2) < DBL_EPS:
        interp = AREA
    if interp == NEAREST:
        return "nearest"
    if interp == LINEAR:
        return "linear"
    assert interp == AREA and dw <= sw and dh <= sh
    ix, iy = int(np.rint(scale_x)), int(np.rint(scale_y))
    if not (abs(scale_x - ix) < DBL_EPS and abs(scale_y - iy) < DBL_EPS):
        return "area_general"
    return "area_2x2" if FORMATS[fmt][0] == np.uint8 and ix == 2 and iy == 2 else "area_fast"


def vector_stores(fmt: int, dw: int, dst_address: int, sky: bool = False) -> bool:
    """the aligned store path: every destination row begins on the store's boundary"""
    if sky or FORMATS[fmt][0] == np.uint8:
        return dw % 4 == 0 and dst_address % 4 == 0
    return dw % PX[fmt] == 0 and dst_address % 16 == 0


def refused(fmt: int, sw: int, sh: int, dw: int, dh: int, interp: int) -> bool:
    return (fmt not in FORMATS or interp not in (NEAREST, LINEAR, AREA) or not all(1 <= v <= MAX_SIDE for v in (sw, sh, dw, dh))
            or (interp == AREA and (dw > sw or dh > sh)))


# ---- tables ----------------------------------------------------------------------------------------------------------------------------------
def nearest_table(dsize: int, ssize: int, scale: float) -> np.ndarray:
    return np.minimum(np.floor(np.arange(dsize, dtype=np.float64) * scale).astype(np.int64), ssize - 1)


def linear_table(dsize: int, ssize: int, scale: float):
    """(s, a float32, one-tap?) of every destination index of one axis"""
    d = np.arange(dsize, dtype=np.float64)
    f = ((d + 0.5) * scale - 0.5).astype(np.float32)                  # evaluated in double, rounded to float32 once
    s = np.floor(f).astype(np.int64)
    a = f - s.astype(np.float32)
    neg = s < 0
    s[neg], a[neg] = 0, 0
    one = s >= ssize - 1
    s[one], a[one] = ssize - 1, 0
    return s, a.astype(np.float32), one


def linear_coefs(a: np.ndarray):
    """the uint8 path's (coefficient of S[s], coefficient of S[s + 1]): round_half_even(c * 2048.f), saturated to int16"""
    c0 = np.clip(np.rint((f32(1) - a) * f32(2048)), -32768, 32767).astype(np.int32)
    c1 = np.clip(np.rint(a * f32(2048)), -32768, 32767).astype(np.int32)
    return c0, c1


def area_taps(dsize: int, ssize: int, scale: float) -> list:
    """area_span: per destination index the list of (source index, float32 weight) in accumulation order"""
    out = []
    for d in range(dsize):
        f1 = d * scale
        f2 = f1 + scale
        cell = min(scale, ssize - f1)
        s1, s2 = int(np.ceil(f1)), min(int(np.floor(f2)), ssize - 1)
        s1 = min(s1, s2)
        taps = []
        if s1 - f1 > 1e-3:
            taps.append((s1 - 1, f32((s1 - f1) / cell)))
        for s in range(s1, s2):
            taps.append((s, f32(1.0 / cell)))
        if f2 - s2 > 1e-3:
            taps.append((s2, f32(min(min(f2 - s2, 1.0), cell) / cell)))
        out.append(taps)
    return out


def _passes(taps: list) -> list:
    """pass r: the r-th tap of every destination index that has one -> (destination indices, source indices, weights)"""
    out = []
    for r in range(max(len(t) for t in taps)):
        rows = [(d, t[r][0], t[r][1]) for d, t in enumerate(taps) if len(t) > r]
        out.append((np.array([x[0] for x in rows]), np.array([x[1] for x in rows]), np.array([x[2] for x in rows], np.float32)))
    return out


# ---- forms, on S (sh, sw, C) ------------------------------------------------------------------------------------------------------------------
def _u8_of(sum_f32: np.ndarray) -> np.ndarray:
    return np.clip(np.rint(sum_f32), 0, 255).astype(np.uint8)        # rintf: half to even, then the clamp


def nearest(S, dw, dh):
    sh, sw = S.shape[:2]
    scale_x, scale_y = scales(sw, sh, dw, dh)
    return S[nearest_table(dh, sh, scale_y)][:, nearest_table(dw, sw, scale_x)].copy()


def linear(S, dw, dh):
    sh, sw = S.shape[:2]
    scale_x, scale_y = scales(sw, sh, dw, dh)
    sx, a, one = linear_table(dw, sw, scale_x)
    sy, b, _ = linear_table(dh, sh, scale_y)
    sx1, sy1 = np.minimum(sx + 1, sw - 1), np.minimum(sy + 1, sh - 1)     # sx1 is read outside the one-tap region alone
    one_ = one[None, :, None]
    if S.dtype == np.float32:
        a_, b_ = a[None, :, None], b[:, None, None]
        with np.errstate(all="ignore"):
            h = np.where(one_, S[:, sx] * f32(1), S[:, sx] * (f32(1) - a_) + S[:, sx1] * a_)
            out = h[sy] * (f32(1) - b_) + h[sy1] * b_
        assert h.dtype == np.float32 and out.dtype == np.float32
        return canon(out)
    a0, a1 = linear_coefs(a)
    b0, b1 = linear_coefs(b)
    T = S.astype(np.int32)
    h = np.where(one_, T[:, sx] * 2048, T[:, sx] * a0[None, :, None] + T[:, sx1] * a1[None, :, None])
    out = (((b0[:, None, None] * (h[sy] >> 4)) >> 16) + ((b1[:, None, None] * (h[sy1] >> 4)) >> 16) + 2) >> 2
    return np.clip(out, 0, 255).astype(np.uint8)


def area_fast(S, dw, dh, ix, iy):
    C = S.shape[2]
    blk = S[:dh * iy, :dw * ix].reshape(dh, iy, dw, ix, C)
    area = ix * iy
    terms = [blk[:, k // ix, :, k % ix] for k in range(area)]             # rows, then columns
    if S.dtype == np.uint8:
        total = sum(t.astype(np.int32) for t in terms)
        if ix == 2 and iy == 2:
            return ((total + 2) >> 2).astype(np.uint8)                    # rounds a half UP
        return _u8_of(total.astype(np.float32) * (f32(1) / f32(area)))
    with np.errstate(all="ignore"):
        s = np.zeros((dh, dw, C), np.float32)
        k = 0
        while k <= area - 4:
            s = s + (((terms[k] + terms[k + 1]) + terms[k + 2]) + terms[k + 3])
            k += 4
        while k < area:
            s = s + terms[k]
            k += 1
        return canon(s * (f32(1) / f32(area)))


def area_general(S, dw, dh):
    sh, sw, C = S.shape
    scale_x, scale_y = scales(sw, sh, dw, dh)
    T = S.astype(np.float32)
    with np.errstate(all="ignore"):
        buf = np.zeros((sh, dw, C), np.float32)
        for di, si, al in _passes(area_taps(dw, sw, scale_x)):
            buf[:, di] = buf[:, di] + T[:, si] * al[None, :, None]
        acc = np.zeros((dh, dw, C), np.float32)
        for di, si, be in _passes(area_taps(dh, sh, scale_y)):
            acc[di] = acc[di] + be[:, None, None] * buf[si]
    return _u8_of(acc) if S.dtype == np.uint8 else canon(acc)


# ---- the calls --------------------------------------------------------------------------------------------------------------------------------
def resize(img: np.ndarray, dw: int, dh: int, interp: int = LINEAR) -> np.ndarray:
    """mav_resize on one image (sh, sw[, C]), uint8 or float32"""
    img = np.ascontiguousarray(img)
    assert img.dtype in (np.uint8, np.float32)
    S = img[..., None] if img.ndim == 2 else img
    sh, sw, C = S.shape
    fmt = {(np.dtype(np.uint8), 1): U8C1, (np.dtype(np.uint8), 3): U8C3, (np.dtype(np.float32), 1): F32C1, (np.dtype(np.float32), 2): F32C2}[(S.dtype, C)]
    assert not refused(fmt, sw, sh, dw, dh, interp)
    form = form_of(fmt, sw, sh, dw, dh, interp)
    if form == "copy":
        out = S.copy()
    elif form == "nearest":
        out = nearest(S, dw, dh)
    elif form == "linear":
        out = linear(S, dw, dh)
    elif form == "area_general":
        out = area_general(S, dw, dh)
    else:
        scale_x, scale_y = scales(sw, sh, dw, dh)
        out = area_fast(S, dw, dh, int(np.rint(scale_x)), int(np.rint(scale_y)))
    assert out.shape == (dh, dw, C) and out.dtype == S.dtype
    return out[..., 0] if img.ndim == 2 else out


def sky_mask(pred_bgr: np.ndarray, dw: int, dh: int, key=(180, 130)) -> np.ndarray:
    """mav_sky_mask on one picture: the two-step route, (dh, dw) uint8 of 0 / 1"""
    img = resize(pred_bgr, dw, dh, LINEAR)
    return ((img[..., 0] == key[0]) & (img[..., 1] == key[1])).astype(np.uint8)
