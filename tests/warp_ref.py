"""TEST INFRASTRUCTURE -- the image warps (csrc/kernels_warp.hip) restated in numpy, operation for operation in the kernel's order:
include/mavflow_warp.h's SAMPLING and COORDINATES (OpenCV 4.x imgwarp.cpp as remembered) and Detector.warp_method's arithmetic
(reference src/detector.py:213-224).  float32 / float64 / int64 arithmetic in the stated order.  The device results are compared with
these byte for byte (tests/test_gpu_warp.py); tests/test_warp_ref_cpu.py holds this file to the definition and to an independent
interpolator.  Not pinned against a cv2 build (cv2 is not installed here): DESIGN.md section 4k lists what to re-check first.

A NaN result is THE quiet NaN (0x7FC00000) here as on the device."""
from __future__ import annotations

import numpy as np

from history_ref import bits, canon  # noqa: F401  (the shared steps; bits is what the device results are compared by)

U8C1, U8C3, F32C1, F32C2 = 0, 1, 2, 3               # MAV_WARP_*
INVERSE_MAP = 16
AFFINE, PERSPECTIVE = 0, 1
FORMATS = {U8C1: (np.uint8, 1), U8C3: (np.uint8, 3), F32C1: (np.float32, 1), F32C2: (np.float32, 2)}
FORMAT_NAMES = {U8C1: "U8C1", U8C3: "U8C3", F32C1: "F32C1", F32C2: "F32C2"}
RECORD_DTYPE = np.dtype([("max_mag", np.float32), ("row", np.int32), ("col", np.int32), ("pad", np.int32)])
_LIM = np.float32(2147483648.0)
INT_MIN, INT_MAX = -2147483648, 2147483647


def image_shape(fmt: int, H: int, W: int) -> tuple:
    return (H, W) if FORMATS[fmt][1] == 1 else (H, W, FORMATS[fmt][1])


def format_of(img: np.ndarray) -> int:
    for fmt, (dt, ch) in FORMATS.items():
        if img.dtype == dt and (img.ndim == 2 if ch == 1 else img.ndim == 3 and img.shape[2] == ch):
            return fmt
    raise TypeError((img.dtype, img.shape))


# ---- SAMPLING ------------------------------------------------------------------------------------------------------------------------------
def sample(src: np.ndarray, fits, qx, qy, trace: list | None = None) -> np.ndarray:
    """One image (H, W) or (H, W, C) uint8 / float32 sampled at the 1/32-pixel positions (qx, qy) (int64 arrays holding int32 values);
    ~fits: wholly outside.  Returns an image of the positions' shape (+ (C,))."""
    src = np.asarray(src)
    H, W = src.shape[:2]
    s3 = src.reshape(H, W, -1)
    sx, ax = np.clip(qx >> 5, -32768, 32767), qx & 31
    sy, ay = np.clip(qy >> 5, -32768, 32767), qy & 31
    inside = fits & ~((sx >= W) | (sx + 1 < 0) | (sy >= H) | (sy + 1 < 0))

    def tap(r, c):
        ok = inside & (r >= 0) & (r < H) & (c >= 0) & (c < W)
        return s3[np.clip(r, 0, H - 1), np.clip(c, 0, W - 1)], ok

    taps = [tap(sy, sx), tap(sy, sx + 1), tap(sy + 1, sx), tap(sy + 1, sx + 1)]
    with np.errstate(all="ignore"):
        if src.dtype == np.float32:
            fx, fy = ax.astype(np.float32) * np.float32(0.03125), ay.astype(np.float32) * np.float32(0.03125)
            gx, gy = np.float32(1) - fx, np.float32(1) - fy
            w = [gy * gx, gy * fx, fy * gx, fy * fx]
            t = [np.where(ok[..., None], v, np.float32(0)) for v, ok in taps]
            out = ((t[0] * w[0][..., None] + t[1] * w[1][..., None]) + t[2] * w[2][..., None]) + t[3] * w[3][..., None]
            assert out.dtype == np.float32
            out = canon(out)
        else:
            w = [32 * (32 - ay) * (32 - ax), 32 * (32 - ay) * ax, 32 * ay * (32 - ax), 32 * ay * ax]
            t = [np.where(ok[..., None], v.astype(np.int64), 0) for v, ok in taps]
            acc = t[0] * w[0][..., None] + t[1] * w[1][..., None] + t[2] * w[2][..., None] + t[3] * w[3][..., None]
            out = ((acc + 16384) >> 15).astype(np.uint8)
    if trace is not None:
        nan_zero_w = np.zeros(np.shape(qx), bool)
        if src.dtype == np.float32:
            for (v, ok), wi in zip(taps, w):
                nan_zero_w |= ok & np.isnan(v).any(axis=-1) & (wi == 0)
        clamped = inside & ((np.clip(qx >> 5, -32768, 32767) != (qx >> 5)) | (np.clip(qy >> 5, -32768, 32767) != (qy >> 5)))
        partial = inside & ~(taps[0][1] & taps[1][1] & taps[2][1] & taps[3][1])
        trace.append(dict(W=W, H=H, fits=fits, qx=qx, qy=qy, sx=sx, sy=sy, ax=ax, ay=ay, inside=inside, nan_zero_w=nan_zero_w,
                          int16_clamped=(np.clip(qx >> 5, -32768, 32767) != (qx >> 5)) | (np.clip(qy >> 5, -32768, 32767) != (qy >> 5)),
                          clamped_inside=clamped, partial=partial))
    return out.reshape(np.shape(qx) + src.shape[2:])


# ---- COORDINATES ---------------------------------------------------------------------------------------------------------------------------
def q_from_map(mx, my, trace: list | None = None):
    """step 1 of ONE REMAP for both coordinates: (fits, qx, qy)"""
    mx, my = np.asarray(mx, np.float32), np.asarray(my, np.float32)
    with np.errstate(all="ignore"):
        px, py = mx * np.float32(32.0), my * np.float32(32.0)
        fits = (px >= -_LIM) & (px < _LIM) & (py >= -_LIM) & (py < _LIM)
        qx = np.rint(np.where(fits, px, np.float32(0))).astype(np.int64)
        qy = np.rint(np.where(fits, py, np.float32(0))).astype(np.int64)
    if trace is not None:
        with np.errstate(all="ignore"):
            frac = [np.abs(p - np.trunc(p)) == np.float32(0.5) for p in (px, py)]
        tie = lambda p: fits & frac[0 if p is px else 1]
        trace.append(dict(px=px, py=py, tie_neg=(tie(px) & (px < 0)) | (tie(py) & (py < 0)), tie_pos=(tie(px) & (px > 0)) | (tie(py) & (py > 0))))
    return fits, qx, qy


def flow_map(flow: np.ndarray):
    """Farneback.warp_flow's map (src/farneback.py:64-67), grid - flow, in numpy's types of that function: the negated float32 field
    plus int64 coordinates in place, one rounding per element."""
    h, w = flow.shape[:2]
    with np.errstate(all="ignore"):
        m = np.negative(np.asarray(flow, np.float32))
        m[..., 0] += np.arange(w)                                        # float32 += int64, in place: one float32 rounding
        m[..., 1] += np.arange(h)[:, None]
    return m


def sat_rint(v):
    """rint, half to even, saturated to int32; NaN -> INT_MIN.  int64 array."""
    v = np.asarray(v, np.float64)
    with np.errstate(all="ignore"):
        r = np.rint(v)
    out = np.empty(v.shape, np.int64)
    nan = np.isnan(v)
    hi, lo = ~nan & (v >= 2147483647.0), ~nan & (v <= -2147483648.0)
    mid = ~(nan | hi | lo)
    out[nan], out[hi], out[lo] = INT_MIN, INT_MAX, INT_MIN
    out[mid] = r[mid].astype(np.int64)
    return out


def wrap32(v):
    """int64 values reduced to int32 with wrap-around, kept in int64"""
    return ((np.asarray(v, np.int64) + 2147483648) & 0xFFFFFFFF) - 2147483648


def invert_affine(M) -> np.ndarray:
    M = np.asarray(M, np.float64).reshape(6)
    f = np.float64
    with np.errstate(all="ignore"):
        M0, M1, M2, M3, M4, M5 = (f(v) for v in M)
        D = M0 * M4 - M1 * M3
        D = f(1.0) / D if D != 0 else f(0.0)
        A11, A22 = M4 * D, M0 * D
        M0 = A11; M1 = M1 * (-D); M3 = M3 * (-D); M4 = A22
        b1 = (-M0) * M2 - M1 * M5
        b2 = (-M3) * M2 - M4 * M5
    return np.array([M0, M1, b1, M3, M4, b2], np.float64)


def invert_perspective(M) -> np.ndarray:
    f = np.float64
    M0, M1, M2, M3, M4, M5, M6, M7, M8 = (f(v) for v in np.asarray(M, np.float64).reshape(9))
    with np.errstate(all="ignore"):
        d = (M0 * (M4 * M8 - M5 * M7) - M1 * (M3 * M8 - M5 * M6)) + M2 * (M3 * M7 - M4 * M6)
        d = f(1.0) / d if d != 0 else f(0.0)
        N = [(M4 * M8 - M5 * M7) * d, (M2 * M7 - M1 * M8) * d, (M1 * M5 - M2 * M4) * d,
             (M5 * M6 - M3 * M8) * d, (M0 * M8 - M2 * M6) * d, (M2 * M3 - M0 * M5) * d,
             (M3 * M7 - M4 * M6) * d, (M1 * M6 - M0 * M7) * d, (M0 * M4 - M1 * M3) * d]
    return np.array(N, np.float64)


def determinant(M) -> float:
    """D / d as the inversions above take it (what the host forms refuse at 0)"""
    m = [np.float64(v) for v in np.asarray(M, np.float64).ravel()]
    with np.errstate(all="ignore"):
        if len(m) == 6:
            return m[0] * m[4] - m[1] * m[3]
        return (m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6])) + m[2] * (m[3] * m[7] - m[4] * m[6])


def q_affine(M, flags: int, H: int, W: int, trace: list | None = None):
    m = np.asarray(M, np.float64).reshape(6) if flags & INVERSE_MAP else invert_affine(M)
    x, y = np.arange(W, dtype=np.float64)[None, :], np.arange(H, dtype=np.float64)[:, None]
    with np.errstate(all="ignore"):
        ry, rx = sat_rint((m[1] * y + m[2]) * 1024.0), sat_rint((m[0] * x) * 1024.0)
        sy_, sx_ = sat_rint((m[4] * y + m[5]) * 1024.0), sat_rint((m[3] * x) * 1024.0)
        X0, Y0 = wrap32(ry + 16), wrap32(sy_ + 16)
        qx, qy = wrap32(X0 + rx) >> 5, wrap32(Y0 + sx_) >> 5
    qx, qy = np.broadcast_to(qx, (H, W)).copy(), np.broadcast_to(qy, (H, W)).copy()
    if trace is not None:
        sat = lambda r: (r == INT_MIN) | (r == INT_MAX)
        trace.append(dict(m=m, saturated=bool(sat(ry).any() or sat(rx).any() or sat(sy_).any() or sat(sx_).any())))
    return np.ones((H, W), bool), qx, qy


def q_perspective(M, flags: int, H: int, W: int, trace: list | None = None):
    m = np.asarray(M, np.float64).reshape(9) if flags & INVERSE_MAP else invert_perspective(M)
    x, y = np.arange(W, dtype=np.float64)[None, :], np.arange(H, dtype=np.float64)[:, None]
    with np.errstate(all="ignore"):
        Wd0 = (m[6] * x + m[7] * y) + m[8]
        Wd = np.where(Wd0 != 0, np.float64(32.0) / Wd0, np.float64(0.0))
        fX, fY = ((m[0] * x + m[1] * y) + m[2]) * Wd, ((m[3] * x + m[4] * y) + m[5]) * Wd
        fits = ~np.isnan(fX) & ~np.isnan(fY)
        cX, cY = np.clip(fX, -2147483648.0, 2147483647.0), np.clip(fY, -2147483648.0, 2147483647.0)
        qx = np.rint(np.where(fits, cX, 0.0)).astype(np.int64)
        qy = np.rint(np.where(fits, cY, 0.0)).astype(np.int64)
    if trace is not None:
        trace.append(dict(m=m, w_zero=np.broadcast_to(Wd0 == 0, (H, W)), w_pos=bool((Wd0 > 0).any()), w_neg=bool((Wd0 < 0).any()),
                          clamped=bool(((fX != cX) & fits).any() or ((fY != cY) & fits).any())))
    return np.broadcast_to(fits, (H, W)).copy(), np.broadcast_to(qx, (H, W)).copy(), np.broadcast_to(qy, (H, W)).copy()


# ---- the calls, one image each -----------------------------------------------------------------------------------------------------------
def remap(src, map_xy, trace=None):
    map_xy = np.asarray(map_xy, np.float32)
    return sample(src, *q_from_map(map_xy[..., 0], map_xy[..., 1], trace), trace)


def remap_planes(src, map_x, map_y, trace=None):
    return sample(src, *q_from_map(map_x, map_y, trace), trace)


def warp_flow(img, flow, trace=None):
    m = flow_map(flow)
    return sample(img, *q_from_map(m[..., 0], m[..., 1], trace), trace)


def warp_affine(src, M, flags=0, trace=None):
    H, W = np.shape(src)[:2]
    return sample(src, *q_affine(M, flags, H, W, trace), trace)


def warp_perspective(src, M, flags=0, trace=None):
    H, W = np.shape(src)[:2]
    return sample(src, *q_perspective(M, flags, H, W, trace), trace)


def warp_method(flow, M, kind, trace=None):
    """Detector.warp_method :213-224 -> (flow_diff (H, W, 2) f32, flow_diff_mag (H, W) f32, record)."""
    flow_uv = np.array(flow, np.float32)
    stable = (warp_perspective if kind == PERSPECTIVE else warp_affine)(flow_uv, M, 0, trace)
    with np.errstate(all="ignore"):
        zero = stable == 0                                               # element-wise: a zero in one channel alone counts
        flow_uv = np.where(zero, stable, flow_uv)                        # flow_reset_c = stable_c there
        diff = canon(flow_uv - stable)
        mag = canon(np.sqrt(diff[..., 0] * diff[..., 0] + diff[..., 1] * diff[..., 1]))
    assert diff.dtype == mag.dtype == np.float32
    row, col = np.unravel_index(mag.argmax(), mag.shape)                  # numpy: the first NaN, else the first maximum
    rec = np.zeros((), RECORD_DTYPE)
    rec["max_mag"], rec["row"], rec["col"] = mag[row, col], row, col
    return diff, mag, rec
