"""TEST INFRASTRUCTURE -- the flow history (csrc/kernels_history.hip) restated in numpy, operation for operation in the kernel's order:
cv2.remap(INTER_LINEAR, BORDER_CONSTANT 0) of a 2-channel field as include/mavflow.h defines it from OpenCV 4.x (five steps), and
Detector.get_history (reference src/detector.py:365-388) written like the reference's function with that remap swapped in.  The device
results are compared with these byte for byte (tests/test_gpu_history.py); tests/test_history_ref_cpu.py holds this file to the
definition and to an independent interpolator.  Not pinned against a cv2 build (cv2 is not installed here): DESIGN.md section 4g.

A NaN result is THE quiet NaN (0x7FF8000000000000 / 0x7FC00000) here as on the device: whether a result is a NaN is arithmetic, its
sign and payload depend on the machine that produced it."""
from __future__ import annotations

import numpy as np

_LIM = np.float32(2147483648.0)


def canon(a: np.ndarray) -> np.ndarray:
    """NaNs replaced by numpy's own quiet NaN (in place; returns a)."""
    a[np.isnan(a)] = np.nan
    return a


def remap_linear_ref(src, map_x, map_y, trace: list | None = None) -> np.ndarray:
    """remap(src, map_x, map_y, INTER_LINEAR, BORDER_CONSTANT, 0): src (H, W, 2) float32 or float64, float32 maps of any (equal)
    shape -> maps' shape + (2,) float64.  trace: a list that receives one dict per call -- which way every element went."""
    src = np.asarray(src)
    H, W = src.shape[:2]
    mx, my = np.asarray(map_x, np.float32), np.asarray(map_y, np.float32)
    with np.errstate(all="ignore"):
        # 1. the coordinates in 1/32 pixels, rounded half to even; NaN, infinite or past int32: wholly outside
        px, py = mx * np.float32(32.0), my * np.float32(32.0)
        fits = (px >= -_LIM) & (px < _LIM) & (py >= -_LIM) & (py < _LIM)
        qx = np.rint(np.where(fits, px, np.float32(0))).astype(np.int64)
        qy = np.rint(np.where(fits, py, np.float32(0))).astype(np.int64)
        # 2. cell (saturated to int16) and fraction
        sx, ax = np.clip(qx >> 5, -32768, 32767), qx & 31
        sy, ay = np.clip(qy >> 5, -32768, 32767), qy & 31
        # 3. the weights: float32, exact multiples of 1/1024
        fx, fy = ax.astype(np.float32) * np.float32(0.03125), ay.astype(np.float32) * np.float32(0.03125)
        gx, gy = np.float32(1) - fx, np.float32(1) - fy
        w = [(gy * gx).astype(np.float64), (gy * fx).astype(np.float64), (fy * gx).astype(np.float64), (fy * fx).astype(np.float64)]
        # 4. wholly outside
        inside = fits & ~((sx >= W) | (sx + 1 < 0) | (sy >= H) | (sy + 1 < 0))

        # 5. the four taps, widened, 0.0 where out of range; every product and sum on its own
        def tap(r, c):
            ok = inside & (r >= 0) & (r < H) & (c >= 0) & (c < W)
            v = src[np.clip(r, 0, H - 1), np.clip(c, 0, W - 1)].astype(np.float64)
            return np.where(ok[..., None], v, 0.0), ok

        taps = [tap(sy, sx), tap(sy, sx + 1), tap(sy + 1, sx), tap(sy + 1, sx + 1)]
        t = [a for a, _ in taps]
        out = ((t[0] * w[0][..., None] + t[1] * w[1][..., None]) + t[2] * w[2][..., None]) + t[3] * w[3][..., None]
    if trace is not None:
        nan_zero_w = np.zeros(mx.shape, bool)
        for (a, ok), wi in zip(taps, w):
            nan_zero_w |= ok & np.isnan(a).any(axis=-1) & (wi == 0)
        trace.append(dict(W=W, H=H, px=px, py=py, mx=mx, my=my, fits=fits, qx=qx, qy=qy, sx=sx, sy=sy, inside=inside, nan_zero_w=nan_zero_w))
    return canon(out)


def schedule(length: int, index: int) -> list:
    """The reference's loop (detector.py:376-385) taken literally: the slots a push at `index` walks."""
    out = []
    k = (index + 1) % (length - 1)
    while k != index % (length - 1):
        out.append(k)
        k = (k + 1) % length
    return out


class HistoryRef:
    """The state Detector.__init__ keeps for get_history (detector.py:39-45) and the function itself.  dtype: the ring's element
    (the reference's is float64; a float32 ring holding the same values gives the same bits).  axes "reference": the reference's
    channel order; "xy": r += v, c += u."""

    def __init__(self, H: int, W: int, length: int = 20, dtype=np.float64, axes: str = "reference"):
        self.x_coords = np.tile(np.arange(W), (H, 1))
        self.y_coords = np.tile(np.arange(H), (W, 1)).T
        self.history_length = length
        self.flow_uv_history = np.zeros((length, H, W, 2), dtype)
        self.history_index = 0
        self.axes = axes

    def get_history(self, flow_uv: np.ndarray, out: str = "reference", trace: list | None = None) -> np.ndarray:
        self.flow_uv_history[self.history_index, ...] = flow_uv

        k = (self.history_index + 1) % (self.history_length - 1)
        orig_map = np.zeros(self.flow_uv_history.shape[1:], dtype=np.float64)
        orig_map[..., 0] = self.y_coords
        orig_map[..., 1] = self.x_coords
        lookup_map = np.copy(orig_map)

        with np.errstate(all="ignore"):
            while k != (self.history_index) % (self.history_length - 1):
                warped = lookup_map.astype(np.float32)
                step = remap_linear_ref(self.flow_uv_history[k, ...], warped[..., 1], warped[..., 0], trace)
                lookup_map += step[..., ::-1] if self.axes == "xy" else step
                k = (k + 1) % self.history_length

            self.history_index = (self.history_index + 1) % self.history_length
            res = lookup_map - orig_map
            if out == "flow":                                   # float32 (c - x, r - y), each rounded once from the double
                return canon(np.ascontiguousarray(res[..., ::-1]).astype(np.float32))
        return canon(res)


def bits(a: np.ndarray) -> np.ndarray:
    """The array's bytes as unsigned integers of its element size: what the device results are compared by."""
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])
