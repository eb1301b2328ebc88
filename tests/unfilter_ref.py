"""PNG filters 0 - 4 in numpy, both ways, and the output conversions of the device decoder, restated from the PNG specification (section
9) and from what cv2.imread / cv2.cvtColor return -- independent of csrc: no code shared, arithmetic in int64 and reduced modulo 256.

    filter_rows(rows, bpp, types)   (H, stride) u8 reconstructed rows + a filter type per row -> the raw scanline bytes
    unfilter(raw, H, stride, bpp)   the raw scanline bytes -> (H, stride) u8 (None where a filter byte is above 4)
    convert(samples, out)           (H, W, ch) samples -> "samples" / "bgr" / "gray"
"""
import numpy as np


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def filter_rows(rows, bpp, types) -> bytes:
    rows = np.asarray(rows, np.uint8)
    H, stride = rows.shape
    x = rows.astype(np.int64)
    left = np.zeros_like(x)
    left[:, bpp:] = x[:, :-bpp] if stride > bpp else 0
    up = np.zeros_like(x)
    up[1:] = x[:-1]
    ul = np.zeros_like(x)
    ul[1:, bpp:] = x[:-1, :-bpp] if stride > bpp else 0
    out = np.empty((H, stride + 1), np.uint8)
    for y, t in enumerate(types):
        pred = (0, left[y], up[y], (left[y] + up[y]) >> 1, _paeth(left[y], up[y], ul[y]))[t]
        out[y, 0] = t
        out[y, 1:] = (x[y] - pred) & 255
    return out.tobytes()


def unfilter(raw, H, stride, bpp):
    raw = np.frombuffer(bytes(raw), np.uint8).reshape(H, stride + 1)
    out = np.zeros((H, stride), np.int64)
    prev = np.zeros(stride, np.int64)
    for y in range(H):
        t, x = int(raw[y, 0]), raw[y, 1:].astype(np.int64)
        if t > 4:
            return None
        if t == 0:
            cur = x
        elif t == 2:
            cur = (x + prev) & 255
        elif t == 1:                                   # a running sum per byte lane of the pixel
            cur = np.zeros(stride, np.int64)
            for j in range(bpp):
                cur[j::bpp] = np.cumsum(x[j::bpp]) & 255
        else:
            cur = np.zeros(stride, np.int64)
            for i in range(stride):
                a = cur[i - bpp] if i >= bpp else 0
                b = prev[i]
                c = prev[i - bpp] if i >= bpp else 0
                if t == 3:
                    pred = (a + b) >> 1
                else:
                    p = a + b - c
                    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                    pred = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
                cur[i] = (x[i] + pred) & 255
        out[y] = cur
        prev = cur
    return out.astype(np.uint8)


def convert(samples, out):
    """(..., H, W, ch) u8 samples of a gray / gray + alpha / RGB / RGBA file -> the decoder's output"""
    s = np.asarray(samples, np.uint8)
    ch = s.shape[-1]
    if out == "samples":
        return s
    bgr = np.repeat(s[..., :1], 3, axis=-1) if ch < 3 else s[..., 2::-1]
    if out == "bgr":
        return np.ascontiguousarray(bgr)
    b, g, r = (bgr[..., k].astype(np.int64) for k in range(3))
    return ((b * 1868 + g * 9617 + r * 4899 + 8192) >> 14).astype(np.uint8)[..., None]
