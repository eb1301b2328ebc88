"""TEST INFRASTRUCTURE -- the Gaussian-window sweep (cv2.OPTFLOW_FARNEBACK_GAUSSIAN, FarnebackUpdateFlow_GaussianBlur) restated in
numpy, operation for operation as the library's kernels compute it (kernels_flow.hip GaussWindow, the window policy of k_blur_iter_fast / k_blur_iter_generic):
float32 everywhere, no fused multiply-add, one fixed order per pixel, and the solve's mixed widths.  The kernels are held to this
file bit for bit (tests/test_gpu_gauss_window.py).

UNPINNED against cv2: the definition, taps included, is restated from OpenCV 4.x optflowgf.cpp from memory -- there is no cv2 on the
machines this project is built on.  The tap normalisation (the running sum that starts at 1 and counts the centre tap twice, so the
taps sum to 0.69 and not to 1) is the first thing to re-check when a cv2 is at hand.

    m = winsize // 2, sigma = 0.3 m (double)
    t_i = float32(exp(-i i / (2 sigma sigma))), i = 0..m;   s = 1 + sum_i 2 t_i (double, i = 0 included);   k_i = float32(t_i (1 / s))
    V(y, x) = M(y, x) k_0;  for i = 1..m in order:  V += (M(max(y - i, 0), x) + M(min(y + i, h - 1), x)) k_i
    S(y, x) = V(y, x) k_0;  for i = 1..m in order:  S += (V(y, max(x - i, 0)) + V(y, min(x + i, w - 1))) k_i
    g11, g12, g22, h1, h2 = S;   d = f32(g11 g22) - f32(g12 g12);   idet = 1 / (double(d) + 1e-3)
    u = float32(double(f32(g11 h2) - f32(g12 h1)) idet);   v = float32(double(f32(g22 h1) - f32(g12 h2)) idet)
"""
from __future__ import annotations

import math

import numpy as np


def taps(winsize: int) -> np.ndarray:
    """k_0 .. k_m, float32; math.exp is the C library's exp."""
    m = winsize // 2
    sigma = m * 0.3
    t = [np.float32(math.exp(-i * i / (2 * sigma * sigma))) for i in range(m + 1)]
    s = 1.0
    for ti in t:
        s += float(ti) * 2
    s = 1.0 / s
    return np.array([np.float32(float(ti) * s) for ti in t], np.float32)


def _pass(a: np.ndarray, k: np.ndarray, axis: int, dtype) -> np.ndarray:
    """One weighted sum along `axis` with replicated borders, in dtype arithmetic, taps in the order 0, 1 .. m."""
    n = a.shape[axis]
    idx = np.arange(n)
    out = a * dtype(k[0])
    for i in range(1, len(k)):
        lo = np.take(a, np.maximum(idx - i, 0), axis=axis)
        hi = np.take(a, np.minimum(idx + i, n - 1), axis=axis)
        out = out + (lo + hi) * dtype(k[i])
    assert out.dtype == dtype
    return out


def window_sums(M: np.ndarray, winsize: int, dtype=np.float32, horizontal_first: bool = False) -> np.ndarray:
    """S of an (h, w, 5) or (h, w) array M: vertical pass, then horizontal (the library's order; horizontal_first swaps them)."""
    k = taps(winsize)
    a = np.asarray(M).astype(dtype)
    first, second = (1, 0) if horizontal_first else (0, 1)
    return _pass(_pass(a, k, first, dtype), k, second, dtype)


def solve(S: np.ndarray) -> np.ndarray:
    """(h, w, 5) float32 sums -> (h, w, 2) float32 flow, with cv2's mixed widths."""
    S = np.asarray(S)
    assert S.dtype == np.float32
    g11, g12, g22, h1, h2 = (S[..., i] for i in range(5))
    d = g11 * g22 - g12 * g12                               # float32 products, float32 difference
    idet = 1.0 / (d.astype(np.float64) + 1e-3)
    u = ((g11 * h2 - g12 * h1).astype(np.float64) * idet).astype(np.float32)
    v = ((g22 * h1 - g12 * h2).astype(np.float64) * idet).astype(np.float32)
    return np.stack([u, v], -1)


def sweep(M: np.ndarray, winsize: int) -> np.ndarray:
    """The flow one Gaussian sweep makes of M (h, w, 5)."""
    return solve(window_sums(np.ascontiguousarray(M, np.float32), winsize))


def calc(oracle, prev, nxt, params) -> np.ndarray:
    """oracle.pyramid's loop (oracle/fb_oracle.py) with this sweep in place of blur_iter, and oracle.update_matrices for M'."""
    prev = np.ascontiguousarray(prev, np.uint8)
    nxt = np.ascontiguousarray(nxt, np.uint8)
    H, W = prev.shape
    p = params
    flow = None
    for k in range(oracle.num_layers(W, H, p) - 1, -1, -1):
        w, h, sigma, ksize = oracle.layer_dims(W, H, p, k)
        flow = np.zeros((h, w, 2), np.float32) if flow is None else oracle.resize_flow(flow, w, h, 1.0 / p.pyr_scale)
        R0, R1 = (oracle.polyexp(oracle.blur_resize(img, w, h, ksize, sigma), p.poly_n, p.poly_sigma) for img in (prev, nxt))
        M = oracle.update_matrices(R0, R1, flow)
        for it in range(p.iterations):
            flow = sweep(M, p.winsize)
            if it < p.iterations - 1:
                M = oracle.update_matrices(R0, R1, flow)
    return flow
