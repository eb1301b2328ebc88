"""TEST INFRASTRUCTURE -- the checker of 16-bit and float32 frames (cv2.calcOpticalFlowFarneback on CV_16U / CV_32F input).

OpenCV's FarnebackOpticalFlowImpl::calc (modules/video/src/optflowgf.cpp) takes any single-channel frame: for every layer it runs
img.convertTo(fimg, CV_32F), GaussianBlur, resize(INTER_LINEAR), and everything from FarnebackPolyExp on works on float32.  So
only the layer image depends on the source depth.  Here:

  blur_resize_f32   oracle/farneback_oracle.c:fbo_blur_resize restated in numpy float32 in the C file's exact operation order
                    (row filter  acc = k[r] s[x];  acc += k[r + j] (s[x - j] + s[x + j]),  reflect-101; the column filter in the same
                    form; INTER_LINEAR with the oracle's float weights), fed float values instead of bytes.  Numpy's float32 operations
                    round exactly as the C file's (built with -ffp-contract=off), so on u8 values it IS the oracle (test_depth_ref_cpu).
  calc_depth        the oracle's stage functions composed as oracle.fb_oracle.Oracle.pyramid / initial_flow_ref.calc_init compose them,
                    with that blur in place of fbo_blur_resize.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

import initial_flow_ref


def gaussian_taps(orc, ksize: int, sigma: float) -> np.ndarray:
    """getGaussianKernel(ksize, sigma) as float32: the oracle's own fbo_gaussian_kernel."""
    k = np.empty(ksize, np.float32)
    orc.lib.fbo_gaussian_kernel(ksize, C.c_double(sigma), k.ctypes.data_as(C.POINTER(C.c_float)))
    return k


def _reflect101(p: np.ndarray, n: int) -> np.ndarray:
    if n == 1:
        return np.zeros_like(p)
    p = p.copy()
    while True:
        lo, hi = p < 0, p >= n
        if not (lo.any() or hi.any()):
            return p
        p[lo] = -p[lo]
        p[hi] = 2 * n - 2 - p[hi]


def _sym_filter(s: np.ndarray, kern: np.ndarray, axis: int) -> np.ndarray:
    """acc = k[r] s[x]; acc += k[r + j] (s[x - j] + s[x + j]) for j = 1 .. r, reflect-101 along `axis`, float32 throughout."""
    r = len(kern) // 2
    n = s.shape[axis]
    x = np.arange(n)
    acc = kern[r] * s
    for j in range(1, r + 1):
        a = np.take(s, _reflect101(x - j, n), axis=axis)
        b = np.take(s, _reflect101(x + j, n), axis=axis)
        acc = acc + kern[r + j] * (a + b)
    return acc


def _coords(d: int, S: int):
    """resize(INTER_LINEAR) half-pixel centres as the oracle evaluates them: fx = (float)((dx + 0.5) * scale - 0.5) in double,
    sx = floor, fx -= sx in float, clamped."""
    scale = S / d
    f = ((np.arange(d, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(np.float32)).astype(np.float32)
    low, high = s < 0, s >= S - 1
    f[low | high] = 0
    s[low] = 0
    s[high] = S - 1
    return s, f


def blur_resize_f32(img: np.ndarray, w: int, h: int, ksize: int, sigma: float, orc=None) -> np.ndarray:
    """convertTo(CV_32F) -> GaussianBlur(ksize, sigma, BORDER_REFLECT_101) -> resize((w, h), INTER_LINEAR) of one frame of any
    depth, in fbo_blur_resize's operation order.  The taps come from the oracle (orc; loaded when None)."""
    if orc is None:
        from oracle import fb_oracle
        orc = fb_oracle.load()
    s = np.ascontiguousarray(img).astype(np.float32)
    H, W = s.shape
    kern = gaussian_taps(orc, ksize, sigma)
    blur = _sym_filter(_sym_filter(s, kern, 1), kern, 0)
    if w == W and h == H:
        return blur
    sx, ax = _coords(w, W)
    sy, ay = _coords(h, H)
    sx1 = np.minimum(sx + 1, W - 1)
    sy1 = np.minimum(sy + 1, H - 1)
    a0, a1 = (np.float32(1) - ax), ax
    b0, b1 = (np.float32(1) - ay)[:, None], ay[:, None]
    r0, r1 = blur[sy], blur[sy1]
    h0 = r0[:, sx] * a0 + r0[:, sx1] * a1
    h1 = r1[:, sx] * a0 + r1[:, sx1] * a1
    return (h0 * b0 + h1 * b1).astype(np.float32)


def calc_depth(orc, prev: np.ndarray, nxt: np.ndarray, p, flow0: np.ndarray | None = None) -> np.ndarray:
    """cv2.calcOpticalFlowFarneback(prev, nxt, flow0, *p) on frames of any depth (converted as convertTo(CV_32F) does: float64 is
    rounded to float32), restated on the oracle's stage functions.  flow0 None: flags = 0 (zero start); else
    OPTFLOW_USE_INITIAL_FLOW as initial_flow_ref.calc_init does it.  p: oracle.fb_oracle.Params (flags not read)."""
    prev = np.asarray(prev).astype(np.float32)
    nxt = np.asarray(nxt).astype(np.float32)
    H, W = prev.shape
    L = orc.num_layers(W, H, p)
    flow = None
    for k in range(L - 1, -1, -1):
        w, h, sigma, ksize = orc.layer_dims(W, H, p, k)
        if flow is None:
            flow = (np.zeros((h, w, 2), np.float32) if flow0 is None
                    else initial_flow_ref.top_layer_flow(flow0, w, h, k, p.pyr_scale))
        else:
            flow = orc.resize_flow(flow, w, h, 1.0 / p.pyr_scale)
        R0, R1 = (orc.polyexp(blur_resize_f32(img, w, h, ksize, sigma, orc), p.poly_n, p.poly_sigma) for img in (prev, nxt))
        M = orc.update_matrices(R0, R1, flow)
        for it in range(p.iterations):
            flow, M = orc.blur_iter(R0, R1, flow, M, p.winsize, it < p.iterations - 1)
    return flow


def pair16(W: int, H: int, pair_index: int = 0, k: float = 0.01):
    """A genuinely 16-bit pair: mavflow.synth.make_pair's scene (its closed-form texture, zoomed by k about an off-centre point, with
    the moving patch) quantised to 0 .. 65535 instead of 0 .. 255 -- the same well-behaved geometry as the u8 end-to-end tests, with
    the detail below one 8-bit step that only the full depth keeps."""
    from mavflow import synth
    rng = np.random.default_rng(20240 + pair_index)
    fx, fy, amp, phase = synth._texture_params(rng)
    x = np.arange(W, dtype=np.float64)
    y = np.arange(H, dtype=np.float64)
    t0 = synth._eval_separable(x, y, fx, fy, amp, phase)
    A = 32767.0 / np.abs(t0).max()
    t1 = synth._eval_separable(x - k * (x - 0.55 * W), y - k * (y - 0.45 * H), fx, fy, amp, phase)
    x0, y0 = W // 4, H // 4
    px, py = np.meshgrid(x[x0:x0 + 24] - 6.0, y[y0:y0 + 24] + 3.0)
    t1[y0:y0 + 24, x0:x0 + 24] = synth._eval_points(px, py, fx, fy, amp, phase)
    f0 = np.clip(np.rint(32767.5 + A * t0), 0, 65535).astype(np.uint16)
    f1 = np.clip(np.rint(32767.5 + A * t1), 0, 65535).astype(np.uint16)
    return f0, f1
