"""TEST INFRASTRUCTURE -- the checker of OPTFLOW_USE_INITIAL_FLOW (cv2.calcOpticalFlowFarneback with an initial flow field).

Composes the pyramid exactly as oracle.fb_oracle.Oracle.pyramid does, from the same stage functions (blur_resize, polyexp,
update_matrices, blur_iter, resize_flow), and differs at one point only, the coarsest layer computed (k = L - 1), where
optflowgf.cpp (FarnebackOpticalFlowImpl::calc) does

    flow = resize(flow0, (w_k, h_k), INTER_AREA);  flow *= scale_k        # scale_k = pyr_scale^k, a repeated double product

PARITY UNPINNED, like the rest of the flow: cv2 is not installed here.  Restated from the published OpenCV 4.x sources:
  * resize.cpp: cv::resize copies when dsize == ssize.  Otherwise scale = 1. / (dsize / ssize) in double; when both ratios are
    whole numbers (|scale - saturate_cast<int>(scale)| < DBL_EPSILON on both axes) the fast-area path runs, else
    computeResizeAreaTab + resizeArea_<float, float> (float weights, float accumulation in table order: x taps, then rows).
  * fast-area for CV_32FC2 (from memory of resizeAreaFast_Invoker): the SIMD helper ResizeAreaFastVec_SIMD_32f serves 2x2 blocks of
    cn 1 / 4 only, so with two channels every output is the scalar loop -- sum over the block in ofs order (rows, then columns),
    the CV_ENABLE_UNROLLED grouping sum += ((a + b) + c) + d four at a time, then the rest one by one -- times 1.f / area.
  * `flow *= scale` (from memory): Mat::convertTo(alpha = scale), a copy when |scale - 1| < DBL_EPSILON, else
    dst = src * (float)scale + 0.f per element (the two only differ from one float multiply on a negative zero).
"""
from __future__ import annotations

import numpy as np

from oracle import pyramid_oracle

DBL_EPS = np.finfo(np.float64).eps


def _passes(tab):
    """pyramid_oracle.area_tab split into passes: pass r holds the r-th entry of every destination index (accumulation order)."""
    passes, seen = [], {}
    for di, si, a in tab:
        r = seen.get(di, 0)
        seen[di] = r + 1
        while len(passes) <= r:
            passes.append(([], [], []))
        passes[r][0].append(di); passes[r][1].append(si); passes[r][2].append(a)
    return [(np.array(d), np.array(s), np.array(a, np.float32)) for d, s, a in passes]


def area_ratio(ssize: int, dsize: int):
    """(scale, saturate_cast<int>(scale), whole number?) of one axis as hal::resize computes them."""
    scale = 1.0 / (dsize / ssize)
    iscale = int(np.rint(scale))
    return scale, iscale, abs(scale - iscale) < DBL_EPS


def resize_area_flow(flow0: np.ndarray, w: int, h: int) -> np.ndarray:
    """cv2.resize(flow0, (w, h), interpolation=cv2.INTER_AREA) for a float32 (H, W, 2) field, shrinking or the same size."""
    flow0 = np.ascontiguousarray(flow0, np.float32)
    H, W = flow0.shape[:2]
    if (w, h) == (W, H):
        return flow0.copy()
    sx, ix, whole_x = area_ratio(W, w)
    sy, iy, whole_y = area_ratio(H, h)
    assert sx >= 1 and sy >= 1, "INTER_AREA enlarging is not restated"
    if whole_x and whole_y:                                    # resizeAreaFast_<float, float>
        area = ix * iy
        blk = flow0[:h * iy, :w * ix].reshape(h, iy, w, ix, 2)
        terms = [blk[:, k // ix, :, k % ix] for k in range(area)]
        s = np.zeros((h, w, 2), np.float32)
        k = 0
        while k <= area - 4:
            s = s + (((terms[k] + terms[k + 1]) + terms[k + 2]) + terms[k + 3])
            k += 4
        while k < area:
            s = s + terms[k]
            k += 1
        return s * (np.float32(1) / np.float32(area))
    out = np.empty((h, w, 2), np.float32)
    xp, yp = _passes(pyramid_oracle.area_tab(W, w, sx)), _passes(pyramid_oracle.area_tab(H, h, sy))
    for c in range(2):
        S = flow0[..., c]
        buf = np.zeros((H, w), np.float32)
        for di, si, a in xp:
            buf[:, di] = buf[:, di] + S[:, si] * a[None, :]
        acc = np.zeros((h, w), np.float32)
        for di, si, b in yp:
            acc[di, :] = acc[di, :] + b[:, None] * buf[si, :]
        out[..., c] = acc
    return out


def times_scale(flow: np.ndarray, scale: float) -> np.ndarray:
    """flow *= scale (Mat::convertTo)."""
    if abs(scale - 1.0) < DBL_EPS:
        return flow.copy()
    return flow * np.float32(scale) + np.float32(0)


def top_layer_flow(flow0: np.ndarray, w: int, h: int, k: int, pyr_scale: float) -> np.ndarray:
    scale = 1.0
    for _ in range(k):
        scale *= pyr_scale
    return times_scale(resize_area_flow(flow0, w, h), scale)


def calc_init(orc, prev, nxt, flow0, p):
    """cv2.calcOpticalFlowFarneback(prev, nxt, flow0, *p, flags=OPTFLOW_USE_INITIAL_FLOW) restated on the oracle's stage functions.
    p: oracle.fb_oracle.Params (its flags field is not read)."""
    prev = np.ascontiguousarray(prev, np.uint8); nxt = np.ascontiguousarray(nxt, np.uint8)
    H, W = prev.shape
    assert flow0.shape == (H, W, 2)
    L = orc.num_layers(W, H, p)
    flow = None
    for k in range(L - 1, -1, -1):
        w, h, sigma, ksize = orc.layer_dims(W, H, p, k)
        flow = top_layer_flow(flow0, w, h, k, p.pyr_scale) if flow is None else orc.resize_flow(flow, w, h, 1.0 / p.pyr_scale)
        R0, R1 = (orc.polyexp(orc.blur_resize(img, w, h, ksize, sigma), p.poly_n, p.poly_sigma) for img in (prev, nxt))
        M = orc.update_matrices(R0, R1, flow)
        for it in range(p.iterations):
            flow, M = orc.blur_iter(R0, R1, flow, M, p.winsize, it < p.iterations - 1)
    return flow


def textured_translation(W: int, H: int, shift, seed: int = 5):
    """The textured pair of tests/test_gpu_analytic.py (closed-form texture, frame 1 = frame 0 moved by `shift` px)."""
    from mavflow import synth
    rng = np.random.default_rng(seed)
    fx, fy, amp, ph = synth._texture_params(rng)
    x = np.arange(W, dtype=np.float64)
    y = np.arange(H, dtype=np.float64)
    t0 = synth._eval_separable(x, y, fx, fy, amp, ph)
    t1 = synth._eval_separable(x - shift[0], y - shift[1], fx, fy, amp, ph)
    A = 119.5 / np.abs(t0).max()
    f0 = np.rint(127.5 + A * t0).astype(np.uint8)
    f1 = np.clip(np.rint(127.5 + A * t1), 0, 255).astype(np.uint8)
    return f0, f1


def smooth_initial_flow(W: int, H: int, seed: int = 3, gain: float = 0.8, noise: float = 0.3, k: float = 0.01) -> np.ndarray:
    """A non-zero initial field: synth.true_flow scaled, plus noise (what a previous pair's flow looks like)."""
    from mavflow import synth
    rng = np.random.default_rng(seed)
    f = synth.true_flow(W, H, k) * np.float32(gain)
    return (f + rng.normal(0, noise, f.shape)).astype(np.float32)
