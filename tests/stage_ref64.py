"""TEST INFRASTRUCTURE -- the Farneback stages restated in float64 numpy, from the mathematics rather than from any C file.

oracle/farneback_oracle.c and the library's kernels share their structure (and, through csrc/mavflow.cpp, close relatives of their
host-side constants), so a slip the two have in common passes every GPU-vs-oracle comparison.  This module is written from the
definitions instead (OpenCV 4.x optflowgf.cpp as SURVEY.md Appendix A states it):

  blur_resize      separable Gaussian (getGaussianKernel: the fixed [1/4, 1/2, 1/4] for ksize 3 at sigma 0, else the normalised
                   closed form), BORDER_REFLECT_101, then resize(INTER_LINEAR) with half-pixel centres, clamped at the edges
  polyexp          the weighted least-squares fit of 1, x, y, x^2, y^2, xy under the weight g(x) g(y), replicated borders; the
                   four inverse moments come from np.linalg.inv of the 6 x 6 moment matrix
  update_matrices  the displaced R1 sample (bilinear, only when the whole 2 x 2 neighbourhood lies inside the image), the averaged
                   coefficients, the 5-pixel border weights, M = (A^T A, A^T b) in five planes
  sweep            (2m + 1)^2 box sums of M (m = winsize // 2, replicated borders) divided by winsize^2, the 2 x 2 solve with
                   + 1e-3 in the determinant, and M' = update_matrices of the new flow
  upsample_flow    resize(INTER_LINEAR) of the coarser layer's flow times 1 / pyr_scale

Every sum and product is float64.  Two quantities are float32 by DEFINITION and are computed as float32 here too, because OpenCV
computes them in float and they select which pixels are read: a resize's sample position ((d + 0.5) * S / s - 0.5, cast to float)
and a displaced position (x + dx, a float sum).  Their rounding moves a sample by up to half an ulp of the coordinate (1.2e-4 px at
x ~ 4000), far more than float32 rounding of the values; an implementation that computes them in double is a different function.

Each stage also returns, where it is asked for, the MAGNITUDE of its result: the same expression evaluated on absolute values
(|taps|, |inputs|).  A float32 evaluation of the expression differs from the float64 one by at most a small multiple of
2^-24 x magnitude x (number of roundings on the longest path); tests/test_stage_ref64_cpu.py holds the C oracle to that.
Layouts: images (h, w); R and M (h, w, 5) interleaved, as the oracle returns them; flow (h, w, 2).
"""
from __future__ import annotations

import numpy as np

EPS32 = 2.0 ** -24
BORDER_WEIGHTS = (0.14, 0.14, 0.4472, 0.4472, 0.4472)     # optflowgf.cpp FarnebackUpdateMatrices: border[BORDER] (BORDER = 5)


# ---- GaussianBlur + resize(INTER_LINEAR) ------------------------------------------------------------------------------
def gaussian_taps(ksize: int, sigma: float) -> np.ndarray:
    """getGaussianKernel(ksize, sigma): the small fixed kernels for sigma <= 0 (only ksize 3 is used here), else the closed form."""
    if sigma <= 0 and ksize == 3:
        return np.array([0.25, 0.5, 0.25])
    if sigma <= 0:
        sigma = ((ksize - 1) * 0.5 - 1) * 0.3 + 0.8
    x = np.arange(ksize) - (ksize - 1) / 2
    g = np.exp(-x * x / (2 * sigma * sigma))
    return g / g.sum()


def _reflect101(i, n):
    if n == 1:
        return np.zeros_like(i)
    period = 2 * n - 2
    i = np.abs(i) % period
    return np.where(i >= n, period - i, i)


def _filter_axis(a, taps, axis):
    r = len(taps) // 2
    n = a.shape[axis]
    out = np.zeros(a.shape)
    for t, c in enumerate(taps):
        out += c * np.take(a, _reflect101(np.arange(n) + t - r, n), axis=axis)
    return out


def resize_coords(S: int, d: int):
    """Source index, next index and weight of each of d destination samples along an axis of S source samples (INTER_LINEAR,
    half-pixel centres): position p = float32((o + 0.5) * S / d - 0.5), i0 = floor(p), weight p - i0; clamped to the edge sample
    with weight 0 outside [0, S - 1]."""
    p = np.float32((np.arange(d) + 0.5) * (S / d) - 0.5).astype(np.float64)
    i0 = np.floor(p).astype(np.int64)
    f = p - i0
    lo, hi = i0 < 0, i0 >= S - 1
    f[lo | hi] = 0.0
    i0[lo] = 0
    i0[hi] = S - 1
    return i0, np.minimum(i0 + 1, S - 1), f


def resize_linear(a: np.ndarray, w: int, h: int) -> np.ndarray:
    """resize(a, (w, h), INTER_LINEAR) of a 2-D or (H, W, c) array; a copy when the size does not change."""
    H, W = a.shape[:2]
    a = np.asarray(a, np.float64)
    if (w, h) == (W, H):
        return a.copy()
    x0, x1, fx = resize_coords(W, w)
    y0, y1, fy = resize_coords(H, h)
    ex = (slice(None), ) + (None,) * (a.ndim - 2)
    fx = fx[ex].T if a.ndim == 2 else fx[:, None]
    fy = fy[:, None] if a.ndim == 2 else fy[:, None, None]
    rows0 = a[y0][:, x0] * (1 - fx) + a[y0][:, x1] * fx
    rows1 = a[y1][:, x0] * (1 - fx) + a[y1][:, x1] * fx
    return rows0 * (1 - fy) + rows1 * fy


def blur_resize(img: np.ndarray, w: int, h: int, ksize: int, sigma: float) -> np.ndarray:
    """convertTo(float) -> GaussianBlur((ksize, ksize), sigma) -> resize((w, h), INTER_LINEAR), in float64.  (All taps are positive
    and the image is non-negative: the result is its own magnitude.)  The blur is evaluated only at the rows and columns the resize
    reads (the separable filter's passes commute in exact arithmetic)."""
    g = gaussian_taps(ksize, sigma)
    img = np.asarray(img, np.float64)
    H, W = img.shape
    if (w, h) == (W, H):
        return _filter_axis(_filter_axis(img, g, 1), g, 0)
    x0, x1, fx = resize_coords(W, w)
    y0, y1, fy = resize_coords(H, h)
    r = len(g) // 2
    need_y, need_x = np.unique(np.concatenate([y0, y1])), np.unique(np.concatenate([x0, x1]))
    cols = sum(c * img[_reflect101(need_y + t - r, H)] for t, c in enumerate(g))             # (rows needed, W)
    b = sum(c * cols[:, _reflect101(need_x + t - r, W)] for t, c in enumerate(g))            # (rows needed, columns needed)
    iy, ix = np.searchsorted(need_y, [y0, y1]), np.searchsorted(need_x, [x0, x1])
    rows0 = b[iy[0]][:, ix[0]] * (1 - fx) + b[iy[0]][:, ix[1]] * fx
    rows1 = b[iy[1]][:, ix[0]] * (1 - fx) + b[iy[1]][:, ix[1]] * fx
    return rows0 * (1 - fy[:, None]) + rows1 * fy[:, None]


# ---- FarnebackPolyExp --------------------------------------------------------------------------------------------------
def poly_constants(n: int, sigma: float):
    """(x, g, (ig11, ig03, ig33, ig55)): the normalised Gaussian weight on [-n, n] and the four distinct entries of the inverse of the
    moment matrix G_ij = sum_(x, y) g(x) g(y) b_i b_j of the basis b = (1, x, y, x^2, y^2, xy)."""
    if sigma < np.finfo(np.float32).eps:
        sigma = n * 0.3
    x = np.arange(-n, n + 1, dtype=np.float64)
    g = np.exp(-x * x / (2 * sigma * sigma))
    g /= g.sum()
    X, Y = np.meshgrid(x, x)
    wgt = np.outer(g, g)
    basis = [np.ones_like(X), X, Y, X * X, Y * Y, X * Y]
    G = np.array([[np.sum(wgt * bi * bj) for bj in basis] for bi in basis])
    inv = np.linalg.inv(G)
    return x, g, (inv[1, 1], inv[0, 3], inv[3, 3], inv[5, 5])


def polyexp(I: np.ndarray, n: int, sigma: float, magnitude: bool = False) -> np.ndarray:
    """(h, w, 5) = (r_y, r_x, r_yy, r_xx, r_xy): the fitted coefficients of y, x, y^2, x^2 and xy around every pixel (OpenCV's channel
    order), replicated borders.  magnitude=True: the same sums over |taps| x |I| with |ig| (the scale of the rounding error)."""
    x, g, ig = poly_constants(n, sigma)
    ig11, ig03, ig33, ig55 = ig
    xg, xxg = x * g, x * x * g
    if magnitude:
        xg, ig03 = np.abs(xg), abs(ig03)
    I = np.asarray(I, np.float64)
    h, w = I.shape
    rows = np.clip(np.arange(h)[:, None] + np.arange(-n, n + 1)[None, :], 0, h - 1)      # replicate
    cols = np.clip(np.arange(w)[:, None] + np.arange(-n, n + 1)[None, :], 0, w - 1)
    v0, v1, v2 = np.zeros((h, w)), np.zeros((h, w)), np.zeros((h, w))                     # vertical: sum g, y g, y^2 g
    for t in range(2 * n + 1):
        s = I[rows[:, t]]
        v0 += g[t] * s
        v1 += xg[t] * s
        v2 += xxg[t] * s
    b = np.zeros((6, h, w))                                                               # horizontal: b1 .. b6
    for t in range(2 * n + 1):
        c = cols[:, t]
        a0, a1, a2 = v0[:, c], v1[:, c], v2[:, c]
        b[0] += g[t] * a0          # 1
        b[1] += xg[t] * a0         # x
        b[2] += g[t] * a1          # y
        b[3] += xxg[t] * a0        # x^2
        b[4] += g[t] * a2          # y^2
        b[5] += xg[t] * a1         # xy
    R = np.empty((h, w, 5))
    R[..., 0] = b[2] * ig11
    R[..., 1] = b[1] * ig11
    R[..., 2] = b[0] * ig03 + b[4] * ig33
    R[..., 3] = b[0] * ig03 + b[3] * ig33
    R[..., 4] = b[5] * ig55
    return np.abs(R) if magnitude else R


# ---- FarnebackUpdateMatrices -------------------------------------------------------------------------------------------
def border_scale(w: int, h: int) -> np.ndarray:
    """(h, w) weight of the 5-pixel frame: border[d] at distance d < 5 from an edge, products where two edges meet (and where a
    narrow image puts a pixel within 5 of both opposite edges).  The weight is applied only where OpenCV's frame test
    (unsigned)(x - 5) >= (unsigned)(w - 10) or its y twin holds: for w, h >= 10 that is "within 5 of an edge", below 10 the
    unsigned comparison leaves some of those pixels at weight 1 -- part of the definition, restated as it is."""
    def axis(n):
        s = np.ones(n)
        i = np.arange(n)
        for d, b in enumerate(BORDER_WEIGHTS):
            s[i == d] *= b
            s[i == n - 1 - d] *= b
        return s, ((i - 5) & 0xFFFFFFFF) >= ((n - 10) & 0xFFFFFFFF)
    sy, ty = axis(h)
    sx, tx = axis(w)
    return np.where(ty[:, None] | tx[None, :], sy[:, None] * sx[None, :], 1.0)


def displaced(flow: np.ndarray):
    """The displaced positions x + dx, y + dy -- float32 sums by definition -- as float64, with their integer parts."""
    flow = np.asarray(flow, np.float32)
    h, w = flow.shape[:2]
    fx = (np.arange(w, dtype=np.float32)[None, :] + flow[..., 0]).astype(np.float64)
    fy = (np.arange(h, dtype=np.float32)[:, None] + flow[..., 1]).astype(np.float64)
    return fx, fy, np.floor(fx).astype(np.int64), np.floor(fy).astype(np.int64)


def inside(flow: np.ndarray) -> np.ndarray:
    """Where the displaced position's 2 x 2 neighbourhood lies inside the image (the R1 sample is taken)."""
    h, w = flow.shape[:2]
    _, _, x1, y1 = displaced(flow)
    return (x1 >= 0) & (x1 < w - 1) & (y1 >= 0) & (y1 < h - 1)


def update_matrices(R0: np.ndarray, R1: np.ndarray, flow: np.ndarray, magnitude: bool = False):
    """M (h, w, 5) = (G11, G12, G22, h1, h2) of every pixel for the given flow; with magnitude=True also the magnitude of each
    entry (the same expression on absolute values) as a second array."""
    R0 = np.asarray(R0, np.float64); R1 = np.asarray(R1, np.float64)
    flow64 = np.asarray(flow, np.float32).astype(np.float64)
    h, w = flow64.shape[:2]
    dx, dy = flow64[..., 0], flow64[..., 1]
    fx, fy, x1, y1 = displaced(flow)
    ins = (x1 >= 0) & (x1 < w - 1) & (y1 >= 0) & (y1 < h - 1)
    xs, ys = np.where(ins, x1, 0), np.where(ins, y1, 0)
    ax, ay = fx - x1, fy - y1
    wts = [(1 - ax) * (1 - ay), ax * (1 - ay), (1 - ax) * ay, ax * ay]
    xn, yn = np.minimum(xs + 1, w - 1), np.minimum(ys + 1, h - 1)         # (only read where inside: then xs + 1 < w, ys + 1 < h)
    nb = [R1[ys, xs], R1[ys, xn], R1[yn, xs], R1[yn, xn]]

    def assemble(R0, nb, dx, dy, sgn):
        s = sum(wt[..., None] * v for wt, v in zip(wts, nb))
        s = np.where(ins[..., None], s, 0.0)
        # averaged quadratic terms where the sample is taken; R0's alone (xy halved, as the average with a zero would) where not
        r4 = np.where(ins, (R0[..., 2] + s[..., 2]) * 0.5, R0[..., 2])
        r5 = np.where(ins, (R0[..., 3] + s[..., 3]) * 0.5, R0[..., 3])
        r6 = np.where(ins, (R0[..., 4] + s[..., 4]) * 0.25, R0[..., 4] * 0.5)
        r2 = (R0[..., 0] + sgn * s[..., 0]) * 0.5 + r4 * dy + r6 * dx
        r3 = (R0[..., 1] + sgn * s[..., 1]) * 0.5 + r6 * dy + r5 * dx
        return r2, r3, r4, r5, r6

    sc = border_scale(w, h)

    def matrices(r):
        r2, r3, r4, r5, r6 = (v * sc for v in r)
        return np.stack([r4 * r4 + r6 * r6, (r4 + r5) * r6, r5 * r5 + r6 * r6, r4 * r2 + r6 * r3, r6 * r2 + r5 * r3], axis=-1)

    M = matrices(assemble(R0, nb, dx, dy, -1.0))
    if not magnitude:
        return M
    mag = matrices(assemble(np.abs(R0), [np.abs(v) for v in nb], np.abs(dx), np.abs(dy), 1.0))
    return M, mag


# ---- FarnebackUpdateFlow_Blur ------------------------------------------------------------------------------------------
def box_sums(M: np.ndarray, m: int) -> np.ndarray:
    """sum over the (2m + 1)^2 window around every pixel, borders replicated, of every plane of M (h, w, c)."""
    M = np.asarray(M, np.float64)
    h, w = M.shape[:2]
    rows = np.clip(np.arange(-m, h + m), 0, h - 1)
    cols = np.clip(np.arange(-m, w + m), 0, w - 1)
    P = M[rows][:, cols]
    c = np.zeros((P.shape[0] + 1, P.shape[1] + 1) + M.shape[2:])
    c[1:, 1:] = P.cumsum(0).cumsum(1)
    k = 2 * m + 1
    return c[k:, k:] - c[:-k, k:] - c[k:, :-k] + c[:-k, :-k]


def solve(G: np.ndarray):
    """The per-pixel 2 x 2 solve of a sweep from the scaled sums G = (g11, g12, g22, h1, h2): flow (h, w, 2)."""
    g11, g12, g22, h1, h2 = (G[..., i] for i in range(5))
    idet = 1.0 / (g11 * g22 - g12 * g12 + 1e-3)
    return np.stack([(g11 * h2 - g12 * h1) * idet, (g22 * h1 - g12 * h2) * idet], axis=-1)


def sweep_system(M: np.ndarray, winsize: int) -> np.ndarray:
    """The scaled window sums (h, w, 5) a sweep solves from: box sums over (2m + 1)^2 pixels, m = winsize // 2, divided by winsize^2
    (OpenCV divides by block_size^2, not by the window's pixel count)."""
    return box_sums(M, winsize // 2) / float(winsize * winsize)


def sweep(R0, R1, M, winsize: int, update: bool = True):
    """One FarnebackUpdateFlow_Blur sweep: (flow, M' or None).  M' is update_matrices of the new flow rounded to float32 (the flow is
    stored as float32 before it is used again)."""
    flow = solve(sweep_system(M, winsize))
    return flow, (update_matrices(R0, R1, flow.astype(np.float32)) if update else None)


def system_bound_terms(G: np.ndarray, d: np.ndarray):
    """For the systems G (h, w, 5) and their solutions d (h, w, 2): ||G^-1|| ( ||G|| ||d|| + ||h|| ) in the 2-norm, the factor by which a
    relative perturbation of the window sums moves the solution.  G^-1 is the solve's regularised inverse adj(G) / (det + 1e-3)."""
    g11, g12, g22, h1, h2 = (np.asarray(G[..., i], np.float64) for i in range(5))
    half_tr, half_diff = (g11 + g22) / 2, np.hypot((g11 - g22) / 2, g12)
    lmax = np.abs(half_tr) + half_diff                                    # spectral norm of the symmetric 2 x 2 (and of its adjugate)
    inv_norm = lmax / np.abs(g11 * g22 - g12 * g12 + 1e-3)
    return inv_norm * (lmax * np.hypot(d[..., 0], d[..., 1]) + np.hypot(h1, h2))


# ---- the coarser layer's flow, upsampled --------------------------------------------------------------------------------
def upsample_flow(flow_coarse: np.ndarray, w: int, h: int, mul: float) -> np.ndarray:
    """resize(flow_coarse, (w, h), INTER_LINEAR) * mul."""
    return resize_linear(np.asarray(flow_coarse, np.float64), w, h) * mul
