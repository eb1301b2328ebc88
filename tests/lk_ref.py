"""CPU restatement in numpy of the sparse optical-flow routines: Shi-Tomasi corners (cv2.goodFeaturesToTrack) and the pyramidal
Lucas-Kanade tracker (cv2.calcOpticalFlowPyrLK, 8-bit path), written from the arithmetic described in DESIGN.md ("Sparse optical flow"),
not from the product.  Plain and slow: integer arrays (int64) for every window sum, float32 arrays for the few operations after them,
in the stated order.  numpy fuses nothing and its float32 sqrt / division are correctly rounded, so a device implementation that keeps
its window sums in integers must agree with this file bit for bit.

No import from the product."""
import numpy as np

F = np.float32
W_BITS = 14
HIST_BINS = 104
# the ways a point leaves a level of the tracker: the first bounds test, the minimum-eigenvalue test, the bounds test of an iteration,
# |delta| <= epsilon, the oscillation rule, the iteration count (max-count-0: a count of 0, the loop never runs)
EXITS = ("outside-first", "min-eig", "outside-iter", "eps", "oscillation", "max-count", "max-count-0")


def reflect101(p, n):
    """BORDER_REFLECT_101 of integer positions p into [0, n) (any distance from the image)."""
    p = np.asarray(p, np.int64)
    if n == 1:
        return np.zeros_like(p)
    period = 2 * (n - 1)
    p = np.mod(p, period)
    return np.where(p >= n, period - p, p)


# ---- corners -----------------------------------------------------------------------------------------------------------------------
def min_eigen(img, block_size=7):
    """cornerMinEigenVal: Sobel 3x3 (REFLECT_101) as integers, integer box sums of the products over block_size x block_size
    (REFLECT_101 of the product images), then five float32 operations.  (H, W) float32."""
    g = np.asarray(img).astype(np.int64)
    H, W = g.shape
    ym, yp = reflect101(np.arange(H) - 1, H), reflect101(np.arange(H) + 1, H)
    xm, xp = reflect101(np.arange(W) - 1, W), reflect101(np.arange(W) + 1, W)
    dx = (g[ym][:, xp] + 2 * g[:, xp] + g[yp][:, xp]) - (g[ym][:, xm] + 2 * g[:, xm] + g[yp][:, xm])
    dy = (g[yp][:, xm] + 2 * g[yp] + g[yp][:, xp]) - (g[ym][:, xm] + 2 * g[ym] + g[ym][:, xp])
    r = block_size // 2
    ry, rx = reflect101(np.arange(-r, H + r), H), reflect101(np.arange(-r, W + r), W)

    def box(a):
        q = a[ry][:, rx]
        c = np.cumsum(np.cumsum(np.pad(q, ((1, 0), (1, 0))), 0), 1)
        b = block_size
        return c[b:, b:] - c[:-b, b:] - c[b:, :-b] + c[:-b, :-b]

    s = F(1.0 / (4 * block_size * 255))
    s2 = F(s * s)
    a = box(dx * dx).astype(F) * s2 * F(0.5)
    b = box(dx * dy).astype(F) * s2
    c = box(dy * dy).astype(F) * s2 * F(0.5)
    return (a + c) - np.sqrt((a - c) * (a - c) + b * b)


def corner_candidates(eig, quality_level=0.2):
    """(values, linear indices) of the interior local maxima above max(eig) * quality_level, in the total order of the pick: value
    descending, ties by linear index descending."""
    H, W = eig.shape
    thr = F(np.float64(eig.max()) * quality_level)
    e = np.where(eig > thr, eig, F(0))
    p = np.pad(e, 1, mode="constant", constant_values=-np.inf)
    nb = np.max([p[j:j + H, i:i + W] for j in range(3) for i in range(3)], axis=0)
    m = (e != 0) & (e == nb)
    m[0, :] = m[-1, :] = False
    m[:, 0] = m[:, -1] = False
    ys, xs = np.nonzero(m)
    v, idx = e[ys, xs], ys * W + xs
    order = np.lexsort((-idx, -v))
    return v[order], idx[order]


def good_features(img, max_corners=2000, quality_level=0.2, min_distance=7, block_size=7, want_values=False):
    """cv2.goodFeaturesToTrack(img, max_corners, quality_level, min_distance, blockSize=block_size): (n, 2) float32 (x, y)."""
    eig = min_eigen(img, block_size)
    W = eig.shape[1]
    v, idx = corner_candidates(eig, quality_level)
    xs, ys = idx % W, idx // W
    md2 = float(min_distance) * float(min_distance)
    sel = np.zeros((max_corners, 2), np.int64)
    vals = []
    n = 0
    for k in range(len(idx)):
        if n == max_corners:
            break
        if min_distance >= 1 and n:
            d = sel[:n] - (xs[k], ys[k])
            if np.any(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] < md2):
                continue
        sel[n] = (xs[k], ys[k])
        vals.append(v[k])
        n += 1
    out = sel[:n].astype(F)
    return (out, np.array(vals, F), len(idx)) if want_values else out


# ---- pyramid and derivatives ---------------------------------------------------------------------------------------------------------
def pyr_down(img):
    """pyrDown: 5x5 separable [1 4 6 4 1], REFLECT_101, ((w + 1) / 2, (h + 1) / 2), (sum + 128) >> 8."""
    a = np.asarray(img).astype(np.int64)
    h, w = a.shape
    oh, ow = (h + 1) // 2, (w + 1) // 2
    k = (1, 4, 6, 4, 1)
    rows = sum(k[j] * a[reflect101(2 * np.arange(oh) - 2 + j, h)] for j in range(5))
    out = sum(k[i] * rows[:, reflect101(2 * np.arange(ow) - 2 + i, w)] for i in range(5))
    return ((out + 128) >> 8).astype(np.uint8)


def build_pyramid(img, win=(21, 21), max_level=3):
    """Levels 0 .. L - 1; building stops before the first level whose width <= win_w or height <= win_h."""
    pyr = [np.asarray(img, np.uint8)]
    for _ in range(max_level):
        h, w = pyr[-1].shape
        if (w + 1) // 2 <= win[0] or (h + 1) // 2 <= win[1]:
            break
        pyr.append(pyr_down(pyr[-1]))
    return pyr


def scharr(img):
    """(h, w, 2) int16 = (Ix, Iy), REFLECT_101 at the image edge."""
    a = np.asarray(img).astype(np.int64)
    h, w = a.shape
    ym, yp = reflect101(np.arange(h) - 1, h), reflect101(np.arange(h) + 1, h)
    xm, xp = reflect101(np.arange(w) - 1, w), reflect101(np.arange(w) + 1, w)
    t0 = 3 * (a[ym] + a[yp]) + 10 * a
    t1 = a[yp] - a[ym]
    ix = t0[:, xp] - t0[:, xm]
    iy = 3 * (t1[:, xm] + t1[:, xp]) + 10 * t1
    return np.stack([ix, iy], axis=-1).astype(np.int16)


# ---- tracker -------------------------------------------------------------------------------------------------------------------------
def _floor_in(px, py, win, w, h):
    """floor of float32 coordinates and the bounds test  -win_w <= ix < w, -win_h <= iy < h; a non-finite coordinate fails it."""
    with np.errstate(invalid="ignore"):
        fx, fy = np.floor(px), np.floor(py)
        ok = np.isfinite(px) & np.isfinite(py) & (fx >= -win[0]) & (fx < w) & (fy >= -win[1]) & (fy < h)
    return fx, fy, ok


def _weights(a, b):
    s = F(1 << W_BITS)
    w00 = np.rint((F(1) - a) * (F(1) - b) * s).astype(np.int64)
    w01 = np.rint(a * (F(1) - b) * s).astype(np.int64)
    w10 = np.rint((F(1) - a) * b * s).astype(np.int64)
    return w00, w01, w10, (1 << W_BITS) - w00 - w01 - w10


def _window(img, ix, iy, win, wts, shift, zero_outside):
    """Bilinear integer window values (n, win_h, win_w) of a level at integer corners (ix, iy): (sum + half) >> shift.  The image
    continues by REFLECT_101; with zero_outside (the derivative planes) everything outside the level is 0."""
    h, w = img.shape
    xs = ix[:, None] + np.arange(win[0] + 1)
    ys = iy[:, None] + np.arange(win[1] + 1)
    if zero_outside:
        P = img[np.clip(ys, 0, h - 1)[:, :, None], np.clip(xs, 0, w - 1)[:, None, :]].astype(np.int64)
        P *= (((ys >= 0) & (ys < h))[:, :, None] & ((xs >= 0) & (xs < w))[:, None, :])
    else:
        P = img[reflect101(ys, h)[:, :, None], reflect101(xs, w)[:, None, :]].astype(np.int64)
    w00, w01, w10, w11 = (q[:, None, None] for q in wts)
    v = P[:, :-1, :-1] * w00 + P[:, :-1, 1:] * w01 + P[:, 1:, :-1] * w10 + P[:, 1:, 1:] * w11
    return (v + (1 << (shift - 1))) >> shift


def lk_track(prev, nxt, pts, win=(21, 21), max_level=3, max_count=30, epsilon=0.01, min_eig_threshold=1e-4, want_hist=False,
             want_exits=False):
    """cv2.calcOpticalFlowPyrLK(prev, nxt, pts, None, winSize=win, maxLevel=max_level, criteria=(EPS | COUNT, max_count, epsilon),
    minEigThreshold=min_eig_threshold) without the error output: (next_pts (n, 2) float32, status (n,) uint8[, iteration histogram]
    [, exits]).  exits (want_exits): how many (point, level) visits left the level by each way out, {(exit, "0" | "coarser"): count}
    over EXITS -- bookkeeping only, no arithmetic depends on it."""
    max_count = min(max(int(max_count), 0), 100)
    epsilon = min(max(float(epsilon), 0.0), 10.0)
    eps2 = epsilon * epsilon
    pts = np.asarray(pts, F).reshape(-1, 2)
    n = len(pts)
    pp, pn = build_pyramid(prev, win, max_level), build_pyramid(nxt, win, max_level)
    L = len(pp)
    out = np.zeros((n, 2), F)
    status = np.ones(n, np.uint8)
    hist = np.zeros(HIST_BINS, np.uint32)
    halfx, halfy = F((win[0] - 1) * 0.5), F((win[1] - 1) * 0.5)
    SC = F(1.0 / (1 << 20))
    exits = {(e, g): 0 for e in EXITS for g in ("0", "coarser")}

    def left(name, lv, count):
        exits[(name, "0" if lv == 0 else "coarser")] += int(count)

    for lv in range(L - 1, -1, -1):
        I, J = pp[lv], pn[lv]
        d = scharr(I)
        h, w = I.shape
        sc = F(1.0 / (1 << lv))
        px, py = pts[:, 0] * sc, pts[:, 1] * sc
        if lv == L - 1:
            nx, ny = px.copy(), py.copy()
        else:
            nx, ny = out[:, 0] * F(2), out[:, 1] * F(2)
        out[:, 0], out[:, 1] = nx, ny
        px, py = px - halfx, py - halfy
        fx, fy, ok = _floor_in(px, py, win, w, h)
        if lv == 0:
            status[~ok] = 0
        sel = np.nonzero(ok)[0]
        left("outside-first", lv, n - len(sel))
        if not len(sel):
            continue
        ix, iy = fx[sel].astype(np.int64), fy[sel].astype(np.int64)
        wts = _weights(px[sel] - fx[sel], py[sel] - fy[sel])
        Iw = _window(I, ix, iy, win, wts, 9, False)
        dx = _window(d[..., 0], ix, iy, win, wts, 14, True)
        dy = _window(d[..., 1], ix, iy, win, wts, 14, True)
        A11 = (dx * dx).sum(axis=(1, 2)).astype(F) * SC
        A12 = (dx * dy).sum(axis=(1, 2)).astype(F) * SC
        A22 = (dy * dy).sum(axis=(1, 2)).astype(F) * SC
        D = A11 * A22 - A12 * A12
        min_eig = (A22 + A11 - np.sqrt((A11 - A22) * (A11 - A22) + F(4) * A12 * A12)) / F(2 * win[0] * win[1])
        good = ~((min_eig < F(min_eig_threshold)) | (D < np.finfo(F).eps))
        if lv == 0:
            status[sel[~good]] = 0
        left("min-eig", lv, len(good) - np.count_nonzero(good))
        sel, Iw, dx, dy = sel[good], Iw[good], dx[good], dy[good]
        A11, A12, A22 = A11[good], A12[good], A22[good]
        D = F(1) / D[good]
        cx, cy = nx[sel] - halfx, ny[sel] - halfy           # the iterated position of the points still in `sel`
        pdx, pdy = np.zeros(len(sel), F), np.zeros(len(sel), F)
        act = np.arange(len(sel))                           # positions inside sel that still iterate
        iters = np.zeros(len(sel), np.int64)
        for j in range(max_count):
            if not len(act):
                break
            gx, gy, ok = _floor_in(cx[act], cy[act], win, w, h)
            if lv == 0:
                status[sel[act[~ok]]] = 0
            iters[act[~ok]] = j
            left("outside-iter", lv, len(ok) - np.count_nonzero(ok))
            act, gx, gy = act[ok], gx[ok], gy[ok]
            if not len(act):
                break
            wts = _weights(cx[act] - gx, cy[act] - gy)
            diff = _window(J, gx.astype(np.int64), gy.astype(np.int64), win, wts, 9, False) - Iw[act]
            b1 = (diff * dx[act]).sum(axis=(1, 2)).astype(F) * SC
            b2 = (diff * dy[act]).sum(axis=(1, 2)).astype(F) * SC
            ddx = (A12[act] * b2 - A22[act] * b1) * D[act]
            ddy = (A12[act] * b1 - A11[act] * b2) * D[act]
            cx[act] = cx[act] + ddx
            cy[act] = cy[act] + ddy
            ox, oy = cx[act] + halfx, cy[act] + halfy
            with np.errstate(invalid="ignore", over="ignore"):
                small = ddx.astype(np.float64) * ddx.astype(np.float64) + ddy.astype(np.float64) * ddy.astype(np.float64) <= eps2
                osc = (np.abs(ddx + pdx[act]).astype(np.float64) < 0.01) & (np.abs(ddy + pdy[act]).astype(np.float64) < 0.01)
            osc = osc & ~small & (j > 0)
            ox = np.where(osc, ox - ddx * F(0.5), ox)
            oy = np.where(osc, oy - ddy * F(0.5), oy)
            out[sel[act], 0], out[sel[act], 1] = ox, oy
            pdx[act], pdy[act] = ddx, ddy
            done = small | osc
            iters[act[done]] = j + 1
            left("eps", lv, np.count_nonzero(small))
            left("oscillation", lv, np.count_nonzero(osc))
            act = act[~done]
        iters[act] = max_count
        left("max-count" if max_count else "max-count-0", lv, len(act))
        hist += np.bincount(np.minimum(iters, HIST_BINS - 1), minlength=HIST_BINS).astype(np.uint32)
    res = (out, status, hist) if want_hist else (out, status)
    return res + (exits,) if want_exits else res
