"""CPU restatement in numpy of what cv2's sparse calls do beyond tests/lk_ref.py: calcOpticalFlowPyrLK's `err` output with the final
bounds test that comes with it, OPTFLOW_USE_INITIAL_FLOW, OPTFLOW_LK_GET_MIN_EIGENVALS, and goodFeaturesToTrack's Harris score.
Written from the arithmetic described in DESIGN.md ("Sparse optical flow", 4c) on lk_ref's own pieces (_floor_in, _weights, _window,
build_pyramid, scharr), not from the product.  OpenCV 4.x lkpyramid.cpp / corner.cpp restated, unpinned against a cv2 build.

No import from the product."""
import numpy as np

import gftt_pick_model as gm
import lk_ref
from lk_ref import F, HIST_BINS, _floor_in, _weights, _window, build_pyramid, reflect101, scharr

USE_INITIAL_FLOW, GET_MIN_EIGENVALS = 4, 8
S_MAX_33 = 8160 * 33 * 33          # the largest sum of |J - I| over a 33 x 33 window: values are (255 * 16384 + 256) >> 9 = 8160 at most


def err_of(S, win):
    """cv2's `errval * 1.f / (32 * w * h)`: a float32 DIVISION of the exact integer sum."""
    return F(S) / F(32 * win[0] * win[1])


def lk_track_err(prev, nxt, pts, next_pts0=None, flags=0, want_err=True, win=(21, 21), max_level=3, max_count=30, epsilon=0.01,
                 min_eig_threshold=1e-4, want_sums=False):
    """cv2.calcOpticalFlowPyrLK(prev, nxt, pts, next_pts0, winSize=win, maxLevel=max_level, criteria=(EPS | COUNT, max_count, epsilon),
    flags=flags, minEigThreshold=min_eig_threshold) -> (next_pts (n, 2) float32, status (n,) uint8, err (n,) float32, iteration
    histogram, exits).  want_err False: the call of a C++ caller with err == NULL (err comes back as zeros, no final bounds test).
    exits: lk_ref's {(exit, "0" | "coarser"): count} and one more key, "outside-final": points whose status the final bounds test
    cleared.  want_sums: a sixth value, the integer sums S (n,) int64 behind err (-1 where none was formed)."""
    if flags & ~(USE_INITIAL_FLOW | GET_MIN_EIGENVALS):
        raise ValueError(f"flags {flags}")
    max_count = min(max(int(max_count), 0), 100)
    epsilon = min(max(float(epsilon), 0.0), 10.0)
    eps2 = epsilon * epsilon
    pts = np.asarray(pts, F).reshape(-1, 2)
    n = len(pts)
    init = None
    if flags & USE_INITIAL_FLOW:
        init = np.asarray(next_pts0, F).reshape(-1, 2)
        assert init.shape == pts.shape
    min_eig_out = bool(flags & GET_MIN_EIGENVALS) and want_err
    pp, pn = build_pyramid(prev, win, max_level), build_pyramid(nxt, win, max_level)
    L = len(pp)
    out = np.zeros((n, 2), F)
    status = np.ones(n, np.uint8)
    err = np.zeros(n, F)
    sums = np.full(n, -1, np.int64)
    hist = np.zeros(HIST_BINS, np.uint32)
    halfx, halfy = F((win[0] - 1) * 0.5), F((win[1] - 1) * 0.5)
    SC = F(1.0 / (1 << 20))
    exits = {(e, g): 0 for e in lk_ref.EXITS for g in ("0", "coarser")}
    exits["outside-final"] = 0
    Iw0 = np.zeros((n, win[1], win[0]), np.int64)           # level 0's window of the previous frame, per point

    def left(name, lv, count):
        exits[(name, "0" if lv == 0 else "coarser")] += int(count)

    for lv in range(L - 1, -1, -1):
        I, J = pp[lv], pn[lv]
        d = scharr(I)
        h, w = I.shape
        sc = F(1.0 / (1 << lv))
        px, py = pts[:, 0] * sc, pts[:, 1] * sc
        if lv == L - 1:
            if init is not None:
                with np.errstate(invalid="ignore", over="ignore"):
                    nx, ny = init[:, 0] * sc, init[:, 1] * sc
            else:
                nx, ny = px.copy(), py.copy()
        else:
            with np.errstate(invalid="ignore", over="ignore"):
                nx, ny = out[:, 0] * F(2), out[:, 1] * F(2)
        out[:, 0], out[:, 1] = nx, ny
        px, py = px - halfx, py - halfy
        fx, fy, ok = _floor_in(px, py, win, w, h)
        if lv == 0:
            status[~ok] = 0
            err[~ok] = 0
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
        if min_eig_out:
            err[sel] = min_eig                              # before the threshold test; level 0 comes last, so its value stays
        good = ~((min_eig < F(min_eig_threshold)) | (D < np.finfo(F).eps))
        if lv == 0:
            status[sel[~good]] = 0
        left("min-eig", lv, len(good) - np.count_nonzero(good))
        sel, Iw, dx, dy = sel[good], Iw[good], dx[good], dy[good]
        if lv == 0:
            Iw0[sel] = Iw
        A11, A12, A22 = A11[good], A12[good], A22[good]
        D = F(1) / D[good]
        with np.errstate(invalid="ignore"):
            cx, cy = nx[sel] - halfx, ny[sel] - halfy
        pdx, pdy = np.zeros(len(sel), F), np.zeros(len(sel), F)
        act = np.arange(len(sel))
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

    if want_err and not (flags & GET_MIN_EIGENVALS):
        # the error pass, for the points still at status 1 after level 0's loop: q = out - halfWin, one more bounds test on its floor
        # (failing it clears the status, err stays 0), then the L1 difference between the next frame at q and level 0's window of the
        # previous frame, with the iteration's interpolation
        J = pn[0]
        h, w = J.shape
        live = np.nonzero(status == 1)[0]
        qx, qy = out[live, 0] - halfx, out[live, 1] - halfy
        fx, fy, ok = _floor_in(qx, qy, win, w, h)
        status[live[~ok]] = 0
        exits["outside-final"] = int(len(ok) - np.count_nonzero(ok))
        live, qx, qy, fx, fy = live[ok], qx[ok], qy[ok], fx[ok], fy[ok]
        if len(live):
            wts = _weights(qx - fx, qy - fy)
            Jw = _window(J, fx.astype(np.int64), fy.astype(np.int64), win, wts, 9, False)
            S = np.abs(Jw - Iw0[live]).sum(axis=(1, 2))
            assert S.max() < 1 << 24
            sums[live] = S
            err[live] = S.astype(F) / F(32 * win[0] * win[1])
    res = (out, status, err, hist, exits)
    return res + (sums,) if want_sums else res


# ---- corners: the Harris score ---------------------------------------------------------------------------------------------------------
def harris_response(img, block_size=3, k=0.04):
    """cornerHarris as goodFeaturesToTrack(useHarrisDetector=True) calls it: lk_ref.min_eigen's integer Sobel pairs, box sums and scale,
    then a = xx s2, b = xy s2, c = yy s2, t = a + c, (a c - b b) - (k t) t in float32 in this order, k rounded to float32 once.
    (H, W) float32; values of either sign."""
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
    a = box(dx * dx).astype(F) * s2
    b = box(dx * dy).astype(F) * s2
    c = box(dy * dy).astype(F) * s2
    t = a + c
    return (a * c - b * b) - (F(k) * t) * t


def corner_response(img, block_size=7, use_harris=False, k=0.04):
    return harris_response(img, block_size, k) if use_harris else lk_ref.min_eigen(img, block_size)


def good_features_score(img, mask=None, max_corners=2000, quality_level=0.2, min_distance=7, block_size=7, use_harris=False, k=0.04):
    """cv2.goodFeaturesToTrack(img, max_corners, quality_level, min_distance, mask=mask, blockSize=block_size,
    useHarrisDetector=use_harris, k=k) -> (n, 2) float32: the score map, gftt_pick_model's masked candidates, its sort and pick.
    A candidate is above max * quality_level, which is positive whenever there is one, so the keys' raw value bits order as the
    values do even though the map has negative entries."""
    resp = corner_response(img, block_size, use_harris, k)
    v, idx = gm.masked_candidates(resp, mask, quality_level)
    assert not len(v) or v.min() > 0
    H, W = resp.shape
    return gm.good_features_from_keys(gm.keys_of(v, idx), W, H, max_corners, min_distance)
