"""numpy restatement of the global-motion branch (Detector.get_transformation_matrix / flow_vec_subtract).

Two halves with different standing:

* the full-frame arithmetic (global_motion, subtract, to_gray) is the reference's own numpy expressions, literally
  (detector.py:126-128,164-185, im_helpers.py:188-199): tests/golden/global_motion.npz, recorded from the reference itself, pins it;
* the fit (find_homography) is the fixed-order restatement csrc/kernels_motion.hip shares operation for operation: float64 only,
  + - * / sqrt fabs and comparisons, every sum over points in plain index order with one accumulator per entry (np.cumsum is
  sequential; np.sum is pairwise and is not used).  It follows OpenCV's method-0 findHomography in structure (normalised DLT, then
  Levenberg-Marquardt on the reprojection error) but is NOT pinned against cv2: DESIGN.md section 4d lists what that would need.
"""
import math

import numpy as np

DBL_EPSILON = float(np.finfo(np.float64).eps)
JACOBI_SWEEPS = 30            # fixed bound of the cyclic Jacobi loop
LM_ITERATIONS = 10            # fixed bound of the refinement
RANK_RATIO = 1e-12            # second smallest eigenvalue of LtL <= RANK_RATIO * largest: the pairs do not determine a homography


# ---- the full-frame part: the reference's expressions ------------------------------------------------------------------------
def coords_new(coords, flow_uv):
    """detector.py:127-128 for coords (n, 2) int64 of (x, y)."""
    coords = np.asarray(coords)
    return coords.astype(np.float64) + flow_uv[coords[:, 1], coords[:, 0]]


def global_motion(M, H, W, dtype=np.float32):
    """detector.py:164-176: M is the homography (rows 0 and 1 are read) or the 2x3 affine matrix, float64."""
    M = np.asarray(M, np.float64)
    x_coords = np.tile(np.arange(W), (H, 1))
    y_coords = np.tile(np.arange(H), (W, 1)).T
    gm = np.zeros((H, W, 2), dtype)
    gm[..., 0] = M[0, 0] * x_coords + M[0, 1] * y_coords + M[0, 2] - x_coords
    gm[..., 1] = M[1, 0] * x_coords + M[1, 1] * y_coords + M[1, 2] - y_coords
    return gm


def to_gray(mag):
    """One channel of im_helpers.to_rgb(mag) (to_int with normalize, max_value None)."""
    with np.errstate(invalid="ignore", divide="ignore"):
        img = np.abs(mag) * 255 / np.max(mag)
        return np.around(img).astype(np.uint8)


def subtract(flow_uv, M):
    """detector.py:164-185 without the window search: dict of global_motion, warped, mag, flow_max (row, col), gray."""
    flow_uv = np.asarray(flow_uv)
    H, W = flow_uv.shape[:2]
    gm = global_motion(M, H, W, flow_uv.dtype)
    warped = gm - flow_uv
    mag = np.sqrt(warped[..., 0] ** 2.0 + warped[..., 1] ** 2.0)
    flow_max = np.unravel_index(mag.argmax(), mag.shape)
    return dict(global_motion=gm, warped=warped, mag=mag, flow_max=(int(flow_max[0]), int(flow_max[1])), gray=to_gray(mag))


# ---- the fit -----------------------------------------------------------------------------------------------------------------
def _seq(a):
    """Sum of a 1-d float64 array in index order with one accumulator."""
    return float(np.cumsum(a)[-1])


def jacobi_eigen(A, n):
    """Cyclic Jacobi on the symmetric n x n matrix A (list of lists, changed in place): rows p < q in row-major order, at most
    JACOBI_SWEEPS sweeps.  Returns (eigenvalues = diagonal, V with the eigenvectors as columns)."""
    V = [[1.0 if i == j else 0.0 for j in range(n)] for i in range(n)]
    for sweep in range(JACOBI_SWEEPS):
        off = 0.0
        for p in range(n - 1):
            for q in range(p + 1, n):
                off = off + abs(A[p][q])
        if not (off > 0.0):              # zero (converged) or NaN: stop
            break
        for p in range(n - 1):
            for q in range(p + 1, n):
                apq = A[p][q]
                if apq == 0.0:
                    continue
                g = 100.0 * abs(apq)
                app, aqq = A[p][p], A[q][q]
                if sweep > 3 and abs(app) + g == abs(app) and abs(aqq) + g == abs(aqq):
                    A[p][q] = 0.0
                    A[q][p] = 0.0
                    continue
                theta = (aqq - app) / (2.0 * apq)
                t = 1.0 / (abs(theta) + math.sqrt(theta * theta + 1.0)) if math.isfinite(theta) else 0.0
                if theta < 0.0:
                    t = -t
                c = 1.0 / math.sqrt(t * t + 1.0)
                s = t * c
                for k in range(n):
                    akp, akq = A[k][p], A[k][q]
                    A[k][p] = c * akp - s * akq
                    A[k][q] = s * akp + c * akq
                for k in range(n):
                    apk, aqk = A[p][k], A[q][k]
                    A[p][k] = c * apk - s * aqk
                    A[q][k] = s * apk + c * aqk
                for k in range(n):
                    vkp, vkq = V[k][p], V[k][q]
                    V[k][p] = c * vkp - s * vkq
                    V[k][q] = s * vkp + c * vkq
    return [A[i][i] for i in range(n)], V


def dlt_rows(src, dst):
    """The normalisation and the two DLT rows of every pair.  Returns None when a coordinate has no spread, else
    (Lx, Ly: lists of 9 arrays (n), (cM, cm, sM, sm)): centroids and per-axis scales n / sum |v - centroid| of src (M) and dst (m)."""
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    n = src.shape[0]
    fn = float(n)
    c = [_seq(src[:, 0]) / fn, _seq(src[:, 1]) / fn, _seq(dst[:, 0]) / fn, _seq(dst[:, 1]) / fn]
    cols = [src[:, 0], src[:, 1], dst[:, 0], dst[:, 1]]
    dev = [_seq(np.abs(cols[k] - c[k])) for k in range(4)]
    for d in dev:
        if not (d > DBL_EPSILON) or not math.isfinite(d):
            return None
    s = [fn / d for d in dev]
    X, Y = (cols[0] - c[0]) * s[0], (cols[1] - c[1]) * s[1]
    x, y = (cols[2] - c[2]) * s[2], (cols[3] - c[3]) * s[3]
    one, zero = np.ones(n), np.zeros(n)
    Lx = [X, Y, one, zero, zero, zero, -x * X, -x * Y, -x]
    Ly = [zero, zero, zero, X, Y, one, -y * X, -y * Y, -y]
    return Lx, Ly, (c[0:2], c[2:4], s[0:2], s[2:4])


def dlt_matrix(src, dst):
    """The 9x9 LtL of the pairs, every entry summed over the pairs in index order: (LtL as list of lists, normalisation) or None."""
    got = dlt_rows(src, dst)
    if got is None:
        return None
    Lx, Ly, norm = got
    LtL = [[0.0] * 9 for _ in range(9)]
    for j in range(9):
        for k in range(j, 9):
            v = _seq(Lx[j] * Lx[k] + Ly[j] * Ly[k])
            LtL[j][k] = v
            LtL[k][j] = v
    return LtL, norm


def dlt_from_vector(h0, norm):
    """H = inv(T_dst) H0 T_src from the unit null vector h0 (9) of the normalised system, before the division by H[2, 2]."""
    cM, cm, sM, sm = norm
    inv_dst = [[1.0 / sm[0], 0.0, cm[0]], [0.0, 1.0 / sm[1], cm[1]], [0.0, 0.0, 1.0]]
    t_src = [[sM[0], 0.0, -cM[0] * sM[0]], [0.0, sM[1], -cM[1] * sM[1]], [0.0, 0.0, 1.0]]
    H0 = [[h0[3 * i + j] for j in range(3)] for i in range(3)]
    T = [[(inv_dst[i][0] * H0[0][j] + inv_dst[i][1] * H0[1][j]) + inv_dst[i][2] * H0[2][j] for j in range(3)] for i in range(3)]
    return [[(T[i][0] * t_src[0][j] + T[i][1] * t_src[1][j]) + T[i][2] * t_src[2][j] for j in range(3)] for i in range(3)]


def dlt(src, dst):
    """The DLT stage: (H 3x3 float64 scaled to H[2, 2] == 1, ok)."""
    got = dlt_matrix(src, dst)
    if got is None:
        return np.zeros((3, 3)), 0
    LtL, norm = got
    w, V = jacobi_eigen(LtL, 9)
    kmin, wmax = 0, abs(w[0])
    for k in range(1, 9):
        if w[k] < w[kmin]:
            kmin = k
        if abs(w[k]) > wmax:
            wmax = abs(w[k])
    second = None
    for k in range(9):
        if k != kmin and (second is None or w[k] < second):
            second = w[k]
    if not (second > RANK_RATIO * wmax):
        return np.zeros((3, 3)), 0
    H = dlt_from_vector([V[j][kmin] for j in range(9)], norm)
    if H[2][2] == 0.0 or not all(math.isfinite(v) for r in H for v in r):
        return np.zeros((3, 3)), 0
    inv = 1.0 / H[2][2]
    H = np.array([[v * inv for v in r] for r in H], np.float64)
    if not np.all(np.isfinite(H)):
        return np.zeros((3, 3)), 0
    return H, 1


def _project(h, X, Y, x, y):
    """The per-point quantities of one LM evaluation: (a, b, ww, rx, ry, xi, yi)."""
    Wd = (h[6] * X + h[7] * Y) + 1.0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        ww = np.where(np.abs(Wd) > DBL_EPSILON, 1.0 / Wd, 0.0)
    xi = ((h[0] * X + h[1] * Y) + h[2]) * ww
    yi = ((h[3] * X + h[4] * Y) + h[5]) * ww
    return X * ww, Y * ww, ww, xi - x, yi - y, xi, yi


def _sq_error(h, X, Y, x, y):
    with np.errstate(all="ignore"):
        _, _, _, rx, ry, _, _ = _project(h, X, Y, x, y)
        return _seq(rx * rx + ry * ry)


def refine(H, src, dst, history=None):
    """Levenberg-Marquardt on the 8 free parameters, at most LM_ITERATIONS evaluations; a step is taken only if the squared error falls.
    history (a list) receives the squared error at the start and after every accepted step."""
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    X, Y, x, y = src[:, 0], src[:, 1], dst[:, 0], dst[:, 1]
    n = src.shape[0]
    h = [float(H[i // 3][i % 3]) for i in range(8)]
    lam = 1e-3
    S = _sq_error(h, X, Y, x, y)
    if history is not None:
        history.append(S)
    zero = np.zeros(n)
    for it in range(LM_ITERATIONS):
        if not (S > 0.0):                # exact already (or NaN): nothing to gain
            break
        with np.errstate(all="ignore"):
            a, b, ww, rx, ry, xi, yi = _project(h, X, Y, x, y)
            Jx = [a, b, ww, zero, zero, zero, -a * xi, -b * xi]
            Jy = [zero, zero, zero, a, b, ww, -a * yi, -b * yi]
            A = [[0.0] * 8 for _ in range(8)]
            for j in range(8):
                for k in range(j, 8):
                    v = _seq(Jx[j] * Jx[k] + Jy[j] * Jy[k])
                    A[j][k] = v
                    A[k][j] = v
            g = [_seq(Jx[j] * rx + Jy[j] * ry) for j in range(8)]
        for j in range(8):
            A[j][j] = A[j][j] + lam * A[j][j]
        w, V = jacobi_eigen(A, 8)
        wmax = 0.0
        for k in range(8):
            if abs(w[k]) > wmax:
                wmax = abs(w[k])
        d = [0.0] * 8
        for k in range(8):
            if not (abs(w[k]) > DBL_EPSILON * wmax):
                continue
            dot = 0.0
            for j in range(8):
                dot = dot + V[j][k] * g[j]
            coef = dot / w[k]
            for j in range(8):
                d[j] = d[j] + V[j][k] * coef
        hn = [h[j] - d[j] for j in range(8)]
        Sn = _sq_error(hn, X, Y, x, y)
        if Sn < S:
            h, S = hn, Sn
            lam = lam / 10.0
            if history is not None:
                history.append(S)
        else:
            lam = lam * 10.0
    return np.array([[h[0], h[1], h[2]], [h[3], h[4], h[5]], [h[6], h[7], 1.0]], np.float64)


def find_homography(src, dst, history=None):
    """(H (3, 3) float64, ok): the DLT, then the refinement.  ok == 0 (H all zero) when the pairs do not determine a homography or an
    entry is not finite."""
    H, ok = dlt(src, dst)
    if not ok:
        return H, 0
    H = refine(H, src, dst, history)
    if not np.all(np.isfinite(H)):
        return np.zeros((3, 3)), 0
    return H, 1
