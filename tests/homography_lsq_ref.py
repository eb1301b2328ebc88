"""TEST INFRASTRUCTURE -- an independent float64 minimiser of the summed squared reprojection error

    cost(H) = sum_i |project(H, src_i) - dst_i|^2,

which is what cv2.findHomography(src, dst, 0) is defined to return the minimiser of.  tests/test_homography_lsq_cpu.py holds the
Levenberg-Marquardt refinement of tests/global_motion_ref.py (and, through byte equality, of csrc/kernels_motion.hip) to it.

Written from the definition; it shares nothing with global_motion_ref.py beyond global_motion_cases.project, and differs from it in
every choice a solver has:

* coordinates: Hartley-normalised (centroid at the origin, mean distance sqrt 2, ONE scale per point set -- an isotropic scale of the
  destinations multiplies every residual by the same number, so the minimiser is the same), de-normalised at the end;
* start: the null vector of the stacked DLT rows by np.linalg.svd;
* step: Gauss-Newton on the 8 free parameters (H[2, 2] == 1 in normalised coordinates) with the analytic Jacobian, the step solved by
  np.linalg.lstsq on J itself (no normal equations, no damping, no Jacobi), halved until the cost falls;
* stop: stationarity, max_j |J^T r|_j / (|J_j| |r|) <= STATIONARY, or no halving of the step lowers the cost any more.

numpy only."""
import numpy as np

from global_motion_cases import project

STATIONARY = 1e-12
MAX_STEPS = 200
MAX_HALVINGS = 60


def hartley(p):
    """3x3 T with T p~ centred and at mean distance sqrt 2."""
    c = p.mean(axis=0)
    d = np.sqrt(((p - c) ** 2).sum(axis=1)).mean()
    s = np.sqrt(2.0) / d
    return np.array([[s, 0.0, -s * c[0]], [0.0, s, -s * c[1]], [0.0, 0.0, 1.0]])


def _apply(T, p):
    return p * T[0, 0] + T[:2, 2]


def _residual_and_jacobian(h, X, Y, x, y):
    """r (2n) and J (2n, 8) of the 8 parameters h; rows: every x residual, then every y residual."""
    w = h[6] * X + h[7] * Y + 1.0
    u = (h[0] * X + h[1] * Y + h[2]) / w
    v = (h[3] * X + h[4] * Y + h[5]) / w
    n = len(X)
    J = np.zeros((2 * n, 8))
    J[:n, 0], J[:n, 1], J[:n, 2] = X / w, Y / w, 1.0 / w
    J[:n, 6], J[:n, 7] = -u * X / w, -u * Y / w
    J[n:, 3], J[n:, 4], J[n:, 5] = X / w, Y / w, 1.0 / w
    J[n:, 6], J[n:, 7] = -v * X / w, -v * Y / w
    return np.concatenate([u - x, v - y]), J


def stationarity(J, r):
    """max_j |J^T r|_j / (|J_j| |r|): the cosine of the angle between the residual and the Jacobian's column most aligned with it."""
    rn = np.linalg.norm(r)
    if rn == 0.0:
        return 0.0
    return float(np.max(np.abs(J.T @ r) / (np.linalg.norm(J, axis=0) * rn)))


def cost(H, src, dst):
    """The definition, in the caller's own coordinates."""
    return float(np.sum((project(np.asarray(H, np.float64), src) - dst) ** 2))


def minimise(src, dst):
    """-> dict(H (3, 3) scaled to H[2, 2] == 1, cost (in the caller's coordinates), stationarity, steps)."""
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    Ts, Td = hartley(src), hartley(dst)
    P, Q = _apply(Ts, src), _apply(Td, dst)
    X, Y, x, y = P[:, 0], P[:, 1], Q[:, 0], Q[:, 1]
    one, zero = np.ones_like(X), np.zeros_like(X)
    L = np.concatenate([np.stack([X, Y, one, zero, zero, zero, -x * X, -x * Y, -x], axis=1),
                        np.stack([zero, zero, zero, X, Y, one, -y * X, -y * Y, -y], axis=1)])
    h9 = np.linalg.svd(L)[2][-1]
    h = h9[:8] / h9[8]
    r, J = _residual_and_jacobian(h, X, Y, x, y)
    S = float(r @ r)
    steps = 0
    for steps in range(1, MAX_STEPS + 1):
        if stationarity(J, r) <= STATIONARY:
            break
        d = np.linalg.lstsq(J, -r, rcond=None)[0]
        t, moved = 1.0, False
        for _ in range(MAX_HALVINGS):
            rn, Jn = _residual_and_jacobian(h + t * d, X, Y, x, y)
            Sn = float(rn @ rn)
            if Sn < S:
                h, r, J, S, moved = h + t * d, rn, Jn, Sn, True
                break
            t *= 0.5
        if not moved:
            break
    Hn = np.array([[h[0], h[1], h[2]], [h[3], h[4], h[5]], [h[6], h[7], 1.0]])
    H = np.linalg.inv(Td) @ Hn @ Ts
    H = H / H[2, 2]
    return dict(H=H, cost=cost(H, src, dst), stationarity=stationarity(J, r), steps=steps)
