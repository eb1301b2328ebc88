"""Point-pair cases of the homography fit, shared by the CPU and GPU tests of the global-motion branch."""
import numpy as np

H_TRUE = np.array([[1.01, 0.02, 3.0], [-0.015, 0.99, -2.0], [1e-5, -2e-5, 1.0]])


def project(H, src):
    p = np.c_[src, np.ones(len(src))] @ H.T
    return p[:, :2] / p[:, 2:]


def fit_cases():
    """(name, src, dst, exact): n = 4, 5, 1000, 2666 exact correspondences of H_TRUE, noisy ones, pairs far from the origin (the
    normalisation matters) and flow-like pairs (dst = src + a float32 vector, what the gather produces)."""
    rng = np.random.default_rng(7)
    out = []
    for n in (4, 5, 1000, 2666):
        src = rng.integers(20, 620, (n, 2)).astype(np.float64)
        if n == 4:
            src = np.array([[30.0, 40.0], [600.0, 35.0], [580.0, 400.0], [25.0, 420.0]])
        out.append((f"exact{n}", src, project(H_TRUE, src), True))
    src = rng.integers(20, 620, (1000, 2)).astype(np.float64)
    out.append(("noisy1000", src, project(H_TRUE, src) + rng.normal(0, 0.7, (1000, 2)).astype(np.float32), False))
    src = rng.integers(1200, 1900, (1000, 2)).astype(np.float64)
    out.append(("exact1000_far", src, project(H_TRUE, src), True))
    src = rng.integers(20, 300, (64, 2)).astype(np.float64)
    out.append(("flowlike64", src, src + rng.normal(0, 2, (64, 2)).astype(np.float32), False))
    return out


def degenerate_pairs(kind, n=12):
    """(src, dst) that determine no homography: collinear points, one repeated point, destinations without spread on one axis."""
    t = np.arange(float(n))
    if kind == "collinear":
        src = np.c_[3 * t + 1, 2 * t + 5]
        return src, src + 1.5
    if kind == "repeated":
        src = np.ones((n, 2)) * 7.0
        return src, src.copy()
    src = np.c_[t * 5 % 37, t * 11 % 41]
    return src, np.c_[np.full(n, 3.0), t]
