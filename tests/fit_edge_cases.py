"""Inputs of the homography fit chosen to take the eigen-solver (jacobi_eigen of tests/global_motion_ref.py and of
csrc/kernels_motion.hip) through each of its branches, and a counting twin of the restatement's solver that says which were taken.
Shared by tests/test_fit_edge_cases_cpu.py (the twin equals the restatement; every branch is reached) and
tests/test_gpu_fit_edge_cases.py (the kernel equals the restatement on every entry)."""
import math

import numpy as np

import global_motion_ref as R
from global_motion_cases import H_TRUE, project

BRANCHES = ("skip", "set_zero", "theta_not_finite", "theta_negative", "nan_stop", "n8", "n9")
# Nearly collinear sets (near_rank): the points of a line, every second one moved off it by +-RANK_EPS.  The second smallest eigenvalue
# of LtL falls with the offset; the two offsets were found with the restatement (bisection on second / largest against RANK_RATIO
# = 1e-12, which it crosses at 1.46454e-4) and sit 0.4 % above and below the crossing (0.8 % in the ratio).  test_fit_edge_cases_cpu.py checks the two sides.
RANK_EPS_ABOVE = 1.4704e-4
RANK_EPS_BELOW = 1.4587e-4


def jacobi_eigen_counting(A, n, counts):
    """R.jacobi_eigen with a counter per branch (counts: dict, incremented in place).  Same operations in the same order."""
    counts["n%d" % n] = counts.get("n%d" % n, 0) + 1
    V = [[1.0 if i == j else 0.0 for j in range(n)] for i in range(n)]
    sweep = -1
    for sweep in range(R.JACOBI_SWEEPS):
        off = 0.0
        for p in range(n - 1):
            for q in range(p + 1, n):
                off = off + abs(A[p][q])
        if not (off > 0.0):
            if off != off:
                counts["nan_stop"] = counts.get("nan_stop", 0) + 1
            break
        for p in range(n - 1):
            for q in range(p + 1, n):
                apq = A[p][q]
                if apq == 0.0:
                    counts["skip"] = counts.get("skip", 0) + 1
                    continue
                g = 100.0 * abs(apq)
                app, aqq = A[p][p], A[q][q]
                if sweep > 3 and abs(app) + g == abs(app) and abs(aqq) + g == abs(aqq):
                    counts["set_zero"] = counts.get("set_zero", 0) + 1
                    A[p][q] = 0.0
                    A[q][p] = 0.0
                    continue
                theta = (aqq - app) / (2.0 * apq)
                if math.isfinite(theta):
                    t = 1.0 / (abs(theta) + math.sqrt(theta * theta + 1.0))
                else:
                    counts["theta_not_finite"] = counts.get("theta_not_finite", 0) + 1
                    t = 0.0
                if theta < 0.0:
                    counts["theta_negative"] = counts.get("theta_negative", 0) + 1
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
    else:
        counts["sweep_cap"] = counts.get("sweep_cap", 0) + 1          # all JACOBI_SWEEPS sweeps ran (no input of the table does it)
    counts["max_sweeps"] = max(counts.get("max_sweeps", 0), sweep + 1)
    return [A[i][i] for i in range(n)], V


def near_rank(eps, n=12):
    """(src, dst): points of the line y = 0.5 x + 7, every second one moved off it by +-eps; dst = src moved by (1.5, -0.75)."""
    t = np.arange(float(n)) * 13.0 + 5.0
    src = np.c_[t, 0.5 * t + 7.0]
    src[1::2, 1] += eps * np.where(np.arange(n // 2) % 2 == 0, 1.0, -1.0)
    return src, src + np.array([1.5, -0.75])


def rank_ratio(src, dst):
    """second smallest / largest eigenvalue of the pairs' LtL, as R.dlt takes them."""
    LtL, _ = R.dlt_matrix(src, dst)
    w, _ = R.jacobi_eigen(LtL, 9)
    w = sorted(w)
    return w[1] / max(abs(v) for v in w)


def table():
    """[(name, src (n, 2), dst (n, 2))], float64."""
    rng = np.random.default_rng(23)
    out = []
    # a grid symmetric about its centroid, moved by an exact translation: entries of LtL are exactly zero (the apq == 0 skip)
    gx, gy = np.meshgrid(np.arange(-3.0, 4.0) * 16.0 + 100.0, np.arange(-2.0, 3.0) * 16.0 + 80.0)
    grid = np.c_[gx.ravel(), gy.ravel()]
    out.append(("symmetric_grid_translation", grid, grid + np.array([4.0, -2.0])))
    # exact correspondences at n = 4 of a known H (a translation of a small square): the DLT returns it exactly, the squared error is 0
    # and the refinement ends before its first evaluation (found with the restatement; the CPU test checks that it does)
    sq = np.array([[63.0, 63.0], [65.0, 63.0], [65.0, 65.0], [63.0, 65.0]])
    out.append(("exact4_zero_error", sq, sq + np.array([4.0, -2.0])))
    src4 = np.array([[32.0, 48.0], [608.0, 32.0], [576.0, 400.0], [16.0, 416.0]])
    out.append(("exact4", src4, project(H_TRUE, src4)))
    for n in (5, 7, 17, 257, 1000):
        src = rng.integers(20, 620, (n, 2)).astype(np.float64)
        out.append((f"noisy{n}", src, project(H_TRUE, src) + rng.normal(0, 0.7, (n, 2)).astype(np.float32)))
    src = rng.integers(20, 620, (64, 2)).astype(np.float64) + 1e6
    out.append(("offset_1e6", src, src + rng.normal(0, 2, (64, 2)).astype(np.float32)))
    out.append(("rank_above", *near_rank(RANK_EPS_ABOVE)))
    out.append(("rank_below", *near_rank(RANK_EPS_BELOW)))
    for name, bad in (("one_nan", np.nan), ("one_inf", np.inf)):
        src = rng.integers(20, 620, (17, 2)).astype(np.float64)
        dst = project(H_TRUE, src)
        dst[5, 1] = bad
        out.append((name, src, dst))
    # sources near 1e153, ordinary destinations: finite, the normalised system is an ordinary one and the DLT succeeds, but squares of
    # the refinement's Jacobian overflow -- its 8x8 matrix holds +-inf and no NaN, theta is (inf - inf) / inf (t = 0), the rotation
    # leaves NaN and the next sweep's off-diagonal sum stops the solver; no step is accepted and ok stays 1
    src = rng.integers(20, 620, (17, 2)).astype(np.float64)
    out.append(("huge_src_1e153", src * 1e153, src + rng.normal(0, 2, (17, 2))))
    # both near 1e155: the 8x8 matrix holds NaN from the start (inf * 0), the solver stops before its first rotation
    out.append(("huge_both_1e155", src * 1e155, (src + rng.normal(0, 2, (17, 2))) * 1e155))
    return out


def find_homography_counting(src, dst, counts):
    """R.find_homography with the counting solver in place of R.jacobi_eigen: (H, ok).  Every matrix the solver receives is first solved
    by R.jacobi_eigen on a copy; the two results must be the same bytes (AssertionError otherwise)."""
    keep = R.jacobi_eigen

    def both(A, n):
        copy = [list(r) for r in A]
        w0, V0 = keep(copy, n)
        w1, V1 = jacobi_eigen_counting(A, n, counts)
        same = np.array(w0).tobytes() == np.array(w1).tobytes() and np.array(V0).tobytes() == np.array(V1).tobytes() and \
            np.array(copy).tobytes() == np.array(A).tobytes()
        assert same, "the counting twin left other bytes than R.jacobi_eigen"
        counts["matrices"] = counts.get("matrices", 0) + 1
        return w1, V1
    R.jacobi_eigen = both
    try:
        return R.find_homography(src, dst)
    finally:
        R.jacobi_eigen = keep
