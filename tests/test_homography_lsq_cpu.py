"""The Levenberg-Marquardt refinement of the homography fit (tests/global_motion_ref.py; csrc/kernels_motion.hip equals it byte for
byte, tests/test_gpu_global_motion.py / test_gpu_fit_edge_cases.py / test_gpu_motion_forms.py) held to what it is for: with method 0,
findHomography returns the minimiser of the summed squared reprojection error, and tests/homography_lsq_ref.py finds that minimiser
independently (Gauss-Newton in Hartley-normalised coordinates, lstsq on the Jacobian).  No GPU.

The condition: the refinement closes at least 99.9 % of the gap the DLT leaves to the optimum,

    cost_fit - cost_opt <= GAP_CLOSED * (cost_dlt - cost_opt),   GAP_CLOSED = 1e-3.

It is a condition, not a measurement: a refinement whose step has the wrong sign, or whose damping rejects every step, stays at the
DLT's cost and misses it by a factor of 1000.  Measured (this file prints the table; profiles/global_motion/README.md keeps a copy):
the left-hand side is <= 0 in eight of nine cases while the DLT's excess is 8.6e-6 to 2.5e-2 of the cost.

The ninth, offset_1e6 (coordinates near 1e6), is a finding and is asserted as one: see test_offset_1e6_is_beyond_the_normal_equations.
"""
import functools

import numpy as np
import pytest

import fit_edge_cases as fe
import global_motion_ref as R
import homography_lsq_ref as L
import motion_cases as mc
from global_motion_cases import fit_cases

GAP_CLOSED = 1e-3
EPS = float(np.finfo(np.float64).eps)
# A step along the Jacobian's column j lowers the cost by (cosine_j)^2 |r|^2.  Below sqrt(eps) that is less than one rounding of the
# cost itself, so "no halving of the step lowers the cost" -- the reference's other way to stop -- cannot leave more than this.
STATIONARY_BOUND = float(np.sqrt(EPS))
# Entries of fit_edge_cases.table() whose destinations are an exact map of the sources (no noise was added): the optimum is zero up to
# rounding and there is no gap to close.  test_exact_entries_are_exact checks each of them against that description.
EXACT = ("symmetric_grid_translation", "exact4_zero_error", "exact4", "rank_above", "rank_below")
NINTH = "offset_1e6"


def all_cases():
    """(name, src, dst): every non-exact case of fit_cases() and of fit_edge_cases.table() with finite inputs below 1e100, and the
    frame-like set."""
    out = [("fit_cases:" + n, s, d) for n, s, d, exact in fit_cases() if not exact]
    for n, s, d in fe.table():
        if n in EXACT or not (np.isfinite(s).all() and np.isfinite(d).all()) or max(np.abs(s).max(), np.abs(d).max()) >= 1e100:
            continue
        out.append((n, s, d))
    out.append(("frame_like", *mc.frame_like_pairs()))
    return out


CASES = all_cases()
NAMES = [c[0] for c in CASES]


@functools.lru_cache(maxsize=None)
def solved(name):
    _, src, dst = CASES[NAMES.index(name)]
    Hd, okd = R.dlt(src, dst)
    Hf, okf = R.find_homography(src, dst)
    assert okd == okf == 1, name
    opt = L.minimise(src, dst)
    return dict(dlt=L.cost(Hd, src, dst), fit=L.cost(Hf, src, dst), opt=opt["cost"], stationarity=opt["stationarity"], steps=opt["steps"],
                Hd=Hd, n=len(src))


def test_the_cases_are_the_nine():
    assert NAMES == ["fit_cases:noisy1000", "fit_cases:flowlike64", "noisy5", "noisy7", "noisy17", "noisy257", "noisy1000", NINTH, "frame_like"]


def test_exact_entries_are_exact():
    """What EXACT leaves out has no noise: where the fit succeeds its error is below a millionth of a pixel per pair."""
    table = {n: (s, d) for n, s, d in fe.table()}
    assert set(EXACT) <= set(table)
    for n in EXACT:
        s, d = table[n]
        H, ok = R.find_homography(s, d)
        if ok:
            assert L.cost(H, s, d) <= len(s) * 1e-12, (n, L.cost(H, s, d))


@pytest.mark.parametrize("name", NAMES)
def test_reference_is_stationary_and_does_not_lose_to_the_dlt(name):
    r = solved(name)
    print(f"{name}: reference stationarity {r['stationarity']:.1e} after {r['steps']} steps (bound {STATIONARY_BOUND:.1e})")
    assert r["stationarity"] <= STATIONARY_BOUND, r
    assert r["opt"] <= r["dlt"], r                           # a minimiser that loses to its own kind of start is none


@pytest.mark.parametrize("name", [n for n in NAMES if n != NINTH])
def test_refinement_closes_the_gap_the_dlt_leaves(name):
    r = solved(name)
    gap_dlt, gap_fit = r["dlt"] - r["opt"], r["fit"] - r["opt"]
    print(f"{name}: n = {r['n']}, cost dlt {r['dlt']:.9e} fit {r['fit']:.9e} opt {r['opt']:.9e}; (dlt - opt) / opt = {gap_dlt / r['opt']:+.2e}, "
          f"(fit - opt) / opt = {gap_fit / r['opt']:+.2e}, closed {1 - gap_fit / gap_dlt:.6f}")
    assert gap_dlt > 0, r
    assert gap_fit <= GAP_CLOSED * gap_dlt, (name, gap_fit / gap_dlt)


def _jacobian_unnormalised(H, src):
    """The refinement's Jacobian at H in the caller's coordinates (2n, 8), as R.refine forms it."""
    X, Y = src[:, 0], src[:, 1]
    w = 1.0 / (H[2, 0] * X + H[2, 1] * Y + 1.0)
    xi, yi = (H[0, 0] * X + H[0, 1] * Y + H[0, 2]) * w, (H[1, 0] * X + H[1, 1] * Y + H[1, 2]) * w
    z = np.zeros_like(X)
    return np.concatenate([np.stack([X * w, Y * w, w, z, z, z, -X * w * xi, -Y * w * xi], axis=1),
                           np.stack([z, z, z, X * w, Y * w, w, -X * w * yi, -Y * w * yi], axis=1)])


def test_offset_1e6_is_beyond_the_normal_equations():
    """offset_1e6 misses the condition by construction: the refinement closes none of the DLT's gap.  Finding: this is inherent to
    refining through the normal equations in un-normalised coordinates -- which is what OpenCV, as recalled, does too -- and no defect
    of the restated damped solve.  At 1e6 offsets the Jacobian's condition number exceeds 1 / eps (5.7e18 measured), so J^T J
    (condition ~ 3e37) holds nothing of the directions along which the cost can still fall: its float64 eigenvalues include a negative
    one, LAPACK's solve of the same damped system gains no more than the restated Jacobi solve with its DBL_EPSILON cut does (4e-9 of
    the cost per step either way), and even lstsq on J itself recovers the gap only in part.  Every other case sits below
    1 / sqrt(eps), where J^T J still carries J.  So the case asserts the weaker, exact statements: the fit does not lose to the DLT, and
    the reference -- in normalised coordinates -- gains the measured relative amount over it.  DESIGN.md section 4d, item 6."""
    r = solved(NINTH)
    gain = (r["dlt"] - r["opt"]) / r["opt"]
    print(f"{NINTH}: cost dlt {r['dlt']:.9e} fit {r['fit']:.9e} opt {r['opt']:.9e}; (dlt - opt) / opt = {gain:+.3e}, "
          f"(fit - opt) / opt = {(r['fit'] - r['opt']) / r['opt']:+.3e}")
    assert r["fit"] <= r["dlt"]
    assert gain >= 6.0e-5, gain                               # measured: 6.03e-5
    conds = {}
    for name, s, _ in CASES:
        conds[name] = float(np.linalg.cond(_jacobian_unnormalised(solved(name)["Hd"], s)))
        print(f"{name}: cond(J) at the DLT's H, un-normalised = {conds[name]:.2e}")
    assert conds[NINTH] > 1.0 / EPS
    assert all(v < 1.0 / np.sqrt(EPS) for k, v in conds.items() if k != NINTH), conds
