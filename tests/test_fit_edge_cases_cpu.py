"""The table of tests/fit_edge_cases.py against the restatement tests/global_motion_ref.py, on the host: the counting twin of the
eigen-solver leaves the restatement's bytes on every matrix the table produces, and over the table every branch of the solver is
taken at least once.  (What the kernel does with the same table: tests/test_gpu_fit_edge_cases.py.)"""
import warnings

import numpy as np
import pytest

import fit_edge_cases as F
import global_motion_ref as R


@pytest.fixture(scope="module")
def runs():
    """{name: (H, ok, counts)} of the table through the counting solver (which asserts equal bytes with R.jacobi_eigen per matrix)."""
    out = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for name, src, dst in F.table():
            counts = {}
            H, ok = F.find_homography_counting(src, dst, counts)
            out[name] = (H, ok, counts)
    return out


def test_counting_twin_changes_no_result(runs):
    assert R.jacobi_eigen.__module__ == "global_motion_ref"              # the restatement's own solver is back in place
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for name, src, dst in F.table():
            H, ok = R.find_homography(src, dst)
            assert ok == runs[name][1] and H.tobytes() == runs[name][0].tobytes(), name


def test_every_branch_of_the_solver_is_reached(runs):
    total = {}
    for _, _, counts in runs.values():
        for k, v in counts.items():
            total[k] = total.get(k, 0) + v
    for branch in F.BRANCHES:
        assert total.get(branch, 0) >= 1, (branch, total)
    assert total["matrices"] == total["n8"] + total["n9"] > 100
    # The 30-sweep cap: no input found takes the solver there (cyclic Jacobi converges quadratically; the table's slowest matrix needs
    # 10 sweeps, and a matrix that does not converge holds NaN and stops at once), so no entry pretends to.
    assert "sweep_cap" not in total and total["max_sweeps"] >= 8, total


def test_entries_are_what_their_names_say(runs):
    table = {name: (src, dst) for name, src, dst in F.table()}
    assert {len(table[f"noisy{n}"][0]) for n in (5, 7, 17, 257, 1000)} == {5, 7, 17, 257, 1000}
    # the symmetric grid: exact zeros in LtL before the first rotation
    LtL, _ = R.dlt_matrix(*table["symmetric_grid_translation"])
    assert sum(1 for p in range(9) for q in range(p + 1, 9) if LtL[p][q] == 0.0) >= 10
    # n = 4, exact: squared error 0 at the DLT's H, no refinement step, the known translation comes back
    H, ok, counts = runs["exact4_zero_error"]
    hist = []
    R.find_homography(*table["exact4_zero_error"], history=hist)
    assert ok == 1 and hist == [0.0] and counts["matrices"] == counts["n9"] == 1
    assert np.array_equal(np.around(H, 9), [[1.0, 0.0, 4.0], [0.0, 1.0, -2.0], [0.0, 0.0, 1.0]])          # (what was put in)
    assert runs["exact4"][1] == 1 and len(table["exact4"][0]) == 4
    assert runs["offset_1e6"][1] == 1 and table["offset_1e6"][0].min() > 1e6
    # either side of the rank threshold, closely
    above, below = F.rank_ratio(*table["rank_above"]), F.rank_ratio(*table["rank_below"])
    assert R.RANK_RATIO < above < 1.02 * R.RANK_RATIO and 0.98 * R.RANK_RATIO < below < R.RANK_RATIO, (above, below)
    assert runs["rank_above"][1] == 1 and runs["rank_below"][1] == 0 and not runs["rank_below"][0].any()
    # not finite: refused before the solver runs
    for name in ("one_nan", "one_inf"):
        src, dst = table[name]
        assert np.sum(~np.isfinite(np.r_[src.ravel(), dst.ravel()])) == 1
        assert runs[name][1] == 0 and not runs[name][0].any() and "matrices" not in runs[name][2]
    # finite but overflowing inside the refinement: the solver meets inf and NaN, ok stays 1 with the DLT's H
    assert runs["huge_src_1e153"][2]["theta_not_finite"] >= 1 and runs["huge_src_1e153"][2]["nan_stop"] >= 1
    assert runs["huge_src_1e153"][1] == 1 and np.isfinite(runs["huge_src_1e153"][0]).all()
    assert runs["huge_both_1e155"][2]["nan_stop"] >= 1
