"""tests/affine_ref.py, the numpy restatement of include/mavflow_affine.h, held to the definition -- what a robust affine fit must do,
stated without the restatement's own expressions: recovery of a known map under gross outliers and a moving patch (where the all-pairs
least-squares fit fails), the refinement against np.linalg.lstsq, the properties of need[] and its margin from rounding ties, the
sequential choice, degenerate samples, and the draw of the triples.  Runs without a GPU."""
import math

import numpy as np
import pytest

import affine_cases as T
import affine_ref as R


def _lstsq(src, dst):
    A = np.column_stack([src, np.ones(len(src))])
    return np.linalg.lstsq(A, dst, rcond=None)[0].T


def test_noise_free_recovery_under_outliers_and_a_moving_patch():
    src, dst, good = T.scene(1000, 1, outliers=0.3, patch=True)
    in_patch = (np.abs(src[:, 0] - 320) < 12) & (np.abs(src[:, 1] - 240) < 12)
    assert in_patch.any() and not good[in_patch].any() and 600 < good.sum() < 720      # the patch holds sampled points; 30 % are gross outliers
    out = R.estimate_one(src, dst, T.triples_for(2, 1000, 2000, 1)[0])
    rec = out["record"]
    assert rec["ok"] == 1 and rec["refined"] == 1
    assert np.array_equal(out["inliers"].astype(bool), good)                 # the mask is the true inlier set
    assert rec["inliers"] == np.count_nonzero(good)
    assert np.abs(out["M"] - T.TRUE_M).max() < 1e-9
    assert rec["iters_run"] < 2000 and rec["best_iter"] < rec["iters_run"]  # the early stop left the loop
    assert np.abs(_lstsq(src, dst) - T.TRUE_M).max() > 0.01                  # what RANSAC buys: every pair pulls the plain fit


def test_refined_matrix_is_the_least_squares_fit_of_the_inliers():
    for seed in (3, 4):
        src, dst, good = T.scene(500, seed, outliers=0.25, noise=0.5)
        out = R.estimate_one(src, dst, T.triples_for(seed, 500, 500, 1)[0])
        inl = out["inliers"].astype(bool)
        assert out["record"]["refined"] == 1 and inl.sum() > 300
        want = _lstsq(src[inl], dst[inl])
        assert np.abs(out["M"] - want).max() <= 1e-9 * np.abs(want).max()
        res = src[inl] @ out["M"][:, :2].T + out["M"][:, 2] - dst[inl]
        assert out["record"]["sq_error"] == pytest.approx((res ** 2).sum(), rel=1e-12)
        minimal = R.estimate_one(src, dst, T.triples_for(seed, 500, 500, 1)[0], refine=False)
        assert minimal["record"]["refined"] == 0 and np.array_equal(minimal["inliers"], out["inliers"])     # the mask is the minimal model's
        assert minimal["record"]["sq_error"] > out["record"]["sq_error"]


@pytest.mark.parametrize("n", T.TIE_SIZES)
def test_need_table_properties_and_tie_margin(n):
    for conf in T.CONFIDENCES:
        need = R.need_table(n, conf, 2000)
        assert need.shape == (n + 1,) and need.dtype == np.int32
        assert np.all(np.diff(need) <= 0) and need[n] == 0 and np.all(need[:3] == 2000)
        closest = 1.0
        for g in range(3, n + 1):
            q = R.need_quotient(n, g, conf)
            if q is None:
                assert need[g] == 0
                continue
            ln, ld = q
            # OpenCV's expression, taken independently of the restatement's grouping
            ep = (n - g) / n
            denom = 1.0 - (1.0 - ep) ** 3
            k = math.log(1.0 - conf) / math.log(denom) if 0 < denom < 1 else math.inf
            assert need[g] == (2000 if k >= 2000 else round(k)), (n, g, conf)
            if k < 2000:
                closest = min(closest, abs(k - math.floor(k) - 0.5))
        assert closest > 1e-6, (n, conf, closest)              # no quotient within 1e-6 of a rounding tie: the table does not depend on the log in use


def test_the_sequential_choice():
    need = np.array([9, 9, 9, 9, 6, 4, 2, 0], np.int32)       # n = 7
    # the first of equal counts wins
    assert R.choose(np.array([-1, 4, 4, 4, 3, 4, 2, 1, 0], np.int32), need)[:2] == (1, 6)
    # counts of 2 or fewer never win; an invalid hypothesis never wins
    assert R.choose(np.array([2, 1, -1, 0], np.int32), need) == (-1, 4, 3, 0)
    # a later, larger count beyond the shrunken niters is not seen: 5 at index 1 sets niters = 4, the 7 at index 4 is outside
    best, niters, valid, g = R.choose(np.array([3, 5, -1, 4, 7, 7, 7, 7, 7], np.int32), need)
    assert (best, niters, valid, g) == (1, 4, 3, 5)
    # ... and one inside is: 6 at index 3 sets niters = 2, which ends the loop at once
    assert R.choose(np.array([3, 5, -1, 6, 7, 7, 7, 7, 7], np.int32), need) == (3, 2, 2, 6)
    # the brute-force loop over random tables
    rng = np.random.default_rng(0)
    for _ in range(200):
        n = int(rng.integers(3, 40))
        need = np.sort(rng.integers(0, 70, n + 1))[::-1].astype(np.int32)
        count = rng.integers(-1, n + 1, 64).astype(np.int32)
        niters, best, bc = 64, -1, 2
        for it in range(64):
            if it >= niters:
                break
            if count[it] > bc:
                best, bc, niters = it, count[it], min(niters, need[count[it]])
        assert R.choose(count, need)[:2] == (best, niters)


def test_degenerate_triples_score_zero_and_collinear_data_fails():
    src, dst, _ = T.scene(30, 5, outliers=0)
    src[4] = src[3]                                            # a repeated point
    src[7] = 0.5 * (src[5] + src[6])                           # three points on a line
    dst[7] = 0.5 * (dst[5] + dst[6])
    bad = np.array([[3, 4, 9], [9, 3, 4], [5, 6, 7], [7, 5, 6], [1, 1, 2], [0, 30, 2], [-1, 0, 2]], np.int32)
    assert np.all(R.counts(src, dst, bad, 3.0) == -1)
    assert R.counts(src, dst, np.array([[0, 1, 2]], np.int32), 3.0)[0] >= 26
    for name in ("all_collinear",):
        c = T.BY_NAME[name]
        out = T.reference(name)
        assert out["records"]["ok"][0] == 0 and not out["M"].any() and not out["inliers"].any()
        assert out["records"]["best_iter"][0] == -1 and out["records"]["valid"][0] == 0 and out["records"]["iters_run"][0] == c.triples.shape[1]


def test_the_special_cases_are_what_their_names_say():
    ref = {c.name: T.reference(c.name)["records"] for c in T.CASES if c.src.shape[1] <= 300}
    r = ref["all_inliers"][0]
    assert r["inliers"] == 65 and r["iters_run"] == 0 and r["valid"] == 0 and r["ok"] == 1
    r = ref["equal_counts"][0]
    c = T.reference("equal_counts")
    assert r["inliers"] == 32 and c["inliers"][0, 32:].all() and not c["inliers"][0, :32].any()      # the first of the equal counts: the second half's
    r = ref["on_threshold"][0]
    c = T.reference("on_threshold")
    assert r["inliers"] == 64 and c["inliers"][0, 10] == 1 and c["inliers"][0, 11] == 0
    r = ref["threshold_0"][0]
    assert r["inliers"] == 64 and r["sq_error"] == 0.0 and T.reference("threshold_0")["inliers"][0, 20] == 0
    assert ref["rank_refused"][0]["refined"] == 0 and ref["rank_refused"][0]["inliers"] == 40 and ref["rank_refused"][0]["ok"] == 1
    assert np.all(ref["noisy_refine0"]["refined"] == 0) and np.all(ref["noisy_refine1"]["refined"] == 1)
    assert np.array_equal(ref["noisy_refine0"]["best_iter"], ref["noisy_refine1"]["best_iter"])
    assert np.all(ref["non_finite"]["ok"] == 1) and np.all(np.isfinite(T.reference("non_finite")["M"]))
    assert list(ref["bad_triples"]["ok"]) == [1, 1, 0] and ref["bad_triples"]["valid"][2] == 0
    for n in T.SIZES[:5]:
        assert np.all(ref[f"n{n}_it65_b3"]["ok"] == 1), n


def test_sample_triples(mav):
    from mavflow import affine

    class Counting:
        def __init__(self, seed):
            self.g, self.calls = np.random.default_rng(seed), []

        def random(self, k):
            self.calls.append(k)
            return self.g.random(k)

    for n in (3, 4, 5, 64, 1000):
        rng = Counting(11)
        t = affine.sample_triples(rng, n, 500, 2)
        assert rng.calls == [2 * 500 * 3]                       # one call of the stated length
        assert t.shape == (2, 500, 3) and t.dtype == np.int32 and t.min() >= 0 and t.max() < n
        assert np.all(t[..., 0] != t[..., 1]) and np.all(t[..., 0] != t[..., 2]) and np.all(t[..., 1] != t[..., 2])
        assert np.array_equal(t, T.triples_for(11, n, 500, 2))
        # batch = 2 is the two halves of the seed's own stream
        u = np.random.default_rng(11).random(3000)
        halves = [affine.sample_triples(type("S", (), {"random": staticmethod(lambda k, h=h: u[1500 * h:1500 * (h + 1)])})(), n, 500)[0] for h in (0, 1)]
        assert np.array_equal(t[0], halves[0]) and np.array_equal(t[1], halves[1])
        if n >= 64:
            assert len(np.unique(t)) > n // 3
    with pytest.raises(ValueError):
        affine.sample_triples(0, 2, 5)
    np.random.seed(5)
    a = affine.sample_triples(np.random, 10, 4)
    np.random.seed(5)
    assert np.array_equal(a, affine.sample_triples(np.random.RandomState(5), 10, 4))


# ---- the case table past the score grid's cap (computed from the source's constants and the restatement alone) -----------------------------
def test_the_score_grid_is_capped_where_the_table_says():
    import re
    c = T.source_constants()
    assert re.search(r"const int cap = AFF_GRID_CAP / a\.B < 1 \? 1 : AFF_GRID_CAP / a\.B;\s*hipLaunchKernelGGL\(k_affine_score, dim3\(per < cap \? per : cap, a\.B\)", c["text"])
    assert re.search(r"const int per = \(a\.max_iters \+ AFF_WAVES \* AFF_HYP_PER_WAVE - 1\) / \(AFF_WAVES \* AFF_HYP_PER_WAVE\);", c["text"]) and T.CHUNK == c["AFF_CHUNK"]
    for case in T.CASES:                                       # no case of the table before these is capped
        assert T.score_grid(case.triples.shape[1], case.src.shape[0], c) == "per-item", (case.name, "is capped")
    capped = [case for case in T.CAP_CASES if T.score_grid(case.triples.shape[1], case.src.shape[0], c) == "capped"]
    assert len(capped) == len(T.CAP_CASES) >= 4, ("not every case of CAP_CASES reaches the form: capped", sorted({case.name for case in T.CAP_CASES} - {case.name for case in capped}))
    assert {(case.triples.shape[1], case.src.shape[1]) for case in capped} == {(mi, n) for mi in (2049, 4096) for n in (65, T.CHUNK + 1)}
    assert all(case.src.shape[0] == T.CAP_BATCH == 16 for case in capped) and T.CAP_ITERS == (2049, 4096)
    # the threshold is where the table says: one iteration fewer at the same batch is not capped
    assert T.score_grid(T.CAP_ITERS[0], T.CAP_BATCH, c) == "capped" and T.score_grid(T.CAP_ITERS[0] - 1, T.CAP_BATCH, c) == "per-item", ("CAP_ITERS", T.CAP_ITERS)
    for case in T.CAP_CASES:                                    # different data per item
        assert len({case.src[b].tobytes() for b in range(T.CAP_BATCH)}) == len({case.triples[b].tobytes() for b in range(T.CAP_BATCH)}) == T.CAP_BATCH


def test_the_late_winners_sit_among_the_last_hypotheses():
    """what makes the capped stride's later trips decide the result: the chosen hypothesis is past every workgroup's first trip, and at
    n = CHUNK + 1 its count is one added to across two chunks"""
    c = T.source_constants()
    late = [case for case in T.CAP_CASES if case.name.endswith("_late")]
    assert {case.src.shape[1] for case in late} == {65, T.CHUNK + 1}
    for case in late:
        mi = case.triples.shape[1]
        first_trip = T.score_blocks(mi, T.CAP_BATCH, c)[1] * c["AFF_WAVES"]          # hypotheses of the capped grid's first trip
        rec = T.reference(case.name)["records"]
        assert (rec["ok"] == 1).all() and (rec["best_iter"] >= mi - 6).all() and (rec["best_iter"] >= first_trip).all(), (case.name, rec)
