"""tests/fundamental_ref.py (include/mavflow_fundamental.h in numpy) held to the definition, without a GPU: every valid minimal model
fits its own seven pairs to rounding, a noise-free scene gives the true K^-T [t]x R K^-1, gross outliers are left out and no true inlier
is, need[] is monotone and away from rounding ties, the sequential choice equals a brute loop, the draw of the subsets equals its
restatement, and the dense pass marks a patch that moves on its own and nothing else.

Measured with this restatement over the case table (profiles/fundamental/README.md): the largest err of a valid model at its own seven
pairs is 3.4e-18 px^2 (pure rounding in pixel coordinates up to 640: bounded here by 1000 x that, 3.4e-15); the largest distance of the
fitted F from the true one over the noise-free scenes below is 1.7e-13 (at n = 8; 2.8e-16 .. 5.0e-14 elsewhere; bounded by 100 x
that, 1.7e-11)."""
import re

import numpy as np
import pytest

import fundamental_cases as T
import fundamental_ref as R

MINIMAL_ERR_SEEN, F_DIST_SEEN = 3.4e-18, 1.7e-13
MINIMAL_ERR_BOUND, F_DIST_BOUND = 1000 * MINIMAL_ERR_SEEN, 100 * F_DIST_SEEN
CLEAN = [(n, seed) for n in (8, 63, 64, 65, 257, 1000, 1025) for seed in (1, 2)]


def _f_dist(f, ft):
    return min(np.abs(f - ft).max(), np.abs(f + ft).max())


def test_minimal_models_fit_their_own_pairs():
    worst, roots = 0.0, {0: 0, 1: 0, 2: 0, 3: 0}
    for c in T.CASES:
        if c.dev_only or c.name == "no_valid":
            continue
        for b in range(c.src.shape[0]):
            for sub in c.subsets[b][:40]:
                m3 = R.models(c.src[b], c.dst[b], sub)
                roots[sum(m is not None for m in m3)] += 1
                for f in m3:
                    if f is None:
                        continue
                    assert abs(np.sqrt((f * f).sum()) - 1.0) < 1e-15 and f[np.argmax(np.abs(f))] > 0
                    worst = max(worst, float(R.pair_errors(f, c.src[b][sub], c.dst[b][sub]).max()))
    print("largest err of a minimal model at its own pairs:", worst, "slots per hypothesis:", roots)
    assert worst <= MINIMAL_ERR_BOUND
    assert roots[1] > 0 and roots[3] > 0                      # cubics with one real root and with three are both in the table


@pytest.mark.parametrize("n,seed", CLEAN)
def test_noise_free_scene_gives_the_true_matrix(n, seed):
    src, dst, good, Ft = T.scene(n, seed, outliers=0)
    # threshold 0.01 px: the data are exact to rounding, and at the default 3 px a spurious root of the cubic can hold all of n = 8 pairs
    # (its eighth pair within 3 px of its line), which is a correct answer to another question
    out = R.find_one(src, dst, T.subsets_for(seed, n, 30, 1)[0], threshold=0.01)
    rec = out["record"]
    assert rec["ok"] == 1 and rec["inliers"] == n and out["inliers"].all() and rec["iters_run"] == rec["best_iter"] + 1
    d = _f_dist(out["F"], Ft)
    print("n", n, "seed", seed, "distance from the true F:", d)
    assert d <= F_DIST_BOUND
    assert abs(np.linalg.det(out["F"])) < 1e-12 and abs(np.sqrt((out["F"] ** 2).sum()) - 1) < 1e-15


@pytest.mark.parametrize("n,seed", [(65, 3), (257, 1), (1000, 2), (1025, 1)])
def test_gross_outliers_are_left_out_and_no_inlier_is(n, seed):
    src, dst, good, Ft = T.scene(n, seed, outliers=0.3)
    out = R.find_one(src, dst, T.subsets_for(seed, n, 200, 1)[0])
    inl = out["inliers"].astype(bool)
    extra = int(np.count_nonzero(inl & ~good))
    print("n", n, "seed", seed, "extra pairs in the mask:", extra, "record", out["record"])
    assert out["record"]["ok"] == 1 and inl[good].all()        # every true inlier is in the mask
    assert extra <= max(2, n // 100)                           # an outlier within 3 px of its epipolar line is an inlier by definition
    if extra == 0:
        assert _f_dist(out["F"], Ft) <= F_DIST_BOUND


def test_seven_pairs_fit_exactly():
    src, dst, _, _ = T.scene(7, 4, outliers=0)
    out = R.find_one(src, dst, T.subsets_for(4, 7, 5, 1)[0])
    assert out["record"]["ok"] == 1 and out["record"]["inliers"] == 7 and out["record"]["best_iter"] == 0
    assert R.pair_errors(out["F"], src, dst).max() <= MINIMAL_ERR_BOUND


@pytest.mark.parametrize("n", T.TIE_SIZES)
@pytest.mark.parametrize("confidence", T.CONFIDENCES)
def test_need_table_is_monotone_and_away_from_ties(n, confidence):
    for max_iters in (65, 1000):
        need = R.need_table(n, confidence, max_iters)
        assert np.all(need[:7] == max_iters) and need[n] == 0 and np.all(np.diff(need[6:].astype(np.int64)) <= 0)
        for g in range(7, n + 1):
            q = R.need_quotient(n, g, confidence)
            if q is None:
                continue
            ln, ld = q
            if ld >= 0.0 or -ln >= max_iters * (-ld):
                continue
            frac = (ln / ld) % 1.0
            assert abs(frac - 0.5) > 1e-6, (n, g, confidence, ln / ld)


def test_choice_equals_a_brute_loop():
    rng = np.random.default_rng(11)
    for trial in range(300):
        n = int(rng.integers(7, 80))
        mi = int(rng.integers(1, 70))
        count = rng.integers(-1, n + 1, (mi, 3)).astype(np.int32)
        count[rng.random((mi, 3)) < 0.3] = -1
        need = R.need_table(n, float(rng.choice(T.CONFIDENCES)), mi)
        # the brute loop: a flat list of visits
        niters, best, bc, ran, valid = mi, (-1, -1), 6, 0, 0
        for it in range(mi):
            if not it < niters:
                break
            ran += 1
            for s in range(3):
                valid += count[it, s] >= 0
                if count[it, s] >= 0 and count[it, s] > bc:
                    best, bc = (it, s), int(count[it, s])
                    niters = min(niters, int(need[bc]))
        assert R.choose(count, need) == (best[0], best[1], ran, valid, bc if best[0] >= 0 else 0)
    # all-inlier data: need[n] = 0 stops the loop after the first iteration, whose later slots are still visited
    count = np.array([[10, 20, 20], [20, 20, 20]], np.int32)
    assert R.choose(count, R.need_table(20, 0.99, 2)) == (0, 1, 1, 3, 20)


def test_special_cases_are_what_they_are_named_for():
    ref = {name: T.reference(name)["records"] for name in ("all_inliers", "no_valid", "equal_counts", "beside_threshold", "threshold_0", "bad_subsets")}
    r = ref["all_inliers"][0]
    assert (r["ok"], r["inliers"], r["best_iter"], r["iters_run"]) == (1, 65, 0, 1)
    r = ref["no_valid"][0]
    assert (r["ok"], r["valid"], r["iters_run"], r["best_iter"], r["best_slot"]) == (0, 0, 65, -1, -1)
    r = ref["equal_counts"][0]
    assert r["ok"] == 1 and r["best_iter"] % 2 == 0            # of a repeated pair of hypotheses the first wins
    c = T.BY_NAME["beside_threshold"]
    inl = T.reference("beside_threshold")["inliers"][0]
    assert inl[10] == 1 and inl[11] == 0 and inl.sum() == 64
    assert ref["threshold_0"][0]["valid"] > 0
    assert ref["bad_subsets"][2]["ok"] == 0 and ref["bad_subsets"][2]["valid"] == 0 and ref["bad_subsets"][0]["ok"] == 1
    assert R.models(c.src[0], c.dst[0], [0, 1, 2, 3, 4, 5, 65]) == [None] * 3 and R.models(c.src[0], c.dst[0], [0, 1, 2, 3, 4, 5, 0]) == [None] * 3


@pytest.mark.parametrize("n", (7, 8, 65, 1000))
def test_sample_subsets_equals_its_restatement(mav, n):
    from mavflow import fundamental as K
    got = K.sample_subsets(3, n, 50, 2)
    assert got.dtype == np.int32 and got.shape == (2, 50, 7) and np.array_equal(got, T.subsets_for(3, n, 50, 2))
    assert got.min() >= 0 and got.max() < n and all(len(set(s)) == 7 for s in got.reshape(-1, 7).tolist())
    if n == 7:
        assert np.array_equal(np.sort(got, -1), np.broadcast_to(np.arange(7), got.shape))       # every subset is a permutation of all pairs
    g = np.random.default_rng(3)
    assert np.array_equal(K.sample_subsets(g, n, 50, 2), got)                                  # a Generator: ONE call of .random
    assert g.random() == np.random.default_rng(3).random(2 * 50 * 7 + 1)[-1]
    with pytest.raises(ValueError):
        K.sample_subsets(3, 6, 5)


@pytest.mark.parametrize("frame", T.FLOW_FRAMES)
def test_dense_pass_marks_the_patch_and_nothing_else(frame):
    w, h = frame
    flow, coords, sub = T.flow_case(w, h, 3)
    _, at = T.dense_scene(w, h, 3)
    src, dst = R.flow_pairs(flow, coords)
    fit = R.find(src, dst, sub, threshold=0.5)
    assert np.all(fit["records"]["ok"] == 1)
    epi = R.epipolar_residual(flow, fit["F"], 1.0)
    patch = np.zeros((h, w), np.uint8)
    patch[at[0]:at[0] + T.PATCH, at[1]:at[1] + T.PATCH] = 255
    for b in range(3):
        assert np.array_equal(epi["mask"][b], patch), (frame, b)
        r = epi["records"][b]
        assert r["movers"] == 64 and r["not_finite"] == 0 and patch[r["max_row"], r["max_col"]] == 255
        assert r["max_residual"] == epi["residual"][b].max() and epi["residual"][b][r["max_row"], r["max_col"]] == r["max_residual"]
    zero = R.epipolar_residual(flow, np.zeros((3, 3, 3)), 1.0)                                  # a failed fit's F
    assert not zero["residual"].any() and not zero["mask"].any() and np.all(zero["records"]["not_finite"] == w * h)
    assert np.all(zero["records"]["max_row"] == -1)


# ---- the case table past the caps (computed from the source's constants and the restatement alone) ------------------------------------------
def test_the_score_grid_is_capped_where_the_table_says():
    c = T.source_constants()
    assert re.search(r"const int cap = FM_GRID_CAP / a\.B < 1 \? 1 : FM_GRID_CAP / a\.B;\s*hipLaunchKernelGGL\(k_fm_score, dim3\(per < cap \? per : cap, a\.B\)", c["text"])
    assert re.search(r"const int per = \(slots \+ FM_WAVES \* FM_SLOTS_PER_WAVE - 1\) / \(FM_WAVES \* FM_SLOTS_PER_WAVE\);", c["text"]) and T.CHUNK == c["FM_CHUNK"]
    for case in T.CASES:                                       # no case of the table before these is capped
        assert T.score_grid(case.subsets.shape[1], case.src.shape[0], c) == "per-item", (case.name, "is capped")
    capped = [case for case in T.CAP_CASES if T.score_grid(case.subsets.shape[1], case.src.shape[0], c) == "capped"]
    assert len(capped) == len(T.CAP_CASES) >= 2, ("not every case of CAP_CASES reaches the form: capped", sorted({case.name for case in T.CAP_CASES} - {case.name for case in capped}))
    assert {case.src.shape[1] for case in capped} == {65, T.CHUNK + 1} and all(case.src.shape[0] == T.CAP_BATCH == 16 for case in capped)
    # the threshold is where the table says: one iteration fewer at the same batch is not capped
    assert T.score_grid(T.CAP_ITERS, T.CAP_BATCH, c) == "capped" and T.score_grid(T.CAP_ITERS - 1, T.CAP_BATCH, c) == "per-item", ("CAP_ITERS", T.CAP_ITERS)
    assert all(case.subsets.shape[1] == T.CAP_ITERS for case in T.CAP_CASES)
    for case in T.CAP_CASES:                                    # different data per item
        assert len({case.src[b].tobytes() for b in range(T.CAP_BATCH)}) == len({case.subsets[b].tobytes() for b in range(T.CAP_BATCH)}) == T.CAP_BATCH


def test_the_late_winners_sit_among_the_last_slots():
    """what makes the capped stride's later trips decide the result: the chosen slot is past every workgroup's first trip, and at
    n = CHUNK + 1 its count is one added to across two chunks"""
    c = T.source_constants()
    per, cap = T.score_blocks(T.CAP_ITERS, T.CAP_BATCH, c)
    first_trip = cap * c["FM_WAVES"]                            # slots the capped grid scores on its first trip (one per wave)
    late = [n for n in T.CAP_CASES if n.name.endswith("_late")]
    assert [n.src.shape[1] for n in late] == [T.CHUNK + 1]
    for name in (n.name for n in late):
        rec = T.reference(name)["records"]
        slot = 3 * rec["best_iter"] + rec["best_slot"]          # in slots, like first_trip
        assert (rec["ok"] == 1).all() and (slot >= 3 * (T.CAP_ITERS - 6)).all() and (rec["iters_run"] > T.CAP_ITERS - 6).all(), (name, rec)
        assert 3 * (T.CAP_ITERS - 6) >= 3 * first_trip          # the winner is on the stride's fourth trip or later
        assert (rec["valid"] > first_trip).all()                # and slots past the first trip are among the valid ones counted


def test_the_dense_pass_cases_past_the_cap():
    c = T.source_constants()
    (w, h), thr = T.EPI_FRAME, c["EPI_CAP"] * c["EPI_WG"]
    assert 0 < w * h - thr <= 2 * c["EPI_WG"], ("EPI_FRAME", T.EPI_FRAME, "is not within two workgroups past EPI_CAP * EPI_WG =", thr)
    assert ">1:partial-last" in T.epi_stride_forms(w * h, c), "EPI_FRAME does not reach the form >1:partial-last"
    assert all(T.epi_stride_forms(W * H, c) == {"1"} for W, H in T.FLOW_FRAMES + ((1, 1), (2, 3), (5, 3), (37, 23), (131, 67)))
    assert len(re.findall(r"p \+= \(size_t\)gridDim\.x \* EPI_WG", c["text"])) == 1 and "need < EPI_CAP ? (need ? need : 1) : EPI_CAP" in c["text"]
    flow, Fm, t, want = T.epi_cap_reference("noise")
    assert flow.shape == (T.EPI_BATCH, h, w, 2) and T.EPI_BATCH == 2 and not np.array_equal(flow[0], flow[1])
    for b in range(T.EPI_BATCH):
        bad = ~np.isfinite(flow[b].reshape(w * h, 2)).all(axis=1)
        mask = want["mask"][b].ravel()
        for side in (slice(0, thr), slice(thr, None)):          # movers, still pixels and not-finite pixels on each side of the threshold
            assert bad[side].sum() >= 2 and (mask[side] == 255).any() and (mask[side] == 0).sum() > bad[side].sum()
        assert want["records"]["not_finite"][b] == bad.sum() and want["records"]["movers"][b] == (mask == 255).sum()
        assert np.isnan(flow[b].reshape(w * h, 2)[:thr]).any() and np.isinf(flow[b].reshape(w * h, 2)[:thr]).any()
        assert np.isnan(flow[b].reshape(w * h, 2)[thr:]).any() and np.isinf(flow[b].reshape(w * h, 2)[thr:]).any()
    r = want["records"][1]                                      # one item whose unique maximum lies past the threshold
    at = np.flatnonzero(want["residual"][1].ravel() == want["residual"][1].max())
    assert len(at) == 1 and at[0] >= thr and (int(r["max_row"]), int(r["max_col"])) == divmod(int(at[0]), w) and r["max_residual"] == want["residual"][1].max()
    _, Fz, _, wz = T.epi_cap_reference("zero_F")
    assert not Fz.any()
    for r in wz["records"]:                                     # the count crosses both trips
        assert (r["max_residual"], r["max_row"], r["max_col"], r["movers"], r["not_finite"]) == (0, -1, -1, 0, w * h)
    assert not wz["residual"].any() and not wz["mask"].any()
