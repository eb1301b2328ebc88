"""tests/essential_ref.py (include/mavflow_essential.h in numpy) held to the definition against an independent float64 five-point solver
(tests/essential_indep_ref.py: SVD null space, numpy.roots, its own back-substitution), the need[] table and the sequential choice,
sample_subsets against its restatement, decomposeEssentialMat's algebra, and utils.rotation_matrix_to_euler / is_rotation_matrix against
the reference's own results (tests/golden/euler.npz).  Runs without a GPU.

Bounds.  Elimination in place of an SVD and bisection in place of an eigen-solver may lose a few digits against the independent solver,
not accuracy as a whole: a factor of 100 on what that solver reaches on the same sample, with a floor of 1e-9 on the distance from the
true matrix.  The RANSAC bounds (more than 95 % of the true inliers, fewer than 10 % of the outliers) are those of
tests/test_gpu_fundamental_shims.py.  1e-12 on the decomposition: float64 SVD round-off on orthogonal factors."""
import os

import numpy as np
import pytest

import essential_cases as T
import essential_indep_ref as I
import essential_ref as R
import fundamental_cases as FC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAMPLES = 300
_state = {}


def _dist(E, Et):
    E, Et = np.asarray(E).ravel(), np.asarray(Et).ravel()
    return min(np.sqrt(((E - Et) ** 2).sum()), np.sqrt(((E + Et) ** 2).sum()))


def minimal_samples():
    """300 minimal samples of the strong-motion scene, solved by the restatement and by the independent solver; computed once"""
    if not _state:
        src, dst, _, (Rm, t) = T.scene(200, 1, outliers=0, motion=T.STRONG)
        sub = T.subsets_for(2, 200, SAMPLES, 1)[0]
        sol = R.solve(src, dst, sub, T.CAM)
        x, y = R.normalised(src, T.CAM)
        X, Y = R.normalised(dst, T.CAM)
        indep = [I.solve(x[s], y[s], X[s], Y[s]) for s in sub]
        _state.update(sub=sub, sol=sol, pts=(x, y, X, Y), indep=indep, Et=T.true_E(Rm, t))
    return _state


def test_tables_are_the_monomial_products():
    assert sorted(sum(R.M2, [])) == sorted([0, 1, 1, 2, 2, 3, 3, 4, 5, 5, 6, 6, 7, 8, 8, 9]) and len(set(R.CUBE)) == 20 and len(set(R.QUAD)) == 10
    assert [tuple(I.ORDER[k]) for k in range(20)] == list(R.CUBE)          # the independent solver's order, parsed from the monomials' names
    assert [R.CUBE[k] for k in (4, 5, 6, 7, 8, 9)] == [(2, 0, 1), (2, 0, 0), (0, 2, 1), (0, 2, 0), (1, 1, 1), (1, 1, 0)]
    src = open(os.path.join(ROOT, "mav-detection_amd", "csrc", "kernels_essential.hip")).read()
    flat = lambda t: "{" + ", ".join("{" + ", ".join(str(v) for v in row) + "}" for row in t) + "}"
    assert flat(R.M2) in src and flat(R.M3) in " ".join(src.split())       # the kernel's tables are these


def test_best_slot_is_as_close_to_the_truth_as_the_independent_solver():
    s = minimal_samples()
    ours, theirs = np.empty(SAMPLES), np.empty(SAMPLES)
    for k in range(SAMPLES):
        v = s["sol"]["valid"][k]
        ours[k] = min([_dist(m, s["Et"]) for m in s["sol"]["models"][k][v]], default=np.inf)
        theirs[k] = min([_dist(m, s["Et"]) for m in s["indep"][k][0]], default=np.inf)
    print("distance of the best slot from +-E_true over", SAMPLES, "minimal samples: restatement max", ours.max(), "median", np.median(ours),
          "; independent solver max", theirs.max(), "median", np.median(theirs))
    bad = np.flatnonzero(~(ours <= np.maximum(100.0 * theirs, 1e-9)))
    assert len(bad) == 0, (bad[:5].tolist(), ours[bad[:5]], theirs[bad[:5]])


def test_valid_slots_satisfy_the_constraints_and_fit_their_pairs():
    """Every valid slot's |det E|, |2 E E^T E - tr(E E^T) E| and |X^T E x| at its five pairs, each bounded per sample by 100 x what the
    independent solver's models reach there.  Without the header's POLISH 78 of the 300 samples exceeded the bound (slots at clustered
    roots reached 1.1e-4 and 1.9e-4 in det and trace); with it none does."""
    s = minimal_samples()
    x, y, X, Y = s["pts"]
    worst_ours, worst_theirs, bad = np.zeros(3), np.zeros(3), []
    for k, sub in enumerate(s["sub"]):
        p = (x[sub], y[sub], X[sub], Y[sub])
        v = s["sol"]["valid"][k]
        ours = np.array([I.residuals(m, *p) for m in s["sol"]["models"][k][v]]).reshape(-1, 3)
        theirs = np.array([I.residuals(m, *p) for m in s["indep"][k][0]]).reshape(-1, 3)
        for m in s["sol"]["models"][k][v]:
            assert abs(np.sqrt((m * m).sum()) - 1.0) < 1e-15 and m[np.argmax(np.abs(m))] > 0
        if len(ours) == 0:
            continue
        worst_ours = np.maximum(worst_ours, ours.max(0))
        if len(theirs):
            worst_theirs = np.maximum(worst_theirs, theirs.max(0))
        if len(theirs) == 0 or not np.all(ours.max(0) <= 100.0 * theirs.max(0)):
            bad.append((k, ours.max(0).tolist(), theirs.max(0).tolist() if len(theirs) else None))
    print("largest (|det E|, |2EE^TE - tr(EE^T)E|, |X^T E x| at the sample) over all valid slots: restatement", worst_ours.tolist(),
          "; independent solver", worst_theirs.tolist(), "; samples over 100 x:", len(bad))
    assert not bad, bad[:5]


def test_ladder_finds_the_real_roots_numpy_finds():
    s = minimal_samples()
    aside, differ = 0, []
    for k in range(SAMPLES):
        r = s["indep"][k][1]
        gap = min((abs(a - b) / max(abs(a), abs(b), 1e-300) for i, a in enumerate(r) for b in r[i + 1:]), default=1.0)
        if gap <= 1e-6:
            aside += 1
            continue
        # the restatement's own polynomial has the same roots (its coefficients differ by a scale): compare the counts
        if int(np.sum(np.imag(r) == 0)) != int(s["sol"]["nroots"][k]):
            differ.append((k, int(np.sum(np.imag(r) == 0)), int(s["sol"]["nroots"][k])))
    print("samples set aside (two roots of numpy.roots within 1e-6 relative):", aside, "of", SAMPLES, "; slots per hypothesis:",
          float(s["sol"]["nroots"].mean()))
    assert aside < 0.05 * SAMPLES
    assert not differ, differ


@pytest.mark.parametrize("motion", ("strong", "pose0"))
def test_ransac_keeps_the_inliers_and_drops_the_outliers(motion):
    mo = T.STRONG if motion == "strong" else None
    src, dst, good, (Rm, t) = T.scene(200, 21, outliers=0.3, noise=0.1, motion=mo)
    out = R.find_one(src, dst, T.subsets_for(22, 200, 300, 1)[0], 1.0, 0.999, T.CAM)
    inl = out["inliers"].astype(bool)
    kept, extra = inl[good].mean(), inl[~good].mean()
    print(motion, "true inliers in the mask:", kept, "outliers in the mask:", extra, out["record"])
    assert out["record"]["ok"] == 1 and kept > 0.95 and extra < 0.10
    # F maps to the fundamental matrix of the same scene: the true inliers lie on its lines
    err = np.sqrt(np.asarray(__import__("fundamental_ref").pair_errors(out["F"], src[good], dst[good])))
    print(motion, "median distance of the true inliers from F's epipolar lines, pixels:", float(np.median(err)))
    assert np.median(err) < 1.0                                    # F maps to the scene's fundamental matrix: within the 1 px threshold
    Ki = np.linalg.inv(T.K_CAM)
    Fe = Ki.T @ out["E"] @ Ki
    assert _dist(out["F"], Fe / np.sqrt((Fe * Fe).sum())) < 1e-12  # F is K^-T E K^-1 of unit norm


def test_noise_free_scene_gives_the_true_matrices():
    for cam, K, name in ((T.CAM, T.K_CAM, "K_CAM"), (T.LITERAL, T.K_LITERAL, "literal")):
        src, dst, _, (Rm, t) = T.scene(100, 31, outliers=0, motion=T.STRONG, K=K)
        subs = T.subsets_for(32, 100, 20, 1)[0]
        out = R.find_one(src, dst, subs, 1e-3, 0.999, cam)
        assert out["record"]["ok"] == 1 and out["record"]["inliers"] == 100
        x, y = R.normalised(src, cam)
        X, Y = R.normalised(dst, cam)
        sub = subs[out["record"]["best_iter"]]
        theirs = min(_dist(m, T.true_E(Rm, t)) for m in I.solve(x[sub], y[sub], X[sub], Y[sub])[0])
        dE, dF = _dist(out["E"], T.true_E(Rm, t)), _dist(out["F"], FC.true_F(K, Rm, t))
        print(name, "distance from the true E:", dE, "(independent solver on the winning sample:", theirs, ") from the true F:", dF, out["record"])
        assert dE <= max(100.0 * theirs, 1e-9)                     # the bound of the minimal samples' check
        assert dF <= max(100.0 * theirs, 1e-9)                     # F is the scene's K^-T [t]x R K^-1, under the same bound
        Ki = np.linalg.inv(K)
        Fe = Ki.T @ out["E"] @ Ki
        assert _dist(out["F"], Fe / np.sqrt((Fe * Fe).sum())) < 1e-12


@pytest.mark.parametrize("n", (5, 6, 63, 64, 65, 257, 1000, 1025))
@pytest.mark.parametrize("confidence", (0.5, 0.99, 0.999))
def test_need_table_is_monotone_and_away_from_ties(n, confidence):
    for max_iters in (65, 1000):
        need = R.need_table(n, confidence, max_iters)
        assert np.all(need[:5] == max_iters) and need[n] == 0 and np.all(np.diff(need[4:].astype(np.int64)) <= 0)
        for g in range(5, n + 1):
            q = R.need_quotient(n, g, confidence)
            if q is None:
                continue
            ln, ld = q
            if ld >= 0.0 or -ln >= max_iters * (-ld):
                continue
            assert abs((ln / ld) % 1.0 - 0.5) > 1e-6, (n, g, confidence, ln / ld)


def test_choice_equals_a_brute_loop():
    rng = np.random.default_rng(11)
    for trial in range(300):
        n = int(rng.integers(5, 80))
        mi = int(rng.integers(1, 70))
        count = rng.integers(-1, n + 1, (mi, 10)).astype(np.int32)
        count[rng.random((mi, 10)) < 0.5] = -1
        need = R.need_table(n, float(rng.choice((0.5, 0.99, 0.999))), mi)
        niters, best, bc, ran, valid = mi, (-1, -1), 4, 0, 0
        for it in range(mi):
            if not it < niters:
                break
            ran += 1
            for s in range(10):
                valid += count[it, s] >= 0
                if count[it, s] >= 0 and count[it, s] > bc:
                    best, bc = (it, s), int(count[it, s])
                    niters = min(niters, int(need[bc]))
        assert R.choose(count, need) == (best[0], best[1], ran, valid, bc if best[0] >= 0 else 0)
    count = np.full((2, 10), 20, np.int32)                         # all-inlier data: need[n] = 0 stops the loop after the first iteration
    count[0, 0] = 10
    assert R.choose(count, R.need_table(20, 0.999, 2)) == (0, 1, 1, 10, 20)


def test_special_cases_are_what_they_are_named_for():
    ref = {name: T.reference(name)["records"] for name in ("all_inliers", "no_valid", "equal_counts", "beside_threshold", "threshold_0", "bad_subsets")}
    r = ref["all_inliers"][0]
    assert (r["ok"], r["inliers"], r["best_iter"], r["iters_run"]) == (1, 65, 0, 1) and r["valid"] > 1
    r = ref["no_valid"][0]
    assert (r["ok"], r["valid"], r["iters_run"], r["best_iter"], r["best_slot"]) == (0, 0, 65, -1, -1)
    r = ref["equal_counts"][0]
    assert r["ok"] == 1 and r["best_iter"] % 2 == 0               # of a repeated pair of hypotheses the first wins
    inl = T.reference("beside_threshold")["inliers"][0]
    assert inl[10] == 1 and inl[11] == 0 and inl.sum() == 64
    assert ref["threshold_0"][0]["valid"] > 0
    assert ref["bad_subsets"][2]["ok"] == 0 and ref["bad_subsets"][2]["valid"] == 0 and ref["bad_subsets"][0]["ok"] == 1
    c = T.BY_NAME["beside_threshold"]
    for sub in ([0, 1, 2, 3, 65], [0, 1, 2, 3, 0], [-1, 1, 2, 3, 4]):
        assert not R.solve(c.src[0], c.dst[0], [sub], c.camera)["valid"].any()
    # across_blocks: slot 61 is accepted and cuts niters to 4, slot 64 -- the next block of 64 -- still wins, iteration 7 does not begin
    c = T.BY_NAME["across_blocks"]
    one = R.find_one(c.src[0], c.dst[0], c.subsets[0], c.threshold, c.confidence, c.camera)
    count, need = one["count"], R.need_table(c.src.shape[1], c.confidence, c.subsets.shape[1])
    assert count[:6].max() < 51 and np.all(need[:51] > 6)          # nothing before iteration 6 cuts niters
    assert count[6, :4].max() == count[6, 1] == 56 and need[56] == 4 and count[6, 4] == 68 and count[7].max() == 68
    r = one["record"]
    assert (r["ok"], r["best_iter"], r["best_slot"], r["inliers"], r["iters_run"]) == (1, 6, 4, 68, 7)
    assert r["valid"] == np.count_nonzero(count[:7] >= 0) < np.count_nonzero(count >= 0)
    assert len(T.CASES) == len(T.SIZES) + len(T.ITERS) + 2 + 9 and sum(c.subsets.shape[1] >= 1000 for c in T.CASES) <= 2


@pytest.mark.parametrize("n", (5, 6, 65, 1000))
def test_sample_subsets_equals_its_restatement(mav, n):
    from mavflow import essential as K
    got = K.sample_subsets(3, n, 50, 2)
    assert got.dtype == np.int32 and got.shape == (2, 50, 5) and np.array_equal(got, T.subsets_for(3, n, 50, 2))
    assert got.min() >= 0 and got.max() < n and all(len(set(s)) == 5 for s in got.reshape(-1, 5).tolist())
    if n == 5:
        assert np.array_equal(np.sort(got, -1), np.broadcast_to(np.arange(5), got.shape))       # every subset is a permutation of all pairs
    g = np.random.default_rng(3)
    assert np.array_equal(K.sample_subsets(g, n, 50, 2), got)                                  # a Generator: ONE call of .random
    assert g.random() == np.random.default_rng(3).random(2 * 50 * 5 + 1)[-1]
    with pytest.raises(ValueError):
        K.sample_subsets(3, 4, 5)


def test_decompose_essential_mat(mav):
    from mavflow import essential as K
    worst = np.zeros(3)
    for k, (Rm, t) in enumerate([T.STRONG, FC.pose(0), FC.pose(2), (FC.rotation(-2.0, 0.4, 2.5), np.array([-1.0, 2.0, -0.3]))]):
        E = T.true_E(Rm, t) * (1.0 if k % 2 == 0 else -3.0)
        R1, R2, tt = K.decomposeEssentialMat(E)
        assert tt.shape == (3, 1) and R1.shape == (3, 3) and R2.shape == (3, 3)
        for Rq in (R1, R2):
            worst[0] = max(worst[0], np.abs(Rq.T @ Rq - np.eye(3)).max(), abs(np.linalg.det(Rq) - 1.0))
            tx = np.array([[0, -tt[2, 0], tt[1, 0]], [tt[2, 0], 0, -tt[0, 0]], [-tt[1, 0], tt[0, 0], 0]])
            back = tx @ Rq
            worst[1] = max(worst[1], _dist(back / np.sqrt((back * back).sum()), E / np.sqrt((E * E).sum())))
        worst[2] = max(worst[2], min(np.abs(R1 - Rm).max(), np.abs(R2 - Rm).max()))
    print("decomposeEssentialMat: orthogonality / determinant", worst[0], "[t]x R against +-E", worst[1], "the true rotation", worst[2])
    assert worst[0] <= 1e-12 and worst[1] <= 1e-12 and worst[2] <= 1e-12
    # on a noise-free scene one of R1 and R2 of the fitted E is the true rotation, under the bound of the minimal samples' check
    src, dst, _, (Rm, t) = T.scene(100, 31, outliers=0, motion=T.STRONG)
    out = R.find_one(src, dst, T.subsets_for(32, 100, 20, 1)[0], 1e-3, 0.999, T.CAM)
    x, y = R.normalised(src, T.CAM)
    X, Y = R.normalised(dst, T.CAM)
    sub = T.subsets_for(32, 100, 20, 1)[0][out["record"]["best_iter"]]
    theirs = min(_dist(m, T.true_E(Rm, t)) for m in I.solve(x[sub], y[sub], X[sub], Y[sub])[0])
    R1, R2, _ = K.decomposeEssentialMat(out["E"])
    d = min(np.sqrt(((R1 - Rm) ** 2).sum()), np.sqrt(((R2 - Rm) ** 2).sum()))
    print("distance of the nearer of R1, R2 from the true rotation:", d, "; the independent solver's E on the winning sample:", theirs)
    assert d <= max(100.0 * theirs, 1e-9)
    with pytest.raises(ValueError):
        K.decomposeEssentialMat(np.zeros((3, 4)))


def test_euler_angles_equal_the_reference_bit_for_bit(mav):
    from mavflow import utils
    g = np.load(os.path.join(ROOT, "tests", "golden", "euler.npz"))
    flags = g["is_rotation"]
    assert len(g["singular"]) >= 8 and (~flags).sum() >= 4
    for k, ok in enumerate(flags):
        Rm = g[f"R{k}"]
        got = utils.is_rotation_matrix(Rm)
        assert isinstance(got, bool) and got == bool(ok), k
        if ok:
            e = utils.rotation_matrix_to_euler(Rm)
            assert e.dtype == g[f"euler{k}"].dtype and e.tobytes() == g[f"euler{k}"].tobytes(), (k, e, g[f"euler{k}"])
        else:
            with pytest.raises(AssertionError):
                utils.rotation_matrix_to_euler(Rm)
    for k in g["singular"]:
        assert g[f"euler{int(k)}"][2] == 0.0                      # the singular branch sets z = 0


def test_python_layer_refuses_what_is_not_built(mav):
    import inspect
    from mavflow import essential as K
    from mavflow.detector import Detector
    pts = np.zeros((9, 2), np.float32)
    for method in (K.LMEDS, 0):
        with pytest.raises(NotImplementedError):
            K.findEssentialMat(pts, pts, method=method)
    E, mask = K.findEssentialMat(pts[:4], pts[:4])               # n < 5: no GPU is touched
    assert E is None and mask.shape == (4, 1) and mask.dtype == np.uint8 and not mask.any()
    sig = inspect.signature(K.findEssentialMat).parameters
    assert list(sig) == ["points1", "points2", "focal", "pp", "method", "prob", "threshold", "maxIters", "mask", "rng"]
    assert (sig["focal"].default, sig["pp"].default, sig["method"].default, sig["prob"].default, sig["threshold"].default,
            sig["maxIters"].default) == (1.0, (0.0, 0.0), K.RANSAC, 0.999, 1.0, 1000)
    assert K.camera_of(2.0, (3.0, 4.0)) == (2.0, 2.0, 3.0, 4.0) and K.camera_of(T.K_CAM) == T.CAM
    assert list(inspect.signature(Detector.get_rotation).parameters) == ["self", "flow_uv", "use_fundamental"]
    assert "five-point" in open(os.path.join(ROOT, "DESIGN.md")).read()


# ---- the case table past the score grid's cap (computed from the source's constants and the restatement alone) -----------------------------
def test_the_score_grid_is_capped_where_the_table_says():
    import re
    c = T.source_constants()
    assert re.search(r"const int cap = EM_GRID_CAP / a\.B < 1 \? 1 : EM_GRID_CAP / a\.B;\s*hipLaunchKernelGGL\(k_em_score, dim3\(per < cap \? per : cap, a\.B\)", c["text"])
    assert re.search(r"const int per = \(slots \+ EM_WAVES \* EM_SLOTS_PER_WAVE - 1\) / \(EM_WAVES \* EM_SLOTS_PER_WAVE\);", c["text"]) and T.CHUNK == c["EM_CHUNK"]
    assert "const int slots = EM_SLOTS * a.max_iters;" in c["text"] and c["EM_SLOTS"] == 10
    for case in T.CASES:                                       # no case of the table before these is capped
        assert T.score_grid(case.subsets.shape[1], case.src.shape[0], c) == "per-item", (case.name, "is capped")
    capped = [case for case in T.CAP_CASES if T.score_grid(case.subsets.shape[1], case.src.shape[0], c) == "capped"]
    assert len(capped) == len(T.CAP_CASES) >= 2, ("not every case of CAP_CASES reaches the form: capped", sorted({case.name for case in T.CAP_CASES} - {case.name for case in capped}))
    assert {case.src.shape[1] for case in capped} == {65, T.CHUNK + 1} and all(case.src.shape[0] == T.CAP_BATCH == 16 for case in capped)
    # the threshold is where the table says: one iteration fewer at the same batch is not capped
    assert T.score_grid(T.CAP_ITERS, T.CAP_BATCH, c) == "capped" and T.score_grid(T.CAP_ITERS - 1, T.CAP_BATCH, c) == "per-item", ("CAP_ITERS", T.CAP_ITERS)
    assert all(case.subsets.shape[1] == T.CAP_ITERS == 205 for case in T.CAP_CASES)
    for case in T.CAP_CASES:                                    # different data per item
        assert len({case.src[b].tobytes() for b in range(T.CAP_BATCH)}) == len({case.subsets[b].tobytes() for b in range(T.CAP_BATCH)}) == T.CAP_BATCH


def test_the_late_winners_sit_among_the_last_slots():
    """what makes the capped stride's later trips decide the result: the chosen slot is past every workgroup's first trip"""
    c = T.source_constants()
    first_trip = T.score_blocks(T.CAP_ITERS, T.CAP_BATCH, c)[1] * c["EM_WAVES"]          # slots the capped grid scores on its first trip
    late = [n for n in T.CAP_CASES if n.name.endswith("_late")]
    assert [n.src.shape[1] for n in late] == [T.CHUNK + 1]
    for name in (n.name for n in late):
        rec = T.reference(name)["records"]
        slot = c["EM_SLOTS"] * rec["best_iter"] + rec["best_slot"]                       # in slots, like first_trip
        assert (rec["ok"] == 1).all() and (rec["best_iter"] >= T.CAP_ITERS - 6).all() and (slot >= c["EM_SLOTS"] * (T.CAP_ITERS - 6)).all(), (name, rec)
        assert c["EM_SLOTS"] * (T.CAP_ITERS - 6) >= 3 * first_trip                       # the winner is on the stride's fourth trip
