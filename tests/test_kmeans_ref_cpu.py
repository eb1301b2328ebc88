"""tests/kmeans_ref.py held to the definition of k-means, independently of its own code: after every assignment each label is a nearest
centre of the centres it was assigned against (the argmin recomputed in float64 agrees wherever the float32 gap is no tie), every centre
is the mean of its members, no cluster is empty, the compactness does not rise from one iteration to the next on repair-free runs, and on
well-separated blobs with one centre drawn inside each blob the partition is scipy's kmeans2(minit="matrix") up to the label order.
Runs without a GPU."""
import numpy as np
import pytest

import kmeans_ref as R


def _blobs(seed, N, D, K, sigma=20.0):
    rng = np.random.default_rng(seed)
    centres = rng.uniform(100, 3000, (K, D))
    which = rng.integers(0, K, N)
    which[:K] = np.arange(K)
    x = centres[which] + rng.normal(0, sigma, (N, D))
    return (np.round(x * 256) / 256).astype(np.float32), centres, which, rng


CASES = [(1, 500, 1, 3), (2, 2000, 2, 8), (3, 1500, 3, 8), (4, 900, 4, 16)]


@pytest.mark.parametrize("seed,N,D,K", CASES)
def test_every_label_is_a_nearest_centre_and_every_centre_a_mean(seed, N, D, K):
    x, _, _, rng = _blobs(seed, N, D, K)
    init = rng.uniform(x.min(0), x.max(0), (K, D)).astype(np.float32)
    run = R.attempt(x, init, max_iter=10, eps=0.0)
    xd = x.astype(np.float64)
    assert 1 <= run["iterations"] <= 9
    for step in run["trace"]:
        c = step["centers"].astype(np.float64)
        d64 = ((xd[:, None, :] - c[None]) ** 2).sum(-1)
        moved = {j for (_, _, j, _, _) in step["repairs"]}
        mine = d64[np.arange(N), step["labels"]]
        gap_ok = mine <= d64.min(1) * (1 + 1e-6) + 1e-9                # a nearest centre, to float32's rounding of the distance
        assert all(gap_ok[i] or i in moved for i in range(N))
        clear = np.sort(d64, 1)
        clear = (clear[:, 1] - clear[:, 0] > 1e-5 * clear[:, 1]) if K > 1 else np.ones(N, bool)
        keep = clear & ~np.isin(np.arange(N), list(moved))
        assert np.array_equal(step["labels"][keep], d64.argmin(1)[keep])
        assert step["n"].min() >= 1 and step["n"].sum() == N           # no cluster is empty after the repairs
        assert np.array_equal(np.bincount(step["labels"], minlength=K), step["n"])
    for k in range(K):
        members = xd[run["labels"] == k]
        assert len(members) == run["counts"][k] >= 1
        assert np.array_equal(run["centers"][k], members.mean(0).astype(np.float32)) or np.allclose(run["centers"][k], members.mean(0), rtol=1e-6)
    # the compactness is the sum of the squared distances to the final centres
    want = ((xd - run["centers"].astype(np.float64)[run["labels"]]) ** 2).sum()
    assert run["compactness"] == pytest.approx(want, rel=1e-5)


@pytest.mark.parametrize("seed,N,D,K", CASES)
def test_compactness_does_not_rise_on_repair_free_runs(seed, N, D, K):
    x, centres, _, rng = _blobs(seed + 10, N, D, K)
    init = (centres + rng.normal(0, 60, centres.shape)).astype(np.float32)       # inside or beside each blob: nothing runs empty
    prev = None
    seen = 0
    for m in range(2, 9):                                                        # the same attempt cut after 1 .. 7 assignments
        run = R.attempt(x, init, max_iter=m, eps=0.0)
        if run["repairs"]:
            continue
        seen += 1
        if prev is not None:
            assert run["compactness"] <= prev * (1 + 1e-6)
        prev = run["compactness"]
    assert seen >= 3


@pytest.mark.parametrize("seed,N,D,K", CASES)
def test_partition_equals_scipy_on_separated_blobs(seed, N, D, K):
    from scipy.cluster.vq import kmeans2
    rng = np.random.default_rng(seed + 20)
    centres = (np.arange(K)[:, None] * 400.0 + 100.0) + rng.uniform(-20, 20, (K, D))        # 400 apart, sigma 10: well separated
    which = rng.integers(0, K, N)
    which[:K] = np.arange(K)
    x = (np.round((centres[which] + rng.normal(0, 10, (N, D))) * 256) / 256).astype(np.float32)
    init = (centres + rng.normal(0, 10, centres.shape)).astype(np.float32)                   # one centre inside each blob
    ref = R.kmeans(x, init[None], max_iter=20, eps=0.0)
    _, lab = kmeans2(x.astype(np.float64), init.astype(np.float64), iter=20, minit="matrix")
    assert ref["repairs"] == 0
    # the same partition up to the label order (here the order too: both start from the same centres)
    pairs = {(int(a), int(b)) for a, b in zip(ref["labels"], lab)}
    assert len(pairs) == K and len({a for a, _ in pairs}) == K and len({b for _, b in pairs}) == K
    assert np.array_equal(ref["labels"], which)


def test_first_minimum_highest_index_and_first_best():
    # two centres at the same distance: the first; an empty cluster takes the donor's farthest sample, the highest index among equals
    x = np.array([[0.0], [2.0], [2.0], [4.0], [4.0]], np.float32)
    run = R.attempt(x, np.array([[1.0], [3.0], [100.0]], np.float32), max_iter=2, eps=0.0)
    step = run["trace"][0]
    assert step["ties"] == 2 and step["repairs"] == [(2, 0, 0, pytest.approx(16.0 / 9.0, rel=1e-6), 1)]
    assert list(run["labels"]) == [2, 0, 0, 1, 1] and run["iterations"] == 1 and run["repairs"] == 1
    same = R.attempt(np.full((6, 2), 3.0, np.float32), np.array([[0, 0], [50, 50], [60, 60]], np.float32), max_iter=2)
    assert [r[2] for r in same["trace"][0]["repairs"]] == [5, 4] and all(r[3] == 0.0 and r[4] > 1 for r in same["trace"][0]["repairs"])
    twin = R.kmeans(x, np.array([[[1.0], [3.0]], [[1.0], [3.0]]], np.float32))
    assert twin["best_attempt"] == 0 and twin["attempts"][0]["compactness"] == twin["attempts"][1]["compactness"]
    assert R.clamp_iter(1) == 2 and R.clamp_iter(1000) == 100 and R.eps_squared(-1.0) == 0.0 and R.eps_squared(3.0) == 9.0
