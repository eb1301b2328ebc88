"""The homography fit on the GPU (k_homography_fit, csrc/kernels_motion.hip) against the restatement tests/global_motion_ref.py on the
table of tests/fit_edge_cases.py, whose entries take the eigen-solver through each of its branches (tests/test_fit_edge_cases_cpu.py
shows that they do).  ok and the bytes of H are compared; no tolerance appears in this file."""
import warnings

import numpy as np
import pytest

import fit_edge_cases as F
import global_motion_ref as R
from global_motion_cases import H_TRUE, project

pytestmark = pytest.mark.gpu

TABLE = F.table()


def restated(src, dst):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return R.find_homography(src, dst)


@pytest.fixture(scope="module")
def expected():
    return {name: restated(src, dst) for name, src, dst in TABLE}


@pytest.fixture(scope="module")
def ctx():
    from mavflow import _lib
    with _lib.Context(64, 64, 65) as c:
        yield c


@pytest.mark.parametrize("name", [t[0] for t in TABLE])
def test_entry_alone(ctx, expected, name):
    src, dst = next((s, d) for n, s, d in TABLE if n == name)
    H, ok = ctx.find_homography(src, dst)
    He, oke = expected[name]
    assert int(ok[0]) == oke and H[0].tobytes() == He.tobytes(), (name, int(ok[0]), oke, H[0], He)


def test_all_entries_as_one_batch(ctx, expected):
    """One workgroup per item: items that need different numbers of sweeps and of refinement steps, items that fail before the solver
    and items that meet inf and NaN inside it, side by side.  The batch call takes one n for all items: every entry's pairs are
    repeated up to the longest entry's n = 1000 (repeated pairs change the sums, so the restatement is taken of the repeated arrays)."""
    n = max(len(s) for _, s, _ in TABLE)
    items = []
    for name, src, dst in TABLE:
        reps = -(-n // len(src))
        items.append((name, np.tile(src, (reps, 1))[:n], np.tile(dst, (reps, 1))[:n]))
    H, ok = ctx.find_homography(np.stack([i[1] for i in items]), np.stack([i[2] for i in items]))
    seen = set()
    for b, (name, src, dst) in enumerate(items):
        He, oke = restated(src, dst)
        seen.add(oke)
        assert int(ok[b]) == oke and H[b].tobytes() == He.tobytes(), (name, int(ok[b]), oke)
    assert seen == {0, 1}
    # and each of them alone gives the same bytes as inside the batch
    for b in (0, 3, len(items) - 2):
        H1, ok1 = ctx.find_homography(items[b][1], items[b][2])
        assert int(ok1[0]) == int(ok[b]) and H1[0].tobytes() == H[b].tobytes(), items[b][0]


def test_batch_of_65_copies_with_distinct_noise(ctx):
    """More items than one wavefront has lanes."""
    rng = np.random.default_rng(65)
    src = rng.integers(20, 620, (33, 2)).astype(np.float64)
    base = project(H_TRUE, src)
    dsts = np.stack([base + rng.normal(0, 0.7, base.shape).astype(np.float32) for _ in range(65)])
    H, ok = ctx.find_homography(np.broadcast_to(src, dsts.shape).copy(), dsts)
    assert ok.all()
    assert len({H[b].tobytes() for b in range(65)}) == 65
    for b in range(65):
        assert H[b].tobytes() == restated(src, dsts[b])[0].tobytes(), b
