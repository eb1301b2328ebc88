"""The device plan of the connected components (tests/components_model.py) gives the restatement's outputs whatever the order in which
the border unions are applied: the outputs depend on the partition into components alone."""
import numpy as np
import pytest

import components_cases as CC
import components_model as M
import components_ref as R

FRAMES = [f for f in CC.FRAMES if f[0] > CC.T_W or f[1] > CC.T_H] + [(CC.T_W, CC.T_H)]      # frames with borders, and one without


@pytest.mark.parametrize("W,H", FRAMES)
@pytest.mark.parametrize("connectivity", (4, 8))
def test_every_order_of_the_border_unions_gives_the_restatement(W, H, connectivity):
    pats = CC.patterns(W, H)
    for name in ("serpentine", "serpentine_t", "comb", "tile_checker", "corner_pairs", "rings", "noise_41", "noise_59", "full"):
        want = R.components(pats[name], connectivity, 2, 40)
        for seed in (None, 0, 1, 2):
            order = None if seed is None else np.random.default_rng(seed)
            got = M.run(pats[name], connectivity, 2, 40, order=order, skip_redundant=seed != 2)
            assert np.array_equal(got[0], want[0]), (name, seed, "labels")
            assert got[1] == want[1], (name, seed, "counts")
            assert got[2].tobytes() == want[2].tobytes(), (name, seed, "table")


def test_a_union_never_raises_a_word_and_ends_within_its_bound():
    rng = np.random.default_rng(5)
    W, H = 131, 67
    mask = CC.patterns(W, H)["noise_59"]
    L = M.tile_roots(mask, 4)
    todo = M.border_unions(mask, 4)
    assert len(todo) > 50
    for i in rng.permutation(len(todo)):
        a, b = todo[i]
        before = L.copy()
        rounds = M.union(L, a, b)
        assert rounds <= max(a, b) + 1
        assert (L <= before).all() and (L[L >= 0] <= np.nonzero(L >= 0)[0]).all()
        assert M.find(L, a) == M.find(L, b)


def test_tile_roots_are_first_pixels_inside_their_tile():
    W, H = 2 * CC.T_W - 1, 3 * CC.T_H + 1
    mask = CC.patterns(W, H)["full"]
    L = M.tile_roots(mask, 4).reshape(H, W)
    for y0 in range(0, H, CC.T_H):
        for x0 in range(0, W, CC.T_W):
            assert (L[y0:y0 + CC.T_H, x0:x0 + CC.T_W] == y0 * W + x0).all()
