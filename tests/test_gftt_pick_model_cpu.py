"""The numpy model of the device's corner sort and pick (tests/gftt_pick_model.py) against the sequential rule (lk_ref.good_features's
loop on a key list), on the candidate families that no small image produces on demand; and the restatement of the candidate step with
cv2's mask.  Equality throughout.  No GPU; the GPU tests run the same families through mav_stage_corner_pick."""
import numpy as np
import pytest

import gftt_pick_model as gm
import lk_ref
from test_lk_ref_cpu import blurred_noise

F = np.float32
W, H = 96, 64
DIAG = float(np.hypot(W, H))
MIN_DISTANCES = (0, 0.99, 1, 1.5, 7, 7.5, 40, DIAG + 1)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def families():
    yield "ramp300", gm.ramp(300, W, H)                                   # one row and a half
    yield "snake700", gm.ramp(700, W, H)                                  # snaking over 15 rows
    yield "plateau", gm.plateau(W, H, 1)
    yield "all_equal", gm.all_equal(W, H)
    yield "sparse", gm.random_set(W, H, 40, 2)
    yield "random", gm.random_set(W, H, 900, 3)
    yield "ties", gm.random_set(W, H, 1500, 4, levels=3)
    yield "every_second_pixel", gm.random_set(W, H, W * H // 2, 5)


def check(name, keys, w, h, mc, md):
    keys = np.random.default_rng(7).permutation(keys)                     # the append order is arbitrary
    got, stats = gm.good_features_from_keys(keys, w, h, mc, md, want_stats=True)
    ref = gm.sequential(keys, w, mc, md)
    assert same(got, ref), (name, mc, md, len(got), len(ref), stats)
    return stats


def test_the_sort_is_the_descending_order():
    rng = np.random.default_rng(0)
    for n in (0, 1, 2, 3, 1000, 4096, 4097, 20000):
        keys = gm.random_set(400, 300, n, n, levels=0 if n % 2 else 5)
        s, global_steps = gm.sort_keys(rng.permutation(keys))
        assert np.array_equal(s, np.sort(keys)[::-1]), n
        assert (global_steps > 0) == (n > gm.SORT_CHUNK), n                # beyond one LDS chunk the merge needs global-memory steps
    assert len(np.unique(gm.all_equal(W, H))) == (W - 2) * (H - 2)        # equal values: the index keeps the keys distinct


@pytest.mark.parametrize("name,keys", list(families()), ids=[n for n, _ in families()])
def test_model_equals_the_sequential_rule(name, keys):
    full = len(gm.sequential(keys, W, 65536, 7))
    for md in MIN_DISTANCES:
        for mc in (1, max(full // 2, 1), 65536):
            check(name, keys, W, H, mc, md)
    # a cut in the middle of what THIS min_distance accepts, too
    for md in (1.5, 7.5):
        n = len(gm.sequential(keys, W, 65536, md))
        check(name, keys, W, H, max(n // 2, 1), md)


def test_the_ramp_is_what_its_name_says():
    """A falling line 2 px apart decides one candidate per round: the rounds grow with the length, with no small bound."""
    rounds = []
    for n in (100, 300, 900, 2700):
        w, h = 200, 160
        stats = check(f"ramp{n}", gm.ramp(n, w, h), w, h, 65536, 2.5)
        rounds.append(stats["rounds"])
        assert stats["chunks"] == (n + gm.CHUNK - 1) // gm.CHUNK
        assert stats["max_rounds"] <= gm.CHUNK                            # the first undecided survivor of a chunk always decides
    assert all(b > 2 * a for a, b in zip(rounds, rounds[1:])), rounds
    assert rounds[-1] >= 2700 // 2
    # a random set of the same size needs a handful
    stats = check("random", gm.random_set(200, 160, 2700, 1), 200, 160, 65536, 2.5)
    assert stats["rounds"] < 40 * stats["chunks"], stats


def test_a_full_buffer():
    """Exactly the capacity: every second interior pixel of 1026 x 514, one value."""
    w, h = 1026, 514
    keys = gm.all_equal(w, h, every=2)
    assert len(keys) == gm.CAPACITY
    for mc, md in ((65536, 7), (1, float(np.hypot(w, h)) + 1), (65536, 0), (3000, 40)):
        stats = check("capacity", keys, w, h, mc, md)
        assert md < 1 or stats["chunks"] >= 1


def test_slots_per_cell_suffice():
    """The densest acceptance: all interior pixels, min_distance at and just above each small integer (the model asserts a free slot)."""
    keys = gm.all_equal(W, H)
    for md in (1, 1.4, 1.5, 2, 2.1, 2.9, 3, 4, 4.01, 5):
        check("dense", keys, W, H, 65536, md)
    for w, h in ((3, 3), (4, 4), (5, 3), (7, 7), (3, 40)):                 # the grid fits the eigenvalue map on tiny frames too
        for md in (1, 2, 3, 5):
            check("tiny", gm.all_equal(w, h), w, h, 65536, md)


# ---- the mask ------------------------------------------------------------------------------------------------------------------------
def test_masked_candidates():
    img = blurred_noise(160, 120, 3)
    eig = lk_ref.min_eigen(img)
    v0, i0 = lk_ref.corner_candidates(eig, 0.2)
    for mask in (None, np.ones((120, 160), np.uint8), np.full((120, 160), 255, np.uint8)):
        v, i = gm.masked_candidates(eig, mask, 0.2)
        assert same(v, v0) and np.array_equal(i, i0)
    assert same(gm.good_features_masked(img, None), lk_ref.good_features(img))
    # hide the global maximum: the threshold falls and candidates that were below it come in
    ym, xm = np.unravel_index(np.argmax(eig), eig.shape)
    mask = np.ones((120, 160), np.uint8)
    mask[max(ym - 10, 0):ym + 11, max(xm - 10, 0):xm + 11] = 0
    v, i = gm.masked_candidates(eig, mask, 0.2)
    old_thr = F(np.float64(eig.max()) * 0.2)
    assert eig[mask != 0].max() < eig.max() and (v <= old_thr).any() and v.max() == eig[mask != 0].max()
    assert np.all(mask.reshape(-1)[i] != 0)
    kept = mask.reshape(-1)[i0] != 0
    assert np.isin(i0[kept], i).all() and len(i) > kept.sum()              # everything visible before stays, more comes in
    # a masked-out neighbour still suppresses: hide only the maximum's own pixel; its 8 neighbours stay out
    one = np.ones((120, 160), np.uint8)
    one[ym, xm] = 0
    _, i1 = gm.masked_candidates(eig, one, 0.2)
    ring = [(ym + j) * 160 + xm + k for j in (-1, 0, 1) for k in (-1, 0, 1)]
    assert not np.isin(ring, i1).any()
    # half planes, nothing at all
    half = np.zeros((120, 160), np.uint8)
    half[:, 80:] = 7
    _, ih = gm.masked_candidates(eig, half, 0.2)
    assert len(ih) and np.all(ih % 160 >= 80)
    v, i = gm.masked_candidates(eig, np.zeros((120, 160), np.uint8), 0.2)
    assert len(v) == 0 and gm.good_features_masked(img, np.zeros((120, 160), np.uint8)).shape == (0, 2)
