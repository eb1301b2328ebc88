"""The sparse path's case table (tests/sparse_cases.py) is what it claims to be -- checked from the predicates and the numpy
restatement (tests/lk_ref.py) alone, without a GPU: every kernel form is reached, every case is what its name says, every exit of
the tracker's per-level loop is taken at level 0 and at a coarser level, and every tracker case on a frame of 43 x 43 or more tracks
at least half of the points placed inside the frame (a case that tracks nothing compares nothing)."""
import time

import numpy as np
import pytest

import gftt_pick_model as gm
import lk_ref
import sparse_cases as sc

F = np.float32


def test_every_form_is_reached():
    """Each frame and each tracker case reaches the forms it names, together they reach every form of FORMS, and nothing outside
    FORMS and UNTESTED occurs (UNTESTED: arguments the entry points refuse, see the comment there)."""
    reached = {g: set() for g in sc.FORMS}
    for item, forms_of in [(f, sc.frame_forms) for f in sc.FRAMES] + [(c, sc.case_forms) for c in sc.CASES]:
        got = forms_of(item)
        names = {f for _, f in got}
        assert item.expects <= names, (item.name, sorted(item.expects - names))
        for g, f in got:
            reached[g].add(f)
    for g, f in sc.other_forms():
        reached[g].add(f)
    for g, forms in sc.FORMS.items():
        assert forms <= reached[g], (g, sorted(forms - reached[g]))
        assert reached[g] <= forms | sc.UNTESTED.get(g, set()), (g, sorted(reached[g] - forms))
        assert not (sc.UNTESTED.get(g, set()) & reached[g])
    assert set(sc.UNTESTED) <= set(sc.FORMS)


def test_constants_are_the_librarys():
    from mavflow import _lib
    assert (sc.MAX_POINTS, sc.MAX_WIN, sc.MAX_LEVEL, sc.MAX_CANDIDATES) == (_lib.LK_MAX_POINTS, _lib.LK_MAX_WIN, _lib.LK_MAX_LEVEL,
                                                                           _lib.GFTT_MAX_CANDIDATES)
    assert lk_ref.HIST_BINS == _lib.LK_HIST_BINS


def test_predicates_at_the_shapes_they_were_chosen_for():
    """the launchers' arithmetic at the table's shapes, spelled out: a changed constant in kernels_lk.hip must change these too"""
    assert [sc.reflections(p, n) for p, n in ((-7, 9), (15, 9), (-7, 8), (-7, 7), (-7, 2), (-1, 2), (5, 1))] == [1, 1, 1, 2, 7, 1, 0]
    assert sc.eig_tile_forms(320, 240, 15) == {"full"} and sc.eig_tile_forms(161, 123, 15) == {"ragged"}
    assert sc.eig_tile_forms(1, 9, 15) == {"ragged", "narrow", "n1"} and "multi-reflect" in sc.eig_tile_forms(5, 3, 7)
    assert "multi-reflect" not in sc.eig_tile_forms(5, 3, 1) and "multi-reflect" in sc.eig_tile_forms(2, 2, 7)
    assert sc.cand_forms(320, 240) == {"whole"} and sc.cand_forms(2, 2) == {"tail", "no-interior"} and sc.cand_forms(3, 3) == {"tail"}
    assert [sc.sort_form(n) for n in (0, 1, 2, 4096, 4097)] == ["n0", "n1", "np<=chunk", "np<=chunk", "np>chunk"]
    assert sc.level_dims(257, 19)[1] == (129, 10) and sc.level_dims(1, 9) == [(1, 9), (1, 5), (1, 3), (1, 2), (1, 1)]
    assert len(sc.level_dims(161, 123)) == 8 and sc.level_dims(1, 1) == [(1, 1)]
    assert (1283 * 821 + 255) // 256 > sc.SCHARR_MAX_BLOCKS >= (1024 * 1024 + 255) // 256
    assert sc.scharr_forms(1283, 821) == {"grid-stride", "levels1", "levels8"} and sc.scharr_forms(17, 9) == {"one-pass", "levels1"}
    # the window rule with 21 x 21: level 1 is 21 (not built), 22 (built), 22 x 21 (not built); 3 x 3 with maxLevel 7: 7 and 8 levels
    assert [sc.track_levels(n, m, (21, 21), 3) for n, m in ((42, 42), (43, 43), (43, 41))] == [1, 2, 1]
    assert sc.track_levels(384, 384, (3, 3), 7) == 7 and sc.track_levels(385, 385, (3, 3), 7) == 8
    assert sc.track_level_forms(42, 42, (21, 21), 3) == {"1", "rule-edge-below"} == sc.track_level_forms(43, 41, (21, 21), 3)
    assert sc.track_level_forms(43, 43, (21, 21), 3) == {"rule-edge-above"}
    assert sc.track_level_forms(385, 385, (3, 3), 7) == {"8", "rule-edge-above"} and sc.track_level_forms(384, 384, (3, 3), 7) == {"rule-edge-below"}
    assert sc.track_level_forms(17, 9, (21, 21), 3) == {"1", "win>frame"}
    assert sc.track_win_forms((7, 7)) == {"npix<64"} and sc.track_win_forms((9, 9)) == {"npix%64"}
    assert sc.track_win_forms((33, 33)) == {"npix%64", "max"} and sc.track_win_forms((33, 5)) == {"npix%64", "wide"}
    assert sc.track_n_forms(65536) == {"n%4=0", "n_max"} and sc.track_n_forms(1) == {"n%4=1", "n1"}
    assert [sc.n_dev_form(m, n) for m, n in sc.N_DEV_CALLS] == ["n_dev<n", "n_dev>n", "n_dev<0", "n_dev=n"]


@pytest.mark.parametrize("f", sc.FRAMES, ids=sc.FRAME_IDS)
def test_level_dims_and_pyramid_agree_with_the_restatement(f):
    """the predicates' level sizes are pyr_down's, and lk_levels_for's count is build_pyramid's for every tracker call of the frame"""
    level = f.images()[f.kinds[0]]
    for w, h in sc.level_dims(f.W, f.H):
        assert level.shape == (h, w)
        level = lk_ref.pyr_down(level)
    c = sc.case_of(f.W, f.H)
    for t in c.tracks:
        assert sc.track_levels(c.W, c.H, t.win, t.max_level) == len(lk_ref.build_pyramid(c.frames(t)[0], t.win, t.max_level)), t.label


def test_frames_are_what_they_say():
    for f in sc.FRAMES:
        assert set(f.images()) == set(f.kinds) and all(i.shape == (f.H, f.W) and i.dtype == np.uint8 for i in f.images().values())
        if "flat" in f.kinds:
            assert len(sc.candidates("flat", f.W, f.H)[1]) == 0                        # no corner, no error
        if f.W < 3 or f.H < 3:
            assert all(len(sc.candidates(k, f.W, f.H)[1]) == 0 for k in f.kinds)       # no interior pixel, no candidate
    # one interior pixel, and it is a corner; single candidates from a frame's own map
    assert sc.candidates("rng2789", 3, 3)[1].tolist() == [4]
    assert len(sc.candidates("rng30", 5, 3)[1]) == 1 and len(sc.candidates("corner", 17, 9)[1]) == 1
    # the checkerboard: equal-valued neighbouring candidates, more than a sort chunk, below the candidate buffer and below max_corners
    v, idx = sc.candidates("checker", 161, 123)
    assert sc.has_plateau(idx, v, 161) and sc.SORT_CHUNK < len(idx) < sc.MAX_POINTS < sc.MAX_CANDIDATES
    assert len(np.unique(v)) < len(v) // 100
    assert not sc.has_plateau(*sc.candidates("noise", 161, 123)[::-1], 161)
    n = [len(sc.candidates("noise", W, H)[1]) for W, H in ((320, 240), (384, 384), (1283, 821))]
    assert 2 <= n[0] <= sc.SORT_CHUNK < n[1] < n[2] < sc.MAX_POINTS
    # the masks leave candidates in and out, and move nothing else
    for W, H in ((161, 123), (320, 240)):
        m = sc.mask_of(W, H)
        eig = sc.eigen("noise", W, H)
        kept = len(gm.masked_candidates(eig, m)[1])
        assert 0 < kept < len(sc.candidates("noise", W, H)[1]) and set(np.unique(m)) == {0, 1, 255}


@pytest.mark.parametrize("W,H,kind", [(17, 9, "blurred"), (43, 41, "noise"), (161, 123, "checker"), (320, 240, "pair0")])
def test_the_pick_model_is_lk_refs_loop(W, H, kind):
    """the GPU tests take the expected corners from gm.sequential over lk_ref's candidates: the same corners as lk_ref.good_features"""
    img = sc.image(kind, W, H)
    v, idx = sc.candidates(kind, W, H)
    keys = gm.keys_of(v, idx)
    for md in (7,) + sc.MIN_DISTANCES:
        assert np.array_equal(gm.sequential(keys, W, 2000, md), lk_ref.good_features(img, min_distance=md)), md
    all_ = np.stack([idx % W, idx // W], axis=1).astype(F)
    assert np.array_equal(gm.sequential(keys, W, sc.MAX_POINTS, 0), all_)
    assert np.array_equal(gm.good_features_masked(img, None, max_corners=sc.MAX_POINTS, min_distance=0), all_)


@pytest.mark.parametrize("W,H,win", [(1, 1, (21, 21)), (1, 9, (3, 3)), (5, 3, (21, 21)), (43, 43, (21, 21)), (257, 19, (33, 5)),
                                     (161, 123, (5, 33)), (161, 123, (33, 33)), (161, 123, (3, 3)), (1283, 821, (21, 21))])
def test_coordinate_targets_land_on_the_float_they_claim(W, H, win):
    labels, pts = sc.coord_points(W, H, win)
    assert set(labels) == sc.FORMS["track.coord"]
    hx, hy = F((win[0] - 1) * 0.5), F((win[1] - 1) * 0.5)
    px, py = pts[:, 0] - hx, pts[:, 1] - hy                      # float32, as the kernel forms them at level 0
    at = {l: i for i, l in enumerate(labels)}
    assert px[at["x=-win"]] == -win[0] and px[at["x<-win"]] == np.nextafter(F(-win[0]), F(-np.inf))
    assert px[at["x=w-1"]] == W - 1 and px[at["x=w"]] == W and np.floor(px[at["x<w"]]) == W - 1
    assert F(np.nextafter(pts[at["x<w"], 0], F(np.inf)) - hx) >= W            # the next coordinate is outside
    assert py[at["y=-win"]] == -win[1] and py[at["y<-win"]] == np.nextafter(F(-win[1]), F(-np.inf))
    assert py[at["y=h-1"]] == H - 1 and py[at["y=h"]] == H and np.floor(py[at["y<h"]]) == H - 1
    assert F(np.nextafter(pts[at["y<h"], 1], F(np.inf)) - hy) >= H
    assert np.abs(pts[[i for i, l in enumerate(labels) if l == ">=2^31"]]).max(axis=1).min() >= 2.0 ** 31
    # what the restatement decides at level 0 alone: the first bounds test is the only one these points can fail there
    a = sc.image("noise", W, H)
    _, status, exits = lk_ref.lk_track(a, a, pts, win=win, max_level=0, min_eig_threshold=0.0, want_exits=True)
    fx, fy, ok = lk_ref._floor_in(px, py, win, W, H)
    claims = sc.coord_claims(W, H, win)
    for i, l in enumerate(labels):
        assert bool(ok[i]) == (claims[l] == "in"), (l, pts[i])
        if not ok[i]:
            assert status[i] == 0, l
    assert exits[("outside-first", "0")] == int((~ok).sum())


def test_every_exit_of_the_iteration_is_taken():
    """at level 0 and at a coarser level, by the baseline case's calls; every (point, level) visit leaves by exactly one exit"""
    c = sc.case_of(320, 240)
    total = {}
    for i, t in enumerate(c.tracks):
        pts, out, status, hist, exits = sc.reference(c.name, i)
        levels = sc.track_levels(c.W, c.H, t.win, t.max_level)
        assert sum(v for (e, g), v in exits.items() if g == "0") == len(pts), t.label
        assert sum(exits.values()) == len(pts) * levels, t.label
        assert hist.sum() == sum(v for (e, g), v in exits.items() if e not in ("outside-first", "min-eig")), t.label
        for k, v in exits.items():
            total[k] = total.get(k, 0) + v
        print(t.label, {f"{e}:{g}": v for (e, g), v in exits.items() if v})
    assert set(total) == {(e, g) for e in lk_ref.EXITS for g in ("0", "coarser")}
    assert all(v > 0 for v in total.values()), sorted(k for k, v in total.items() if not v)
    # the histogram's ends: 40 px of motion runs into maxCount, a count of 0 leaves everything in bin 0
    far = next(i for i, t in enumerate(c.tracks) if t.moved == "far" and t.max_level == 3)
    assert sc.reference(c.name, far)[3][30] > 0


def test_exits_leave_the_arithmetic_alone():
    c = sc.case_of(43, 43)
    t = c.tracks[0]
    a, b = c.frames(t)
    pts = c.points(t)
    plain = lk_ref.lk_track(a, b, pts, want_hist=True, **t.params())
    booked = lk_ref.lk_track(a, b, pts, want_hist=True, want_exits=True, **t.params())
    assert len(booked) == 4 and all(x.tobytes() == y.tobytes() for x, y in zip(plain, booked[:3]))
    assert len(lk_ref.lk_track(a, b, pts, want_exits=True)) == 3


@pytest.mark.parametrize("c", sc.CASES, ids=sc.CASE_IDS)
def test_tracker_cases_track(c):
    """On a frame of at least 43 x 43 at least half of the points placed inside the frame end with status 1; on every frame the points
    outside it, the NaNs and the infinities end with status 0."""
    for i, t in enumerate(c.tracks):
        t0 = time.perf_counter()
        pts, out, status, hist, exits = sc.reference(c.name, i)
        dt = time.perf_counter() - t0
        k = c.n_inside(t)
        inside = pts[:k]
        big = min(c.W, c.H) >= sc.MIN_TRACKED_SIDE          # (on a frame of a few pixels border_points' half-pixel offsets leave the frame)
        assert not big or (np.all(inside >= 0) and np.all(inside[:, 0] <= c.W - 1) and np.all(inside[:, 1] <= c.H - 1)), t.label
        print(f"{c.name} {t.label}: {len(pts)} points, {int(status[:k].sum())} of {k} inside tracked, reference {dt:.2f} s")
        if big and k:
            assert 2 * int(status[:k].sum()) >= k, (t.label, int(status[:k].sum()), k)
        if t.points == "mixed":
            assert np.all(status[-5:] == 0) and len(pts) == k + 15
        assert len(pts) <= sc.MAX_POINTS and np.isfinite(out[status == 1]).all()
