"""The window search's case table (tests/window_cases.py) is what it claims to be -- checked from the predicates and the numpy oracle
(oracle/pyramid_oracle.py) alone, without a GPU: every kernel form is reached, every image is what its name says, and no walk of
optimize_window comes near the kernel's step cap."""
import numpy as np
import pytest

import window_cases as wc
from oracle import pyramid_oracle as po

UNIFORM = (3 * 64 * 64 * 255, 0, 0, 0, 0, 0)


def test_every_form_is_reached():
    reached = {g: set() for g in wc.FORMS}
    for c in wc.CASES:
        got = wc.case_forms(c)
        names = {f for _, f in got}
        assert c.expects <= names, (c.name, sorted(c.expects - names))
        for g, f in got:
            reached[g].add(f)
    for g, forms in wc.FORMS.items():
        assert forms <= reached[g], (g, sorted(forms - reached[g]))
        assert reached[g] <= forms | wc.UNTESTED.get(g, set()), (g, sorted(reached[g] - forms))
        assert not (wc.UNTESTED.get(g, set()) & reached[g])
    assert set(wc.UNTESTED) <= set(wc.FORMS)


def test_predicates_at_the_shapes_they_were_chosen_for():
    """the launchers' arithmetic at the table's shapes, spelled out: a changed constant in kernels_window.hip must change these too"""
    assert [wc.windows_of(w, h) for w, h in ((63, 100), (64, 64), (80, 64), (4176, 100), (2784, 66))] == [(0, 3), (1, 1), (2, 1), (258, 3), (171, 1)]
    assert [wc.scan_form(w, h) for w, h in ((63, 100), (64, 64), (80, 64), (4176, 100), (2784, 66))] == ["none", "one", "nwx<=256", "nwx>256", "nwx<=256"]
    assert po.pyramid_dims(96, 96)[:2] == [(96, 96), (64, 64)] and po.pyramid_dims(70, 1) == [(70, 1)]
    assert po.pyramid_dims(4176, 100)[:2] == [(4176, 100), (2784, 66)]
    # scale 1.5 exactly: even destination indices start on a cell boundary, odd ones end on one
    forms = wc.area_forms(96, 64)
    assert forms == {("area.scale", "1.5"), ("area.first", "first"), ("area.first", "no-first"), ("area.last", "last"), ("area.last", "no-last"),
                     ("area.clamp", "clamp")}                                       # the last index: floor(f2) = ssize
    assert ("area.scale", "other") in wc.area_forms(97, 64) and ("area.clamp", "clamp") in wc.area_forms(97, 64) | wc.area_forms(146, 96)
    assert wc.sat_forms(100, 70) == {"w<256"} and wc.sat_forms(512, 70) == {"w=k*256"} and wc.sat_forms(1000, 70) == {"w%256"}
    assert wc.sat_forms(70, 1) == {"w<256", "h1"} and wc.step_cap(1000, 70) == 4344


@pytest.mark.parametrize("ssize,dsize", [(96, 64), (97, 64), (146, 96), (333, 222), (217, 144), (4176, 2784), (100, 66)])
def test_area_spans_are_the_oracles_table(ssize, dsize):
    """the predicate's cells -- an optional partial first one, whole ones, an optional partial last one -- are the source indices that
    computeResizeAreaTab's restatement lists for every destination index, in its order"""
    tab = po.area_tab(ssize, dsize, 1.0 / (dsize / ssize))
    per = {}
    for di, si, a in tab:
        per.setdefault(di, []).append(si)
    spans = wc.area_spans(ssize, dsize)
    assert len(per) == dsize == len(spans)
    for d, (s1, s2, first, last, clamped) in enumerate(spans):
        assert per[d] == ([s1 - 1] if first else []) + list(range(s1, s2)) + ([s2] if last else []), d
        assert 0 <= per[d][0] and per[d][-1] <= ssize - 1
    assert abs(sum(float(a) for _, _, a in tab) - dsize) < 1e-3 * dsize       # every destination's weights sum to 1


def test_images_are_what_they_say():
    for c in wc.CASES:
        assert c.dims() == [(l.shape[1], l.shape[0]) for l in wc.levels(c.kinds[0], c.W, c.H)]
        for kind in c.kinds:
            best, n_levels, n_windows, n_pixels = wc.analysis(kind, c.W, c.H)
            has_window = any(wc.scan_form(w, h) != "none" for w, h in c.dims())
            if kind == "uniform" and has_window:
                assert best == UNIFORM and n_pixels == 64 * 64, (c.name, best)        # every window of every level ties
                assert n_windows == wc.windows_of(c.W, c.H)[0] * wc.windows_of(c.W, c.H)[1]
            if kind == "zero" or not has_window:
                assert best == (0,) * 6
            if kind == "band" and c.W >= 32 + 64:
                # the first window clear of the band wins, the windows behind it tie with it
                assert best[:4] == (UNIFORM[0], 32, 0, 0) and wc.BAND % wc.STEP and (n_windows > 1 or c.W < 32 + 64 + 16)
            elif kind == "band":
                assert 0 < best[0] < UNIFORM[0]
            if kind == "right":
                # the last window of the first row, level 0: beyond the first 256 windows of k_level_scan's loop
                assert best[1:4] == (c.W - 64 - (c.W - 64) % 16, 0, 0) and best[1] // 16 >= 256 and n_windows == wc.windows_of(c.W, c.H)[1]
                assert wc.window_max_reference(kind, c.W, c.H) == best[:3]
            if kind == "dots":
                assert best[3] == 1 and c.kinds.index(kind) > 0                        # a coarser level wins, in a pair b > 0
                lv1 = wc.levels(kind, c.W, c.H)[1]
                x, y = best[1:3]
                assert lv1[y:y + 64, x:x + 64].sum() == lv1.sum()                      # the level-1 window holds all four dots
                assert wc.window_max_reference(kind, c.W, c.H)[0] < best[0]
    # uniform levels stay uniform: the tie across levels is exact
    assert all((l == 255).all() for l in wc.levels("uniform", 97, 146))
    assert wc.analysis("uniform", 96, 96)[1] == 2 and wc.analysis("uniform", 4176, 100)[1] == 2


@pytest.mark.parametrize("c", [c for c in wc.CASES if c.opt], ids=[c.name for c in wc.CASES if c.opt])
def test_walks_are_the_oracles_and_stay_below_the_cap(c):
    """walk() is po.optimize_window with a step count; every case stays below k_optimize_window's cap 4 (W + H) + 64, the long walks
    exceed min(W, H) steps, the windows outside the image and on a zero image take none"""
    longest = 0
    for kind, start in wc.opt_pairs(c):
        score, win, steps, events = wc.opt_reference(kind, c.W, c.H, start)
        assert (score, win) == po.optimize_window(wc.image(kind, c.W, c.H), wc.start_windows(c.W, c.H)[start]), (kind, start)
        assert steps < wc.step_cap(c.W, c.H) // 2, (kind, start, steps)
        if start == "outside" or kind in ("zero", "dots"):
            assert steps == 0 and score == 0 and win == wc.start_windows(c.W, c.H)[start]
        if start == "empty" and kind not in ("zero", "dots"):
            assert steps > 0 and score > 0
        longest = max(longest, steps)
        print(f"{c.name} {kind} {start}: {steps} steps of {wc.step_cap(c.W, c.H)}, score {score}, window {win}, {sorted(events)}")
    if "long-walk" in c.expects:
        assert longest > min(c.W, c.H) and longest == max(c.W, c.H) - 1
        assert wc.opt_reference("uniform", c.W, c.H, "corner")[0] == 3 * 255 * c.W * c.H        # the whole frame
