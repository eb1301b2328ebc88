"""tests/shapes_ref.py and tests/shapes_cases.py held to conditions of their own, without a GPU: the restatement against independent
statements of the same shapes (vis_ref's pixel-by-pixel line, the project's disc spans, a numpy slice, a geometric band for the thick
line), and the case table against the forms and situations it has to reach."""
import numpy as np
import pytest

import shapes_cases as sc
import shapes_ref as R
import vis_ref


def thin_by_iterator(W, H, s):
    m = np.zeros((H, W), bool)
    ok, q1, q2 = vis_ref.clip_line(W, H, (int(s["x0"]), int(s["y0"])), (int(s["x1"]), int(s["y1"])))
    if ok:
        for x, y in vis_ref.line_pixels(q1, q2):
            m[y, x] = True
    return m


def test_thickness_1_lines_equal_the_line_iterator():
    n = 0
    for c in sc.CASES:
        for s in c.shapes:
            if R.valid(s, sc.B) and int(s["kind"]) == R.LINE and int(s["thickness"]) == 1:
                assert np.array_equal(R.record_mask(s, c.W, c.H), thin_by_iterator(c.W, c.H, s)), (sc.case_id(c), s)
                n += 1
    rng = np.random.RandomState(1)
    for W, H in sc.FRAMES:
        for _ in range(1500):
            x0, x1 = rng.randint(-W, 2 * W, 2)
            y0, y1 = rng.randint(-H, 2 * H, 2)
            s = R.table([R.shape(R.LINE, 0, x0, y0, x1, y1, 1, sc.GREEN)])[0]
            assert np.array_equal(R.record_mask(s, W, H), thin_by_iterator(W, H, s)), s
            n += 1
    assert n > 3000


def test_filled_circles_equal_the_disc_spans():
    from mavflow.focus_of_expansion import disc_half_widths
    for r in list(range(0, 40)) + [128, 300]:
        assert R.disc_half_widths(r) == disc_half_widths(r)
    W, H = sc.FRAMES[0]
    for s in R.table(sc.circles(W, H)):
        want = np.zeros((H, W), bool)
        cx, cy, r = int(s["x0"]), int(s["y0"]), int(s["x1"])
        for k, h in enumerate(disc_half_widths(r)):
            for y in {cy - k, cy + k}:
                x0, x1 = max(cx - h, 0), min(cx + h, W - 1)
                if 0 <= y < H and x0 <= x1:
                    want[y, x0:x1 + 1] = True
        assert np.array_equal(R.record_mask(s, W, H), want), s


def test_the_disc_walk_has_a_closed_form():
    """what the device evaluates: h[k] = floor(sqrt(R^2 - k^2)), no row left empty"""
    import math
    for r in list(range(0, 400)) + [1000, 4096, 300000, 1 << 20]:
        h = R.disc_half_widths(r)
        assert h == [math.isqrt(r * r - k * k) for k in range(r + 1)], r


def test_filled_rectangle_is_a_slice_and_corners_may_be_exchanged():
    for W, H in sc.FRAMES:
        for s in R.table(sc.rectangles(W, H)):
            x0, y0, x1, y1 = (int(s[k]) for k in ("x0", "y0", "x1", "y1"))
            got = R.record_mask(s, W, H)
            if int(s["thickness"]) == R.FILLED:
                want = np.zeros((H, W), bool)
                want[max(min(y0, y1), 0):max(max(y0, y1) + 1, 0), max(min(x0, x1), 0):max(max(x0, x1) + 1, 0)] = True
                assert np.array_equal(got, want), s
            for a, b, c, d in ((x1, y1, x0, y0), (x0, y1, x1, y0), (x1, y0, x0, y1)):
                t = s.copy()
                t["x0"], t["y0"], t["x1"], t["y1"] = a, b, c, d
                assert np.array_equal(R.record_mask(t, W, H), got), (s, t)


@pytest.mark.parametrize("case", sc.CASES, ids=sc.case_id)
def test_the_restatement_meets_the_band_on_every_case(case):
    recs = sc.banded_records(case)
    must_sets = 0
    for s in recs:
        got = R.record_mask(s, case.W, case.H)
        must, may_not = sc.band_of(s, case.W, case.H)
        assert not (must & ~got).any(), ("a pixel within t / 2 - 1 is not drawn", s, np.argwhere(must & ~got)[:5])
        assert not (may_not & got).any(), ("a pixel beyond t / 2 + 1.5 is drawn", s, np.argwhere(may_not & got)[:5])
        must_sets += bool(must.any())
    if any(int(s["thickness"]) >= 3 for s in recs):
        assert must_sets > 0, "a case with thick lines whose must-draw set is empty shows nothing"


def test_thickness_2_is_three_pixels_wide_and_3_is_five():
    W, H = 66, 33
    for t, wide in ((2, 3), (3, 5), (4, 5), (5, 7)):
        m = R.record_mask(R.table([R.shape(R.LINE, 0, 10, 16, 50, 16, t, sc.GREEN)])[0], W, H)
        assert m[:, 30].sum() == wide, (t, m[:, 30].sum())
        m = R.record_mask(R.table([R.shape(R.LINE, 0, 30, 5, 30, 28, t, sc.GREEN)])[0], W, H)
        assert m[16, :].sum() == wide, (t, m[16, :].sum())


def test_order_decides_thousands_of_pixels_of_the_heavy_overlap_case():
    case = [c for c in sc.CASES if c.name == "heavy-overlap"][0]
    img = sc.canary(case.W, case.H, 3)
    fwd, rev = R.draw_shapes(img, case.shapes), R.draw_shapes(img, case.shapes[::-1].copy())
    assert (fwd != rev).any(axis=-1).sum() >= 2000
    own, cnt = R.owner_plane(case.shapes, sc.B, case.H, case.W)
    assert (cnt[0] > 5).sum() > 2000 and (own[1] == 0).all()


def test_add_and_mosaic_restatements():
    for c in sc.ADD_CASES:
        a, b = sc.add_inputs(c)
        s = R.add_saturate(a, b)
        assert np.array_equal(s, np.minimum(a.astype(np.uint16) + b, 255)) and s.dtype == np.uint8
        assert s.reshape(-1)[:4].tolist() == [255, 255, 0, 255]
    for c in sc.MOSAIC_CASES:
        tiles = sc.mosaic_inputs(c)
        m = R.mosaic(tiles, c.rows, c.cols, c.batch, c.H, c.W)
        assert m.shape == (c.batch, c.rows * c.H, c.cols * c.W, 3)
        for i, t in enumerate(tiles):
            r, q = divmod(i, c.cols)
            part = m[:, r * c.H:(r + 1) * c.H, q * c.W:(q + 1) * c.W]
            want = np.zeros_like(part) if t is None else np.broadcast_to(t, part.shape)
            assert np.array_equal(part, want)


def test_every_form_and_situation_is_reached(mav):
    from mavflow import shapes
    forms = {(sc.one_colour(c.shapes, c.channels), c.channels) for c in sc.CASES}
    assert forms == {(True, 1), (True, 3), (False, 1), (False, 3)}               # direct and ordered, 1 and 3 channels
    for c in sc.CASES:                                                          # ... as the library itself chooses
        assert shapes.shapes_form(c.shapes, c.channels) == (shapes.FORM_DIRECT if sc.one_colour(c.shapes, c.channels) else shapes.FORM_ORDERED)
    add = {sc.bytes_form_of(c.W * c.H * c.channels * c.batch, c.offset, c.offset, c.offset) for c in sc.ADD_CASES}
    mos = {sc.bytes_form_of(c.W * c.H * 3 * c.batch * c.rows * c.cols, c.offset) for c in sc.MOSAIC_CASES}
    assert add == {0, 1} and mos == {0, 1}
    base = 1 << 20
    for c in sc.ADD_CASES:
        n = c.W * c.H * c.channels * c.batch
        assert shapes.bytes_form(n, base + c.offset, base + c.offset, base + c.offset) == sc.bytes_form_of(n, c.offset, c.offset, c.offset)
    assert shapes.bytes_form(15, base, base, base) == shapes.FORM_BYTES and shapes.bytes_form(16, base, base, base) == shapes.FORM_WORDS
    assert shapes.bytes_form(64, base, base + 8, base) == shapes.FORM_BYTES and shapes.bytes_form(0, base) == -1
    assert {int(t) for c in sc.CASES for t in c.shapes["thickness"] if 1 <= t <= 255} >= set(sc.THICKNESSES)
    kinds = {int(k) for c in sc.CASES for k in c.shapes["kind"]}
    assert kinds >= {R.LINE, R.RECT, R.CIRCLE}
    assert not any(sc.uses_image_1(c) for c in sc.CASES)                         # image 1 stays untouched in every case
    bad = sc.skipped_records(*sc.FRAMES[0])
    t = R.table(bad[0])
    assert sum(not R.valid(s, sc.B) for s in t) == bad[1] and sum(R.valid(s, sc.B) for s in t) == bad[1] + 2
    assert (np.dtype(shapes.SHAPE_DTYPE) == R.SHAPE_DTYPE) and shapes.scratch_bytes(131, 67, 3) == 4 * 131 * 67 * 3


# ---- past the caps of the launches ---------------------------------------------------------------------------------------------------------
def test_the_cap_cases_sit_just_past_the_caps_the_source_defines():
    c = sc.source_caps()
    W, H = sc.RESOLVE_FRAME
    N, thr = W * H * sc.B, c["resolve"] * c["wg"]
    # the frame 701 x 499 x 3 is 821 elements past the cap, more than the 2 * SH_WG the other frames are held to: the bound here is
    # 4 * SH_WG, and fewer than two rows of the last image
    assert 0 < N - thr <= 4 * c["wg"] and N - thr < 2 * W, ("RESOLVE_FRAME", sc.RESOLVE_FRAME, "is not just past the resolve cap * SH_WG =", thr)
    assert ">1:partial-last" in sc.resolve_forms(W, H, sc.B, c), "RESOLVE_FRAME does not reach the form >1:partial-last"
    assert 0 < sc.ROWS_N_DEV - c["rows"] < sc.ROWS_RECORDS - c["rows"] <= c["wg"], ("ROWS_RECORDS / ROWS_N_DEV", sc.ROWS_RECORDS, sc.ROWS_N_DEV, "against the rows cap", c["rows"])
    assert ">1:partial-last" in sc.rows_forms(sc.ROWS_RECORDS, c) and ">1:partial-last" in sc.rows_forms(sc.ROWS_N_DEV, c), "ROWS_RECORDS does not reach the form >1:partial-last"
    assert sc.rows_forms(c["rows"], c) == {"1"} and sc.rows_forms(c["rows"] + 1, c) == {">1", ">1:partial-last"} and sc.rows_forms(2 * c["rows"], c) == {">1"}
    # the loops the caps bound, read as text
    assert "stride = (unsigned long long)gridDim.x * SH_WAVES" in c["text"] and "stride = (size_t)gridDim.x * SH_WG" in c["text"]
    assert "#define SH_WAVES (SH_WG / 64)" in c["text"]
    # without these no case reaches a second trip of either loop
    for case in sc.CASES:
        assert sc.resolve_forms(case.W, case.H, sc.B, c) == {"1"} and sc.rows_forms(len(case.shapes), c) == {"1"}, sc.case_id(case)


def test_order_decides_pixels_past_the_resolve_cap():
    c = sc.source_caps()
    W, H = sc.RESOLVE_FRAME
    thr = c["resolve"] * c["wg"]
    t = sc.resolve_cap_table(W, H)
    assert 75 <= len(t) <= 90 and {int(i) for i in t["image"]} == {0, 1, 2} and not sc.one_colour(t, 3) and not sc.one_colour(t, 1)
    assert all(R.valid(s, sc.B) for s in t)
    own, cnt = R.owner_plane(t, sc.B, H, W)
    o = own.ravel()[thr:]
    owners = set(np.unique(o[o > 0]).tolist())
    assert (o > 0).sum() >= 200 and len(owners) >= 3 and (o == 0).any()
    assert len({tuple(t["colour"][i - 1]) for i in owners}) >= 3                          # of different colours
    kinds = {(int(t["kind"][i - 1]), int(t["thickness"][i - 1]) == R.FILLED) for i in owners}
    assert (R.RECT, True) in kinds and (R.CIRCLE, True) in kinds and any(k == R.LINE for k, _ in kinds)
    # a lower-numbered record beneath the owner, from the records' own masks
    beneath = np.zeros(W * H * sc.B - thr, bool)
    for i, s in enumerate(t):
        if int(s["image"]) == 2:
            m = np.zeros((sc.B, H, W), bool)
            m[2] = R.record_mask(s, W, H)
            beneath |= m.ravel()[thr:] & (o > i + 1)
    assert beneath.sum() >= 100 and (cnt.ravel()[thr:] > 2).any()
    assert (own[0] > 0).any() and (own[1] > 0).any()


def test_the_records_past_the_rows_cap_own_pixels_over_earlier_records():
    c = sc.source_caps()
    W, H = sc.FRAMES[0]
    t = sc.rows_cap_table(W, H)
    assert len(t) == sc.ROWS_RECORDS and not sc.one_colour(t, 3) and sc.one_colour(sc.rows_cap_table(W, H, green=True), 3)
    own, cnt = R.owner_plane(t, sc.B, H, W)
    late = own >= c["rows"] + 1                                                           # owner index + 1 of a record i >= 8192
    assert late.sum() >= 100 and (late & (cnt > 1)).sum() >= 1
    # (the owner is the last record that reaches a pixel: where more than one does, the others are earlier records' masks)
    assert (own[0] > sc.ROWS_N_DEV).any() and ((own[0] > c["rows"]) & (own[0] <= sc.ROWS_N_DEV)).any()     # either side of the device count
