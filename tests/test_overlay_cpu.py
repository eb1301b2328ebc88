"""CPU pins of the processed.mp4 frame (tests/overlay_ref.py): the blend is exact in integers, the disc's span table, its shape and
clipping, the centre's truncation and guards -- and FocusOfExpansion.draw_FoE / im_helpers.add_weighted against them."""
import numpy as np
import pytest

import overlay_ref as ov


def _fma32(x, y, z):
    """float32 fma(x, y, z): x * y + z is exact in float64 for u8 x and float32 y, z of this size (at most 34 significant bits)."""
    return (x.astype(np.float64) * np.float64(y) + np.asarray(z, np.float32).astype(np.float64)).astype(np.float32)


def test_blend_is_exact_for_every_byte_pair():
    p, q = (a.ravel() for a in np.meshgrid(np.arange(256), np.arange(256), indexing="ij"))
    want = (p + 4 * q + 2) // 5
    pf, qf = p.astype(np.float32), q.astype(np.float32)
    a, b, g = np.float32(0.2), np.float32(1.0 - 0.2), np.float32(0.0)
    forms = [(pf * a + qf * b) + g, (qf * b + pf * a) + g, pf * a + (qf * b + g),       # separate multiply-add, any order
             _fma32(pf, a, qf * b), _fma32(qf, b, pf * a), _fma32(pf, a, _fma32(qf, b, g))]  # fused
    for t in forms:
        assert t.dtype == np.float32
        assert np.array_equal(np.rint(t).astype(np.int64), want)
        t64 = t.astype(np.float64)
        assert np.abs(t64 - np.floor(t64) - 0.5).min() > 0.09           # fractions .4 and .6 are the nearest to a tie
    assert np.array_equal(ov.blend(p.astype(np.uint8), q.astype(np.uint8)), want)
    assert np.array_equal(ov.blend(p.astype(np.uint8), p.astype(np.uint8)), p)       # outside the mask the byte is p
    from mavflow import im_helpers
    assert np.array_equal(im_helpers.add_weighted(p.astype(np.uint8), 0.2, q.astype(np.uint8), 1.0 - 0.2, 0.0), want)


def test_r10_table():
    assert ov.HALF_WIDTHS_R10 == (10, 9, 9, 9, 9, 8, 8, 7, 6, 4, 0)
    assert tuple(ov.half_widths(10)) == ov.HALF_WIDTHS_R10
    assert int(ov.disc(41, 41, 20, 20, 10).sum()) == 317
    from mavflow.focus_of_expansion import disc_half_widths
    for r in range(0, 64):
        assert disc_half_widths(r) == ov.half_widths(r), r
    assert ov.half_widths(0) == [0] and ov.half_widths(1) == [1, 0]


@pytest.mark.parametrize("r", [0, 1, 2, 3, 5, 10, 17, 40])
def test_disc_is_symmetric_under_both_reflections(r):
    d = ov.disc(2 * r + 5, 2 * r + 5, r + 2, r + 2, r)
    assert np.array_equal(d, d[::-1]) and np.array_equal(d, d[:, ::-1])
    rows = d.sum(axis=1)
    assert (np.diff(rows[: r + 3]) >= 0).all()                         # widths grow toward the centre row


def test_r10_disc_lies_between_the_euclidean_discs():
    d = ov.disc(41, 41, 20, 20, 10)
    yy, xx = np.mgrid[0:41, 0:41]
    dist = np.hypot(xx - 20, yy - 20)
    assert d[dist <= 9.5].all()
    assert (dist[d] <= 10.5).all()


def test_clipped_disc_is_the_full_disc_inside_the_image():
    W, H, r, pad = 23, 17, 10, 40
    centres = set()
    for off in range(0, 12):
        for cy in (-off, H // 2, H - 1 + off):
            for cx in (-off, W // 2, W - 1 + off):
                centres.add((cx, cy))
    for cx, cy in sorted(centres):
        full = ov.disc(H + 2 * pad, W + 2 * pad, cx + pad, cy + pad, r)[pad:pad + H, pad:pad + W]
        assert np.array_equal(ov.disc(H, W, cx, cy, r), full), (cx, cy)
    assert ov.disc(H, W, -10, H // 2, r).any() and not ov.disc(H, W, -11, H // 2, r).any()
    assert ov.disc(H, W, W // 2, H - 1 + 10, r).any() and not ov.disc(H, W, W // 2, H - 1 + 11, r).any()


def test_centre_truncates_toward_zero():
    assert ov.centre((-0.7, 5.9)) == (0, 5)
    assert ov.centre((-1.2, -0.999)) == (-1, 0)
    assert np.array_equal(ov.disc_of(30, 30, (-0.7, 12.5)), ov.disc(30, 30, 0, 12, 10))
    assert not np.array_equal(ov.disc_of(30, 30, (-0.7, 12.5)), ov.disc(30, 30, -1, 12, 10))


def test_guards():
    assert ov.centre((1e9, -1e9)) == (10 ** 9, -10 ** 9)
    for foe in ((1e9 + 1, 0.0), (0.0, -1e9 - 1), (np.inf, 0.0), (np.nan, 0.0), (0.0, np.nan)):
        assert ov.centre(foe) is None, foe
    for foe in ((float("nan"), 0.0), (0.0, np.float64("nan"))):
        with pytest.raises(ValueError):
            ov.centre(foe)
    # the binding maps the np.nan object to "not drawn" and hands any other NaN on (the library refuses it)
    from mavflow import _lib
    got = _lib.Context._foes([(np.nan, 3.0), (float("nan"), 1e9 + 1)], 2, "foe")
    assert np.isinf(got[0, 0]) and got[0, 1] == 3.0 and np.isnan(got[1, 0]) and got[1, 1] == 1e9 + 1
    assert _lib.Context._foes((1.5, 2.5), 1, "foe").tolist() == [[1.5, 2.5]]
    with pytest.raises(ValueError):
        _lib.Context._foes([(1.0, 2.0)], 2, "foe")


def test_draw_order_flag_and_paint():
    H, W = 40, 50
    frame = np.arange(H * W * 3, dtype=np.uint32).reshape(H, W, 3).astype(np.uint8)
    keep = frame.copy()
    mask = np.zeros((H, W), bool)
    out, written = ov.overlay(frame, mask, (20.0, 20.0), (24.0, 20.0))
    assert np.array_equal(frame, keep) and written
    g, w = ov.disc_of(H, W, (20.0, 20.0)), ov.disc_of(H, W, (24.0, 20.0))
    assert (out[w] == 255).all()                                       # white over green, unblended outside the mask
    assert (out[g & ~w] == ov.GREEN).all()
    assert np.array_equal(out[~g & ~w], frame[~g & ~w])
    mask[0, 0] = mask[20, 20] = True
    out, written = ov.overlay(frame, mask, (20.0, 20.0), (24.0, 20.0))
    assert tuple(out[0, 0]) == tuple((np.array(frame[0, 0], int) + 4 * np.array(ov.PURPLE) + 2) // 5)
    assert tuple(out[20, 20]) == tuple((255 + 4 * np.array(ov.PURPLE) + 2) // 5)
    assert not ov.overlay(frame, np.zeros((H, W), bool), (-11.0, 5.0), (5.0, H + 10.0))[1]
    assert ov.overlay(frame, np.zeros((H, W), bool), (-10.0, 5.0), (np.nan, 0.0))[1]
    assert ov.overlay(frame, mask, (1e9 + 1, 0.0), (np.nan, np.nan))[1]


class _LK:
    total_num_corners = 4
    old_frame = np.zeros((8, 8), np.uint8)


def test_draw_foe_matches_the_restatement():
    from mavflow.focus_of_expansion import FocusOfExpansion
    fo = FocusOfExpansion(_LK())
    rng = np.random.default_rng(1)
    H, W = 37, 53
    for r in (0, 1, 4, 10, 23):
        for foe in [(-0.7, 3.2), (-11.0, 5.0), (W + 3.5, H - 1.0), (26.3, 18.9), (1e9, 5.0), (1e9 + 1, 5.0), (np.nan, 2.0),
                    tuple(rng.uniform(-15, 70, 2))]:
            frame = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
            want = ov.draw(frame.copy(), foe, [0, 255, 0], r)
            got = fo.draw_FoE(frame, foe, [0, 255, 0], r)
            assert got is frame and np.array_equal(got, want), (r, foe)
    frame = np.zeros((H, W, 3), np.uint8)
    assert np.array_equal(fo.draw_FoE(frame, (10.0, 10.0)), ov.draw(np.zeros((H, W, 3), np.uint8), (10.0, 10.0), [0, 42, 255]))
    with pytest.raises(ValueError):
        fo.draw_FoE(frame, (float("nan"), 1.0))
    gray = np.zeros((H, W), np.uint8)
    fo.draw_FoE(gray, (5.0, 5.0), [200, 0, 0], 3)
    assert np.array_equal(gray > 0, ov.disc(H, W, 5, 5, 3)) and gray.max() == 200
