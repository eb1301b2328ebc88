"""The two forms of the polynomial-expansion tile (kernels_flow.hip: polyexp_tile, the relaxed form for any width and alignment, and
polyexp_tile_fast, the aligned form for widths that are a multiple of 4 at poly_n 8, 7 and 5) give the same bits.

  * Fast against relaxed: a layer of width w, w % 4 == 0, takes the fast form; the same image in a context of width w + 1 whose extra
    column repeats column w - 1 takes the relaxed one.  The expansion replicates its borders, so columns 0 .. w - 1 of the wider
    result are the narrower result, value for value.
  * The forms this change leaves alone (poly_n 6: polyexp<0>; a width that is no multiple of 4) against CRCs of the build before the
    fast form existed (tests/golden/polyexp_forms_crc.json).
  * k_polyexp_multi takes the same tile code: a 3-layer pyramid expanded by one launch (batch 1) and layer by layer (batch 3) gives
    (with the small-group schedule switched off: 200 x 200 is small enough to take the one launch at batch 3 too) gives the same flow.

The inputs are float32 noise (no multiples of 1/16: every product rounds), from an integer hash, so that they do not depend on the
version of numpy's generators."""
import json
import os
import zlib
from collections import Counter

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "polyexp_forms_crc.json")
POLY_SIGMA = {8: 1.7, 7: 1.5, 6: 1.3, 5: 1.1}
# 8x2: less than one quad-row of halo inside the image; 64x16: exactly one tile; 68x18: one tile + a 4-pixel column of tiles and 2 rows;
# 132x35: interior, left-edge and 4-pixel-wide right-edge tiles, ragged tile rows; 4x33: one quad wide, three tile rows
SHAPES = [(8, 2), (64, 16), (68, 18), (132, 35), (4, 33)]
# the forms left alone: (w, h, poly_n)
OTHER_FORMS = [(68, 18, 6), (67, 18, 8)]


def noise(w, h, seed):
    """(h, w) float32 in [0, 255), a fixed function of (w, h, seed)"""
    i = np.arange(w * h, dtype=np.uint64) + np.uint64(seed) * np.uint64(0x9E3779B9)
    x = (i * np.uint64(0x9E3779B97F4A7C15)) & np.uint64(0xFFFFFFFFFFFFFFFF)
    x ^= x >> np.uint64(29)
    x = (x * np.uint64(0xBF58476D1CE4E5B9)) & np.uint64(0xFFFFFFFFFFFFFFFF)
    x ^= x >> np.uint64(32)
    u = (x & np.uint64(0xFFFFFF)).astype(np.float32)            # 24 bits: exact in float32
    return (u * np.float32(255.0 / (1 << 24))).reshape(h, w)


def expansion(w, h, n, I):
    from mavflow import _lib
    fb = _lib.fb_defaults(levels=1)
    fb.poly_n, fb.poly_sigma = n, POLY_SIGMA[n]
    with _lib.Context(w, h, 1, fb) as ctx:
        assert ctx.num_layers() == 1 and ctx.layer_dims(0)[:2] == (w, h)
        return ctx.stage_polyexp(I, 0).copy()


def other_form_crcs():
    """CRC-32 of the (5, h, w) float32 result of every OTHER_FORMS case (tests/golden/polyexp_forms_crc.json holds the parent build's)"""
    return {f"{w}x{h}-n{n}": "%08x" % zlib.crc32(expansion(w, h, n, noise(w, h, 100 + n)).tobytes()) for w, h, n in OTHER_FORMS}


@pytest.mark.parametrize("n", [8, 7, 5])
@pytest.mark.parametrize("w,h", SHAPES, ids=[f"{w}x{h}" for w, h in SHAPES])
def test_fast_form_equals_relaxed_form(mav, w, h, n):
    assert w % 4 == 0
    I = noise(w, h, n)
    fast = expansion(w, h, n, I)
    relaxed = expansion(w + 1, h, n, np.concatenate([I, I[:, -1:]], axis=1))[:, :, :w]
    assert np.isfinite(fast).all() and np.abs(fast).max() > 0
    if not np.array_equal(fast, relaxed):
        bad = (fast != relaxed).any(axis=0)
        y, x = (int(v) for v in np.argwhere(bad)[0])
        pytest.fail(f"{w}x{h} poly_n {n}: {int(bad.sum())} of {bad.size} pixels differ, first at (y, x) = ({y}, {x}): "
                    f"{fast[:, y, x].tolist()} vs {relaxed[:, y, x].tolist()}")


def test_other_forms_unchanged(mav):
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert other_form_crcs() == golden


def test_multi_launch_takes_the_same_code(mav):
    from mavflow import _lib, synth
    W = H = 200
    prev, nxt, _ = synth.make_pair(W, H, 3)
    flows, launches = {}, {}
    for B in (1, 3):
        fb = _lib.fb_defaults(levels=3)
        with _lib.Context(W, H, B, fb) as ctx:
            assert [ctx.layer_dims(k)[0] for k in range(ctx.num_layers())] == [200, 80, 32]
            if B == 3:
                ctx.set_option("small_batch", 0)         # a frame this small would take the one-launch pyramid at batch 3 as well
            p, q = np.repeat(prev[None], B, axis=0), np.repeat(nxt[None], B, axis=0)
            ctx.profile_enable(1)
            flows[B] = ctx.farneback(p, q).copy()
            kid, _, _, _ = ctx.profile_intervals()
            names = list(ctx.profile_get())
            launches[B] = Counter(names[k] for k in kid)["polyexp"]
            ctx.profile_enable(0)
    assert launches[1] == 1 and launches[3] >= 3, launches          # the whole pyramid in one launch / per-layer launches
    assert np.isfinite(flows[1]).all() and np.abs(flows[1]).max() > 0
    for b in range(3):
        assert flows[3][b].tobytes() == flows[1][0].tobytes(), b
