"""The detection case table (tests/detect_cases.py) is what it claims to be -- checked from the predicates and the numpy oracle alone,
without a GPU: every kernel form is reached, every noise field separates both masks and keeps every pixel out of the band in which
device and oracle may differ, every planted rectangle is the oracle's box, and the multi-chunk FoE cases really carry survivors,
winners and ties past the first chunk of 1024 line pairs."""
import numpy as np
import pytest

import detect_cases as dc
from oracle import foe_oracle as fo


def test_every_kernel_form_is_reached():
    """Each case reaches the forms it names, and together the cases reach every form of FORMS (those of UNTESTED need a misaligned
    device pointer and are left out on purpose; see the comment there)."""
    reached = {g: set() for g in dc.FORMS}
    for case in dc.PHI_CASES + [dc.AUTO_CASE]:
        got = dc.case_forms(case)
        names = {f for _, f in got}
        assert case.expects <= names, (case.name, sorted(case.expects - names))
        for g, f in got:
            reached[g].add(f)
    for g, f in dc.other_forms():
        reached[g].add(f)
    for g, forms in dc.FORMS.items():
        assert forms <= reached[g], (g, sorted(forms - reached[g]))
        assert not (dc.UNTESTED.get(g, set()) & reached[g])


def test_predicates_at_the_shapes_they_were_chosen_for():
    """the launcher's arithmetic at the table's shapes, spelled out: a changed constant in kernels_detect.hip must change these too"""
    assert [dc.phi_gx(W) for W in (63, 66, 257, 260, 516, 1920)] == [1, 2, 5, 2, 3, 8]
    assert [dc.phi_nby(H) for H in (1, 15, 17, 33, 37)] == [1, 1, 2, 3, 3]
    assert dc.phi_yloop(8, 32, 3000) == 2 and dc.phi_steps(8, 32, 3000) == 2          # gx * B * nby = 6000 > 4096
    assert dc.phi_yloop(1920, 1080, 64) == 9                                           # the timed configuration: 68 row blocks
    assert dc.phi_steps(66, 33, 3) == 1 and dc.phi_steps(66, 33, 3, 2) == 2 and dc.phi_steps(66, 33, 3, 8) == 3
    assert [dc.foe_chunks(n) for n in dc.FOE_COUNTS] == [1, 2, 2, 3, 4]
    assert dc.window_form(4176, 64) == "nwx>256" and (4176 - 64) // 16 + 1 == 258
    assert [dc.window_form(W, H) for W, H in ((64, 64), (80, 63), (63, 80), (80, 64))] == ["one", "none", "none", "nwx<=256"]
    assert dc.render_forms(66, 33, 1) == {"tail"} and dc.render_forms(63, 17, 3) == {"tail", "straddle"}
    assert dc.render_forms(640, 480, 4) == set()


@pytest.mark.parametrize("case", dc.PHI_CASES, ids=dc.PHI_IDS)
def test_noise_fields_separate_the_masks_and_avoid_the_band(case):
    for call in dc.PHI_CALLS:
        for with_sky in (False, True):
            for b, ref in enumerate(dc.noise_reference(case.W, case.H, call, with_sky)):
                tag = (case.name, call.name, with_sky, b)
                assert dc.band_pixels(ref) == 0, tag            # a condition, not a tolerance: change NOISE_SEED if it ever fails
                if case.W * case.H >= 64 and not with_sky:
                    assert 0.05 <= ref["fixed"].mean() <= 0.95, (tag, ref["fixed"].mean())
                    assert 0.05 <= ref["total"].mean() <= 0.95, (tag, ref["total"].mean())
    if case.W * case.H >= 64:                                   # the sky masks take set pixels away
        for b, (a, s) in enumerate(zip(dc.noise_reference(case.W, case.H, dc.PHI_CALLS[0], False),
                                       dc.noise_reference(case.W, case.H, dc.PHI_CALLS[0], True))):
            assert s["total"].sum() < a["total"].sum(), (case.name, b)


@pytest.mark.parametrize("case", dc.PHI_CASES, ids=dc.PHI_IDS)
def test_planted_rectangle_is_the_oracles_box(case):
    flow, foe, sky, boxes = dc.planted_fields(case.W, case.H)
    assert len(boxes) >= 4 and boxes[-3] == (-1, -1, -1, -1) == boxes[-2] and boxes[-1] == (case.W - 1, case.H - 1) * 2
    for call in dc.PLANT_CALLS:
        for b, want in enumerate(boxes):
            ref = dc.reference(dc.seen_field(flow[b], call.mode(b), np.zeros(3), 1.0), foe[b], sky[b])
            assert ref["box"] == want, (case.name, call.name, b, ref["box"], want)
            assert fo.simple_bounding_box(ref["total"]) == want           # the dynamic mask is the rectangle too
            assert dc.band_pixels(ref) == 0
            if want[0] >= 0:
                x0, y0, x1, y1 = want
                assert int(ref["fixed"].sum()) == (x1 - x0 + 1) * (y1 - y0 + 1)


def test_planted_edges_fall_where_the_kernel_changes_path():
    flow, foe, sky, boxes = dc.planted_fields(516, 37)
    x0s, x1s = {b[0] for b in boxes}, {b[2] for b in boxes}
    y0s, y1s = {b[1] for b in boxes}, {b[3] for b in boxes}
    assert {63, 64, 255, 256} <= x0s and {63, 64, 255, 256, 515} <= x1s
    assert {15, 16} <= y0s and {15, 16, 36} <= y1s
    assert {1, 2, 3} <= {x % 4 for x in x0s} and {1, 2, 3} <= {x % 4 for x in x1s}


def test_large_batch_reference_avoids_the_band():
    refs = dc.auto_reference()
    assert len(refs) == dc.AUTO_CASE.B == 3000
    assert sum(dc.band_pixels(r) for r in refs) == 0
    boxes = {r["box"] for r in refs}
    foes_ = {r["foe"] for r in refs}
    assert len(boxes) > 20 and len(foes_) > 1000                 # the pairs differ: a record written to the wrong pair shows
    fixed = np.mean([r["fixed"].mean() for r in refs])
    assert 0.05 < fixed < 0.95


def test_multi_chunk_foe_cases_carry_state_past_the_first_chunk():
    many, late, tie = 0, 0, 0
    for kind, (gate, radius) in dc.FOE_KINDS.items():
        for n in dc.FOE_COUNTS:
            if dc.foe_chunks(n) < 2:
                continue
            flow, smp = dc.foe_inputs(kind, n)
            t = dc.foe_trace(flow.astype(np.float64), smp, gate, radius)
            assert t["foe"] == fo.get_foe_dense(flow.astype(np.float64), smp, gate, radius)
            print(f"{kind} n_pairs={n}: survivors {t['survivors']}, winner at line pair {t['winner']}, {t['ties']} share the best score")
            many += t["survivors"] > 1024
            late += t["winner"] >= 1024
            tie += t["ties"] > 1
    assert many >= 2 and late >= 2 and tie >= 1, (many, late, tie)


@pytest.mark.parametrize("count", dc.RANSAC_COUNTS)
def test_ransac_sets_are_what_they_claim(count):
    last = dc.ransac_set(count, "last")
    assert fo.ransac(last, dc.RANSAC_RADIUS) == dc.STAR_LAST == tuple(last[-1])
    assert fo.ransac(last[:-1], dc.RANSAC_RADIUS) == (0.0, 0.0)   # without it nobody has a second neighbour... or a first: no winner
    tie = dc.ransac_set(count, "tie")
    assert fo.ransac(tie, dc.RANSAC_RADIUS) == dc.STAR_FIRST == tuple(tie[3])     # index 3 beats the equal score of the last estimate
    assert fo.ransac(tie[::-1], dc.RANSAC_RADIUS) == dc.STAR_LAST
    if count > 16:
        assert 3 // 16 != (count - 1) // 16
    assert dc.ransac_forms(count)


def test_bbox_threshold_type_cannot_show_on_u8_images():
    """k_u8_extents forms `0.1 * max` in double as the reference does (im_helpers.py:55-84).  For u8 images no test can tell that from
    a float32 product: over all 255 maxima and 256 pixel values the two thresholds decide `value > threshold` alike (0.1 and 0.1f both
    lie above 1/10, so at value = max / 10 both products are >= the value) -- which is why tests/test_gpu_detect_forms.py takes the
    expected box from the oracle and claims no more."""
    v = np.arange(256, dtype=np.float64)[None, :]
    m = np.arange(1, 256)
    thr64 = (0.1 * m.astype(np.float64))[:, None]
    thr32 = (np.float32(0.1) * m.astype(np.float32)).astype(np.float64)[:, None]
    assert np.array_equal(v > thr64, v > thr32)
    at = np.arange(256)[None, :] * 10 == m[:, None]               # value = max / 10, the only place the two could part
    assert at.sum() == 25 and not (v > thr64)[at].any() and not (v > thr32)[at].any()


@pytest.mark.parametrize("W,H", dc.RENDER_SHAPES)
def test_render_fields_have_no_pixel_in_the_arctan2_band(W, H):
    """tests/test_gpu_render.py excuses flow-image pixels whose byte changes when arctan2 moves by 2 ulps, up to 1e-4 of a frame: at
    these sizes that is no pixel at all, so the fields must hold none (a condition, as for the arccos band: change NOISE_SEED if not)."""
    import render_ref as rr
    fl = dc.noise_fields(W, H)
    for b in range(dc.PHI_B):
        for seen in (fl[b], fl[b].astype(np.float64), fo.derotate(fl[b], dc.OMEGA[b], dc.DT[b])):
            assert not rr.atan2_sensitive(seen, 2).any(), (W, H, b, seen.dtype)
