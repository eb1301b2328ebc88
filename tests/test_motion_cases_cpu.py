"""The global-motion case table (tests/motion_cases.py) is what it claims to be -- checked from the predicates and the numpy
restatement alone, without a GPU: every form of the two passes, of the calls around them and of the fit's sums is reached by a case,
every case reaches what it names, the thresholds of the grid-stride loops are where the table says, and the planted ties and the step
inputs are what tests/test_gpu_motion_forms.py takes them for."""
import numpy as np
import pytest

import global_motion_ref as R
import motion_cases as mc

# Every entry of CASES by name: a case taken out of the table has to be taken out here too, and then test_every_form_is_reached says
# what it was the only one to reach -- or nothing does, and the removal needs a line of its own in the review.
NAMES = ["tiny1x1b3", "tiny2x1b3", "tiny3x1b3", "tiny1x5b3", "tiny3x3b3", "tiny5x2b3", "64x64b1", "97x71b3", "1025x1025b1", "1025x1025b2",
         "1449x1449b1", "outputs97x71b3", "outputs1025x1025b2", "step97x71b3_failed", "caller64x64b2_aligned", "caller64x64b2_flow+8B",
         "caller64x64b2_gray+1B", "caller64x64b2_warped+8B", "caller64x64b2_mag+4B", "caller97x71b3_aligned", "step64x64b2_aligned", "step64x64b2_flow+8B",
         "step64x64b2_gray+1B", "fit4", "fit15", "fit16", "fit256", "fit1000_frame_like", "fit_bound"]


def _reached(cases):
    reached = {g: set() for g in mc.FORMS}
    for c in cases:
        for g, f in mc.case_forms(c):
            reached[g].add(f)
    return reached


def test_every_form_is_reached():
    """Each case reaches the forms it names, together they reach every form of FORMS, and what UNTESTED lists is indeed not reached."""
    assert [c.name for c in mc.CASES] == NAMES
    for c in mc.CASES:
        names = {f"{g}={f}" for g, f in mc.case_forms(c)}
        assert c.expects and c.expects <= names, (c.name, sorted(c.expects - names))
    reached = _reached(mc.CASES)
    for g, forms in mc.FORMS.items():
        assert reached[g] <= forms, (g, sorted(reached[g] - forms))                 # a predicate invented a form FORMS does not name
        assert forms <= reached[g], (g, sorted(forms - reached[g]))
    assert set(mc.UNTESTED) <= set(mc.FORMS)
    for g, forms in mc.UNTESTED.items():
        assert not forms & (reached[g] | mc.FORMS[g]), g


def test_the_table_needs_its_cases():
    """Without the cases past the caps, the tiny frames, the output cases, the step cases or the caller's pointers, forms go unreached:
    the check above is not satisfied by the existing sizes alone."""
    def missing(keep):
        reached = _reached([c for c in mc.CASES if keep(c)])
        return {f"{g}={f}" for g, forms in mc.FORMS.items() for f in forms - reached[g]}
    assert missing(lambda c: c.n0 <= mc.second_iteration_pixel(mc.PX_A)) == {"passA.stride=>1", "passA.stride=>1:partial-last", "passB.stride=>1"}
    assert "passB.stride=>1" in missing(lambda c: c.name != "1449x1449b1")
    assert missing(lambda c: not c.name.startswith("tiny")) == {"passB.quad=several-row-ends", "passB.tail=cnt2"}
    assert {"passA.outputs=none", "passA.outputs=warped", "passA.outputs=mag", "passA.outputs=gm:nokey", "passA.outputs=warped:nokey",
            "passA.key=nokey"} <= missing(lambda c: not c.name.startswith("outputs") and c.entry != "step")
    assert {"m_stride=9", "ok=all-good", "ok=one-failed", "gather.blocks=n%256==0"} <= missing(lambda c: c.entry != "step")
    assert {f"ptr={f}" for f in mc.FORMS["ptr"] - {"staged"}} <= missing(lambda c: c.entry == "host" or c.entry == "fit")
    assert {"fit.n=4", "fit.n=bound", "fit.sum_tail=n<16"} <= missing(lambda c: c.entry != "fit")
    # the two sizes kept from tests/test_gpu_global_motion.py reach these and no more of the passes' forms
    old = _reached([mc.BY_NAME["64x64b1"], mc.BY_NAME["97x71b3"]])
    assert old["passA.stride"] == {"1"} and old["passB.stride"] == {"1"} and old["passB.tail"] == {"cnt4", "cnt3"}


def test_thresholds_of_the_grid_stride_loops():
    """The arithmetic of motion_blocks() and of the two loops, spelled out: a changed constant in kernels_motion.hip must change these."""
    assert mc.second_iteration_pixel(mc.PX_A) == 2048 * 256 * 2 == 1_048_576
    assert mc.second_iteration_pixel(mc.PX_B) == 2048 * 256 * 4 == 2_097_152
    assert [mc.motion_blocks(n) for n in (0, 1, 256, 257, 2047 * 256, 2047 * 256 + 1, 10 ** 7)] == [1, 1, 1, 2, 2047, 2048, 2048]
    for W, H, a, b in ((211, 97, {"1"}, {"1"}), (1280, 720, {"1"}, {"1"}), (1024, 1024, {"1"}, {"1"}),
                       (1025, 1025, {">1", ">1:partial-last"}, {"1"}), (1920, 1024, {">1", ">1:partial-last"}, {"1"}),
                       (2048, 1024, {">1"}, {"1"}), (1449, 1449, {">1", ">1:partial-last"}, {">1", ">1:partial-last"})):
        assert mc.stride_forms(W * H, mc.PX_A) == a and mc.stride_forms(W * H, mc.PX_B) == b, (W, H)
    # the pixel the table calls the first of the second iteration is the first one thread 0 of workgroup 0 takes there, and the last
    # pixel of the first iteration belongs to the last thread of the last workgroup
    for n0, px in ((1025 * 1025, mc.PX_A), (1449 * 1449, mc.PX_A), (1449 * 1449, mc.PX_B)):
        T = mc.grid_threads(n0, px)
        assert T == 2048 * 256 and mc.pass_items(n0, px) > T
        assert (0 + T) * px == mc.second_iteration_pixel(px) and ((T - 1) * px + px - 1) == mc.second_iteration_pixel(px) - 1
    assert mc.pass_items(1025 * 1025, 2) - 2048 * 256 == 1025                       # pairs of pass A's second iteration at 1025 x 1025
    assert 1449 == min(s for s in range(1025, 1500, 2) if s * s > mc.second_iteration_pixel(mc.PX_B))
    assert 1025 == min(s for s in range(3, 1500, 2) if s * s > mc.second_iteration_pixel(mc.PX_A))


def _walk(W, H, px):
    """The kernels' own index walk over a small frame: per thread item the pixels it holds and the row ends between them."""
    n0, out = W * H, []
    for q in range((n0 + px - 1) // px):
        p0 = px * q
        cnt = min(px, n0 - p0)
        y, x = divmod(p0, W)
        ends = 0
        for i in range(cnt):
            if i:
                ends += (x == 0)
            x += 1
            if x == W:
                x, y = 0, y + 1
        out.append((cnt, ends))
    return out


@pytest.mark.parametrize("W,H", mc.TINY + [(4, 3), (7, 5), (8, 2), (2, 6), (97, 71)])
def test_tail_and_row_end_predicates_equal_a_literal_walk(W, H):
    a, b = _walk(W, H, 2), _walk(W, H, 4)
    assert mc.pass_a_tail(W * H) == ("odd-last-pixel" if a[-1][0] == 1 else "even")
    assert mc.pass_a_pair_forms(W, H) == {("straddles-row-end" if e else "in-row") for c, e in a if c == 2}
    assert mc.pass_b_tail_forms(W * H) == {f"cnt{c}" for c, _ in b}
    assert mc.pass_b_quad_forms(W, H) == {("in-row", "one-row-end", "several-row-ends")[min(e, 2)] for _, e in b}


def test_access_predicates_at_the_bases_they_were_chosen_for():
    # odd W * H: item 1's flow base is 8 bytes past a 16-byte boundary, item 2's is aligned again
    assert [mc.pass_a_vec(97 * 71, b) for b in range(3)] == [True, False, True]
    assert [mc.pass_b_vec(97 * 71, b) for b in range(3)] == [True, False, False]    # gray + 2 * 6887: 2 mod 4
    assert [mc.pass_b_vec(10, b) for b in range(3)] == [True, False, True] and all(mc.pass_a_vec(10, b) for b in range(3))
    n0 = 64 * 64
    assert all(mc.pass_a_vec(n0, b) and mc.pass_b_vec(n0, b) for b in range(2))
    assert not any(mc.pass_a_vec(n0, b, flow_off=8) or mc.pass_b_vec(n0, b, flow_off=8) for b in range(2))
    assert not any(mc.pass_b_vec(n0, b, gray_off=1) for b in range(2)) and all(mc.pass_a_vec(n0, b) for b in range(2))
    assert not mc.pass_a_vec(n0, 0, warped_off=8) and mc.pass_a_vec(n0, 0, warped_off=None, mag_off=None, gm_off=None)
    assert not mc.pass_a_vec(n0, 0, mag_off=4) and mc.pass_a_vec(n0, 0, mag_off=8) and not mc.pass_a_vec(n0, 0, gm_off=8)
    # an output that is not requested does not count: only the flow's base decides then
    assert mc.pass_a_vec(n0, 0, warped_off=None, mag_off=None, gm_off=None) and not mc.pass_a_vec(n0, 0, 8, None, None, None)


@pytest.mark.parametrize("name", ["1025x1025b1", "1449x1449b1"])
def test_planted_ties_report_their_first_pixel(name):
    """The restatement on the planted fields: magnitude 5.0 exactly at the planted pixels, the first of them is flow_max, the gray image is
    255 there and 0 elsewhere."""
    c = mc.BY_NAME[name]
    ties = mc.tie_pixels(c)
    assert set(ties) == {k for k in c.fields if k.startswith("ties")}
    edge = mc.second_iteration_pixel(mc.PX_A)
    assert ties["ties_all"] == (edge - 1, edge, c.n0 - 1) and ties["ties_late"] == (edge, c.n0 - 1) and ties["ties_last"] == (c.n0 - 1,)
    if "tiesB_all" in ties:
        assert ties["tiesB_all"][:2] == (2_097_151, 2_097_152) and ties["tiesB_late"][0] == 2_097_152
    for kind, px in ties.items():
        flows, Ms = mc.fields_of(c, kind)
        sub = R.subtract(flows[0], Ms[0])
        assert sub["flow_max"] == divmod(px[0], c.W), (kind, sub["flow_max"])
        flat = sub["mag"].ravel()
        assert np.flatnonzero(flat).tolist() == list(px) and (flat[list(px)] == np.float32(mc.TIE_MAG)).all()
        assert np.flatnonzero(sub["gray"].ravel()).tolist() == list(px) and (sub["gray"].ravel()[list(px)] == 255).all()


def test_step_inputs_fail_where_the_table_says():
    for c in mc.CASES:
        if c.entry != "step":
            continue
        flows, coords = mc.step_inputs(c)
        assert coords.shape == (c.n, 2) and coords[:, 0].max() < c.W and coords[:, 1].max() < c.H and coords.min() >= 0
        oks = [R.find_homography(coords.astype(np.float64), R.coords_new(coords, flows[b]))[1] for b in range(c.B)]
        assert oks == [0 if b == c.failed else 1 for b in range(c.B)], (c.name, oks)


def test_fit_pairs_have_the_size_the_case_names():
    for c in mc.CASES:
        if c.entry == "fit":
            src, dst = mc.fit_pairs(c)
            assert src.shape == dst.shape == (c.n, 2) and src.dtype == dst.dtype == np.float64, c.name
    assert mc.MAX_PAIRS == 65536
    import os
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "mavflow.h")).read()
    assert f"#define MAV_HOMOGRAPHY_MAX_PAIRS {mc.MAX_PAIRS}\n" in hdr
