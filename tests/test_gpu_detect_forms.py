"""Every kernel instance of the detection path (csrc/kernels_detect.hip) against the numpy oracle at ragged shapes: the cases of
tests/detect_cases.py -- widths that are no multiple of 4, one and several column tiles and row blocks, frames of a single pixel, a
row-block loop of more than one step (by option and by the launcher's own rule), line-pair counts past one chunk of 1024, batches
past one block of 64 -- through the C ABI, against oracle/foe_oracle.py and tests/render_ref.py.

Bars: FoE, masks, boxes, records, counts, derotated flow and the result / phi images bit for bit; phi and max(phi) within the
project's own bars (PHI_ATOL of tests/test_gpu_detect.py for float64 pairs, ARCCOS_ULPS of tests/test_frame0.py for float32 pairs);
the flow image as tests/test_gpu_render.py holds it.  Masks are compared with array_equal and nothing is excused:
tests/test_detect_cases_cpu.py shows from the oracle alone that no pixel of any field used here lies inside the band in which the
device's arccos could decide differently."""
import ctypes as C

import numpy as np
import pytest

import detect_cases as dc
from oracle import foe_oracle as fo
from test_gpu_render import _check_flow_image, _expected

pytestmark = pytest.mark.gpu


def _ctx(W, H, B):
    from mavflow import _lib
    return _lib.Context(W, H, B)


def _run_phi(c, call, flow32, foe, omega, dt, sky, want_phi, smp=None):
    """One call into k_phi_mask the way `call` names it -> dict(phi, max_phi, fixed, total, box, foe), each None where the entry point
    does not return it."""
    from mavflow import _lib
    B = flow32.shape[0]
    if call.entry == "stage":
        phi, mf, md, box = c.stage_phi_mask(flow32, foe, omega=omega if call.rates else None, dt=dt if call.rates else None, sky=sky,
                                            want_phi=want_phi)
        return dict(phi=phi, max_phi=None, fixed=mf, total=md, box=box, foe=None)
    if call.entry == "host":
        fl = flow32 if call.flow == "f32" else flow32.astype(np.float64)
        phi, mf, md, mx = c.phi_mask(fl, foe, sky=sky, want_phi=want_phi)
        return dict(phi=phi, max_phi=mx, fixed=mf, total=md, box=None, foe=None)
    fp = _lib.foe_defaults()
    fp.n_pairs, fp.mag_threshold = dc.DETECT_PAIRS, dc.DETECT_GATE
    f0 = [call.frame0[b % len(call.frame0)] for b in range(B)]
    out = c.detect(flow32, smp, omega=omega, dt=dt, sky=sky, frame0=f0, foe_params=fp, want_phi=want_phi)
    return dict(phi=out["phi"], max_phi=None, fixed=out["mask_fixed"], total=out["mask_dyn"], box=out["results"]["box"],
                foe=out["results"]["foe"])


def _hold(got, refs, tag):
    """one call's outputs against the oracle's answer for each of its pairs"""
    for b, ref in enumerate(refs):
        t = tag + (b,)
        if got["foe"] is not None:
            assert tuple(got["foe"][b]) == ref["foe"], t
        assert np.array_equal(got["fixed"][b], ref["fixed"]), (t, int((got["fixed"][b] != ref["fixed"]).sum()))
        assert np.array_equal(got["total"][b], ref["total"]), (t, int((got["total"][b] != ref["total"]).sum()))
        if got["box"] is not None:
            assert tuple(int(v) for v in got["box"][b]) == ref["box"], (t, tuple(got["box"][b]), ref["box"])
        if got["phi"] is not None:
            assert dc.phi_close(got["phi"][b], ref["phi"]), t
        if got["max_phi"] is not None:
            assert dc.phi_close(got["max_phi"][b:b + 1], ref["phi"].max(keepdims=True).reshape(1)), t


def _same(a, b):
    return all((a[k] is None and b[k] is None) or (k in ("phi", "max_phi")) or np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes()
               for k in a)


@pytest.mark.parametrize("case", dc.PHI_CASES, ids=dc.PHI_IDS)
def test_phi_mask_noise_fields(mav, case):
    """Three pairs with a field, FoE (in the middle, outside the frame, on a pixel centre), sky mask and rates of their own, through
    every entry point and pair mode, screened and exact, with and without sky; one mav_detect call mixes a frame-0 pair with two
    derotated ones."""
    W, H = case.W, case.H
    fl, fe = dc.noise_fields(W, H), dc.foes(W, H)
    smp = dc.detect_samples(W, H, dc.PHI_B, dc.DETECT_PAIRS)
    with _ctx(W, H, dc.PHI_B) as c:
        for call in dc.PHI_CALLS:
            for with_sky in (False, True):
                sky = dc.sky_masks(W, H) if with_sky else None
                refs = dc.noise_reference(W, H, call, with_sky)
                screened = _run_phi(c, call, fl, fe, dc.OMEGA, dc.DT, sky, False, smp)
                exact = _run_phi(c, call, fl, fe, dc.OMEGA, dc.DT, sky, True, smp)
                _hold(screened, refs, (case.name, call.name, with_sky, "screened"))
                _hold(exact, refs, (case.name, call.name, with_sky, "exact"))
                assert _same(screened, exact), (case.name, call.name, with_sky)
                assert exact["phi"] is not None and screened["phi"] is None


@pytest.mark.parametrize("case", dc.PHI_CASES, ids=dc.PHI_IDS)
def test_phi_mask_planted_rectangles(mav, case):
    """Exactly radial flow with one rectangle turned by 90 degrees per pair: the box must be the rectangle, whose edges fall on and
    either side of every column and row at which the kernel starts a new lane, tile, nibble or row block; an empty mask, an
    all-sky pair and a single pixel in the last column of the last row among them."""
    W, H = case.W, case.H
    flow, foe, sky, boxes = dc.planted_fields(W, H)
    B = len(boxes)
    zero, one = np.zeros((B, 3)), np.ones(B)
    with _ctx(W, H, B) as c:
        for call in dc.PLANT_CALLS:
            refs = [dc.reference(dc.seen_field(flow[b], call.mode(b), zero[b], 1.0), foe[b], sky[b]) for b in range(B)]
            assert [r["box"] for r in refs] == boxes
            for want_phi in (False, True):
                got = _run_phi(c, call, flow, foe, zero, one, sky, want_phi)
                _hold(got, refs, (case.name, call.name, want_phi))
        # the masks as plain u8 images through mav_bbox: k_u8_max / k_u8_extents at the same edges
        masks = np.stack([r["fixed"] for r in refs]).astype(np.uint8) * 200
        assert [tuple(int(v) for v in bx) for bx in c.bbox(masks)] == boxes


@pytest.mark.parametrize("case", [k for k in dc.PHI_CASES if k.yloop_options], ids=lambda k: k.name)
def test_phi_options_change_no_byte(mav, case):
    """Option "phi_yloop" at 1, 2 and a value above the number of row blocks, and "phi_screen" = 0, on the shapes with three row
    blocks: the same bytes as the default context's, which are the oracle's (include/mavflow.h: "None of them changes a result bit")."""
    W, H = case.W, case.H
    fl, fe, sky = dc.noise_fields(W, H), dc.foes(W, H), dc.sky_masks(W, H)
    assert dc.phi_nby(H) == 3 and max(case.yloop_options) > 3
    calls = (dc.PHI_CALLS[0], dc.PHI_CALLS[1], dc.PHI_CALLS[2])
    with _ctx(W, H, dc.PHI_B) as c:
        base = {call.name: _run_phi(c, call, fl, fe, dc.OMEGA, dc.DT, sky, False) for call in calls}
    for call in calls:
        _hold(base[call.name], dc.noise_reference(W, H, call, True), (case.name, call.name, "default"))
    settings = [("phi_yloop", v) for v in case.yloop_options] + [("phi_screen", 0)]
    for name, value in settings:
        with _ctx(W, H, dc.PHI_B) as c:
            c.set_option(name, value)
            assert c.get_option(name) == value
            for call in calls:
                got = _run_phi(c, call, fl, fe, dc.OMEGA, dc.DT, sky, False)
                assert _same(got, base[call.name]), (case.name, call.name, name, value)
                got = _run_phi(c, call, fl, fe, dc.OMEGA, dc.DT, sky, True)
                _hold(got, dc.noise_reference(W, H, call, True), (case.name, call.name, name, value, "exact"))


def test_a_null_mask_output(mav):
    """mav_stage_phi_mask with one mask output NULL: the other mask and the box are unchanged."""
    from mavflow import _lib
    W, H = 66, 33
    fl, fe, sky = dc.noise_fields(W, H), dc.foes(W, H), dc.sky_masks(W, H).astype(np.uint8)
    refs = dc.noise_reference(W, H, dc.PHI_CALLS[0], True)
    flow = np.ascontiguousarray(fl)
    foe = np.ascontiguousarray(fe)
    thr = _lib.thr_defaults()
    with _ctx(W, H, dc.PHI_B) as c:
        for keep in ("fixed", "total"):
            m = np.full((dc.PHI_B, H, W), 7, np.uint8)
            box = np.full((dc.PHI_B, 4), 7, np.int32)
            p = m.ctypes.data_as(C.c_void_p)
            _lib.check(c.lib.mav_stage_phi_mask(c.h, flow.ctypes.data_as(C.c_void_p), foe.ctypes.data_as(C.c_void_p), None, None,
                                                sky.ctypes.data_as(C.c_void_p), dc.PHI_B, C.byref(thr), None,
                                                p if keep == "fixed" else None, p if keep == "total" else None,
                                                box.ctypes.data_as(C.c_void_p)))
            for b, ref in enumerate(refs):
                assert np.array_equal(m[b].view(np.bool_), ref[keep]) and m[b].max() <= 1, (keep, b)
                assert tuple(int(v) for v in box[b]) == ref["box"], (keep, b)


def test_large_batch_on_tiny_frames_takes_two_row_blocks_per_workgroup(mav):
    """8 x 32 x 3000 pairs through mav_detect: gx * B * nby = 6000 > 4096, so the launcher folds two row blocks into each workgroup
    (the automatic yloop > 1, otherwise reached at 1080p x 64 only), blockIdx.z runs to 2999, and k_box_init / k_finalize get 47
    blocks.  Every pair's record, masks and box against the oracle; then the masks through mav_bbox."""
    from mavflow import _lib
    case = dc.AUTO_CASE
    assert dc.phi_steps(case.W, case.H, case.B) == 2
    flow, omega, dt, frame0, sky, smp = dc.auto_inputs()
    refs = dc.auto_reference()
    fp = _lib.foe_defaults()
    fp.n_pairs, fp.mag_threshold = dc.AUTO_PAIRS, dc.DETECT_GATE
    with _ctx(case.W, case.H, case.B) as c:
        out = c.detect(flow, smp, omega=omega, dt=dt, sky=sky, frame0=frame0, foe_params=fp)
        boxes = c.bbox(out["mask_fixed"].view(np.uint8))
    want_foe = np.array([r["foe"] for r in refs])
    want_box = np.array([r["box"] for r in refs], np.int32)
    bad = np.flatnonzero((out["results"]["foe"].view(np.uint64) != want_foe.view(np.uint64)).any(axis=1))
    assert bad.size == 0, (bad.size, bad[:5])
    assert np.array_equal(out["mask_fixed"], np.stack([r["fixed"] for r in refs]))
    assert np.array_equal(out["mask_dyn"], np.stack([r["total"] for r in refs]))
    bad = np.flatnonzero((out["results"]["box"] != want_box).any(axis=1))
    assert bad.size == 0, (bad.size, bad[:5], out["results"]["box"][bad[:5]], want_box[bad[:5]])
    assert np.array_equal(boxes, want_box)


# ---- FoE -----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx_foe(mav):
    with _ctx(dc.FOE_W, dc.FOE_H, 2) as c:
        yield c


@pytest.mark.parametrize("n_pairs", dc.FOE_COUNTS)
@pytest.mark.parametrize("kind", sorted(dc.FOE_KINDS))
def test_foe_with_several_chunks(ctx_foe, kind, n_pairs):
    """k_foe_candidates walks its line pairs in chunks of 1024 and carries the survivor count between them; RANSAC's first-wins
    tie-break needs the order kept across chunks.  float64 flow, float32 flow (the float32 gate) and, through mav_detect, a frame-0
    pair next to a derotated one: the FoE as bytes."""
    from mavflow import _lib
    gate, radius = dc.FOE_KINDS[kind]
    flow32, smp = dc.foe_inputs(kind, n_pairs)
    p = _lib.foe_defaults()
    p.n_pairs, p.mag_threshold, p.ransac_threshold = n_pairs, gate, radius
    flow64 = flow32.astype(np.float64)
    with np.errstate(all="ignore"):
        want64 = np.array(fo.get_foe_dense(flow64, smp, gate, radius))
        want32 = np.array(fo.get_foe_dense(flow32, smp, gate, radius))
        der = fo.derotate(flow32, dc.OMEGA[1], dc.DT[1])
        want_der = np.array(fo.get_foe_dense(der, smp, gate, radius))
    assert ctx_foe.foe_dense(flow64, smp, p)[0].tobytes() == want64.tobytes()
    assert ctx_foe.foe_dense(flow32, smp, p)[0].tobytes() == want32.tobytes()
    out = ctx_foe.detect(np.stack([flow32, flow32]), np.stack([smp, smp]), omega=dc.OMEGA[:2], dt=dc.DT[:2], frame0=[1, 0], foe_params=p)
    assert out["results"]["foe"][0].tobytes() == want32.tobytes()
    assert out["results"]["foe"][1].tobytes() == want_der.tobytes()
    # the second pair's candidates lie behind the first's in the scratch (cand + b * 2 * N): both orders of the pairs
    out = ctx_foe.detect(np.stack([flow32, flow32]), np.stack([smp, smp]), omega=dc.OMEGA[[1, 0]], dt=dc.DT[[1, 0]], frame0=[0, 1], foe_params=p)
    assert out["results"]["foe"][0].tobytes() == want_der.tobytes()
    assert out["results"]["foe"][1].tobytes() == want32.tobytes()


@pytest.mark.parametrize("count", dc.RANSAC_COUNTS)
def test_ransac_counts_at_workgroup_and_wave_boundaries(ctx_foe, count):
    """mav_ransac at and around the 16-candidate workgroup and 4-candidate wave boundaries and at the 4096 bound: a cluster in clutter,
    a set whose winner is the last estimate, and two equal best scores whose earlier estimate sits in another workgroup."""
    for kind in ("random", "last", "tie"):
        est = dc.ransac_set(count, kind)
        assert ctx_foe.ransac(est) == fo.ransac(est, dc.RANSAC_RADIUS), (count, kind)
    est = dc.ransac_set(count, "random")
    assert ctx_foe.ransac(est, 5.0) == fo.ransac(est, 5.0)


def test_ransac_refuses_more_than_4096_estimates(ctx_foe):
    with pytest.raises(ValueError, match="4097"):                             # MAV_ERR_ARG, as mavflow._lib.check maps it
        ctx_foe.ransac(np.zeros((4097, 2)))
    assert ctx_foe.ransac(dc.ransac_set(17, "last")) == dc.STAR_LAST          # the context is still usable


# ---- result images ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", dc.RENDER_BATCHES)
@pytest.mark.parametrize("W,H", dc.RENDER_SHAPES)
def test_render_tail_and_straddle(mav, W, H, B):
    """k_render gives a thread four consecutive pixels of the flattened (B, H, W) index: with W * H no multiple of 4 the last thread
    has a tail, and with B = 3 a thread's pixels belong to two pairs (other FoE, rates, sky, arithmetic type).  Built exactly as
    test_process_batch_images_match_the_restatement builds it, from mav_detect's own phi and mask (held to the oracle above)."""
    from mavflow import _lib
    assert "tail" in dc.render_forms(W, H, B) and (B == 1 or "straddle" in dc.render_forms(W, H, B))
    fl = dc.noise_fields(W, H)[:B]
    sky = dc.sky_masks(W, H)[:B].astype(np.uint8)
    smp = dc.detect_samples(W, H, B, dc.DETECT_PAIRS)
    fp = _lib.foe_defaults()
    fp.n_pairs, fp.mag_threshold = dc.DETECT_PAIRS, dc.DETECT_GATE
    with _ctx(W, H, B) as c:
        for frame0 in ([1, 0, 0][:B], [0, 1, 0][:B]):
            omega, dt = dc.OMEGA[:B], dc.DT[:B]
            out = c.detect(fl, smp, omega=omega, dt=dt, sky=sky, frame0=frame0, foe_params=fp, want_phi=True)
            last = c.render_last(B)
            foe = np.ascontiguousarray(out["results"]["foe"])
            fresh = c.render(fl, foe, omega=omega, dt=dt, sky=sky, frame0=frame0)
            alone = {k: c.render(fl, foe, omega=omega, dt=dt, sky=sky, frame0=frame0, images=(k,)) for k in ("result", "flow", "phi")}
            for k in ("result", "flow", "phi"):
                assert np.array_equal(last[k], fresh[k]), (k, frame0)
                assert set(alone[k]) == {k} and np.array_equal(alone[k][k], fresh[k]), (k, frame0)
            for b in range(B):
                want, der = _expected(fl[b], out["phi"][b], out["mask_fixed"][b], omega[b], dt[b], frame0[b])
                assert np.array_equal(fresh["result"][b], want["result"]), (b, frame0)
                assert np.array_equal(fresh["phi"][b], want["phi"]), (b, frame0)
                _check_flow_image(fresh["flow"][b], der, f"{W}x{H}x{B} pair {b} frame0={frame0[b]}")


@pytest.mark.parametrize("B", dc.RENDER_BATCHES)
@pytest.mark.parametrize("W,H", dc.RENDER_SHAPES)
def test_flow_to_color_tail_and_straddle(mav, W, H, B):
    fl = dc.noise_fields(W, H)[:B]
    with _ctx(W, H, B) as c:
        for field in (fl, fl.astype(np.float64)):
            got = c.flow_to_color(field)
            for b in range(B):
                _check_flow_image(got[b], field[b], f"flow_to_color {field.dtype} {W}x{H}x{B} pair {b}")


# ---- window search, level 0 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", dc.WINDOW_SHAPES)
def test_window_max_shapes(mav, W, H):
    """No window at all (a side below 64), exactly one, and 258 windows in a row: k_window_max's `wx += 256` loop takes a second step
    for windows 256 and 257 only."""
    rng = np.random.default_rng(W + H)
    imgs = np.zeros((3, H, W), np.uint8)
    imgs[0] = rng.integers(0, 256, (H, W))
    if dc.window_form(W, H) == "nwx>256":
        imgs[0] = rng.integers(0, 100, (H, W))
        imgs[0, :, 257 * 16:] = 255                                   # the strictly largest sum belongs to window 257, the last
        imgs[1, :, 0:64] = 9                                          # windows 0 and 256 tie: window 0 must win
        imgs[1, :, 256 * 16:256 * 16 + 64] = 9
    else:
        imgs[1, H // 2:, W // 3:] = 255
    with _ctx(W, H, 3) as c:
        got = c.window_max(imgs)
    for b in range(3):
        assert tuple(int(v) for v in got[b]) == fo.analyze_pyramid_level0(imgs[b]), b
    assert tuple(got[2]) == (0, 0, 0)
    if dc.window_form(W, H) == "none":
        assert not got.any()
    if dc.window_form(W, H) == "nwx>256":
        assert tuple(got[0][1:]) == (257 * 16, 0) and tuple(got[1]) == (3 * 9 * 64 * 64, 0, 0)
        assert fo.analyze_pyramid_level0(imgs[1][:, 16:])[1] == 255 * 16          # without window 0 the tie goes to window 256


def test_window_max_batch_of_70(mav):
    W, H, B = dc.WINDOW_BATCH
    rng = np.random.default_rng(70)
    imgs = rng.integers(0, 256, (B, H, W)).astype(np.uint8)
    imgs[65] = 0
    imgs[69, :, 16:] //= 2
    with _ctx(W, H, B) as c:
        got = c.window_max(imgs)
    for b in range(B):
        assert tuple(int(v) for v in got[b]) == fo.analyze_pyramid_level0(imgs[b]), b
    assert tuple(got[65]) == (0, 0, 0) and len({tuple(g) for g in got}) > 60


# ---- get_simple_bounding_box on u8 images ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", dc.BBOX_SHAPES)
def test_bbox_column_tiles(mav, W, H):
    """k_u8_extents walks 256-column tiles.  Single brightest pixels at columns 0, 255, 256 and the last; a pixel of value 1 under
    a maximum of 10 (1 > 0.1 * 10 is decided by the reference's double comparison: the expected value is the oracle's); all zero."""
    cols = sorted({0, min(255, W - 1), min(256, W - 1), W - 1})
    imgs = np.zeros((len(cols) + 4, H, W), np.uint8)
    for i, x in enumerate(cols):
        imgs[i] = 20
        imgs[i, (i * 2) % H, x] = 255
    n = len(cols)
    imgs[n, H - 1, W - 1] = 10                                        # maximum 10 ...
    imgs[n, 0, 0] = 1                                                 # ... and a pixel of value 1
    imgs[n + 1, H // 2, W // 2] = 10
    imgs[n + 1, H - 1, 0] = 2
    imgs[n + 2] = 255
    with _ctx(W, H, len(imgs)) as c:
        got = c.bbox(imgs)
    for b in range(len(imgs)):
        assert tuple(int(v) for v in got[b]) == fo.simple_bounding_box(imgs[b]), b
    for i, x in enumerate(cols):
        assert tuple(got[i]) == (x, (i * 2) % H, x, (i * 2) % H)
    assert tuple(got[-1]) == (-1, -1, -1, -1) and tuple(got[n + 2]) == (0, 0, W - 1, H - 1)


# ---- derotation ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", dc.DEROT_SHAPES)
def test_derotate_ragged_shapes(mav, W, H):
    fl = dc.noise_fields(W, H)
    with _ctx(W, H, dc.PHI_B) as c:
        got = c.derotate(fl, dc.OMEGA, dc.DT)
    for b in range(dc.PHI_B):
        assert got[b].tobytes() == fo.derotate(fl[b], dc.OMEGA[b], dc.DT[b]).tobytes(), b


# ---- calculate_tpr_fpr ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", dc.TPR_SHAPES)
def test_tpr_fpr_counts_mask_values(mav, W, H):
    """37 x 29 takes the byte-by-byte kernel (the pixel count is no multiple of 16), 64 x 48 the 16-byte one; mask_value 2 (gt * 2 > 127
    only from gt = 64 up), 128 and 65535 (no 8- or 16-bit wrap), formed as test_validation_counts_on_resident_masks forms the rates."""
    rng = np.random.default_rng(W)
    B = 3
    gt = rng.choice(np.array([0, 1, 63, 64, 90, 127, 128, 191, 192, 254, 255], np.uint8), (B, H, W))
    mask = rng.random((B, H, W)) < 0.4
    with _ctx(W, H, B) as c:
        for value in dc.TPR_VALUES:
            counts = c.tpr_fpr_counts(gt, mask, value)
            for b in range(B):
                with np.errstate(all="ignore"):
                    exp = fo.calculate_tpr_fpr(gt[b], value * mask[b].astype(np.int64))
                    got = (counts[b][2] / counts[b][0], counts[b][3] / counts[b][1])
                assert np.array(got).tobytes() == np.array(exp, np.float64).tobytes(), (value, b, counts[b])
                assert counts[b][0] == (gt[b] > 127).sum() and counts[b][1] == ((255 - gt[b].astype(np.int64)) > 127).sum()
        for value in (0, 65536):
            with pytest.raises(ValueError, match="mask_value"):                # MAV_ERR_ARG, as mavflow._lib.check maps it
                c.tpr_fpr_counts(gt, mask, value)
        assert c.tpr_fpr_counts(gt, mask, 255).shape == (B, 4)
