"""The global-motion branch on the GPU (csrc/kernels_motion.hip and the calls around it) against the numpy restatement
tests/global_motion_ref.py and, for the window search on the normalised image, oracle/pyramid_oracle.py.  Equal bytes everywhere:
no tolerance appears in this file.  The restatement's full-frame half is pinned to the reference by tests/golden/global_motion.npz
(tests/test_global_motion_ref_cpu.py); the fit's restatement is held to an independent least-squares minimiser by
tests/test_homography_lsq_cpu.py and is not pinned against cv2."""
import logging
import os

import numpy as np
import pytest

import global_motion_ref as R
from global_motion_cases import degenerate_pairs, fit_cases
from oracle import pyramid_oracle as po

pytestmark = pytest.mark.gpu

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "global_motion.npz"))
HOMOGRAPHY = np.array([[1.013, -0.021, 2.75], [0.017, 0.991, -1.5], [3e-5, -2e-5, 1.0]])
# W, H, batch: exactly one window | ragged, three windows, level 1 too small | windows on two levels | no window fits | the golden
# window fixtures' size.  None has an integer-ratio pyramid level.
SIZES = [(64, 64, 1), (97, 71, 3), (211, 97, 2), (63, 80, 1), (200, 150, 1)]


def _ctx(W, H, B=1):
    from mavflow import _lib
    return _lib.Context(W, H, B)


def expected_record(gray, sub, optimize):
    """The record mav_global_motion must produce for the restated fields `sub` and their image `gray`."""
    pyr = po.analyze_pyramid(gray)
    win = (pyr[1], pyr[2], 64, 64) if pyr[0] else (0, 0, 0, 0)
    score, opt = po.optimize_window(gray, win) if optimize else (0, win)
    return dict(max_mag=np.float32(sub["mag"].max()), max_row=sub["flow_max"][0], max_col=sub["flow_max"][1], window=tuple(int(v) for v in pyr),
                opt_score=int(score), opt_window=tuple(int(v) for v in opt))


def check_record(rec, exp, what):
    assert np.float32(rec["max_mag"]).tobytes() == exp["max_mag"].tobytes(), (what, rec["max_mag"], exp["max_mag"])
    assert (int(rec["max_row"]), int(rec["max_col"])) == (exp["max_row"], exp["max_col"]), (what, rec, exp)
    assert tuple(int(v) for v in rec["window"]) == exp["window"], (what, rec["window"], exp["window"])
    assert int(rec["opt_score"]) == exp["opt_score"] and tuple(int(v) for v in rec["opt_window"]) == exp["opt_window"], (what, rec, exp)


def check_fields(out, b, flow, M, optimize, what):
    sub = R.subtract(flow, M)
    assert out["warped"][b].tobytes() == sub["warped"].tobytes(), what
    assert out["mag"][b].tobytes() == sub["mag"].tobytes(), what
    assert not np.isnan(out["mag"][b]).any() and not np.isnan(out["warped"][b]).any(), what
    assert np.array_equal(out["gray"][b], sub["gray"]), (what, int(np.abs(out["gray"][b].astype(int) - sub["gray"]).max()))
    check_record(out["results"][b], expected_record(sub["gray"], sub, optimize), what)
    return sub


def field_cases(W, H, B, seed):
    """(name, flows (B, H, W, 2) float32, matrices (B, 3, 3))."""
    rng = np.random.default_rng(seed)
    eye = np.broadcast_to(np.eye(3), (B, 3, 3)).copy()
    gen = np.stack([HOMOGRAPHY + rng.normal(0, 1e-3, (3, 3)) * np.array([[1], [1], [0]]) for _ in range(B)])
    zero = np.zeros((B, H, W, 2), np.float32)
    blob = rng.normal(0, 1.5, (B, H, W, 2)).astype(np.float32)
    for b in range(B):                                   # a moving patch, somewhere else in every item
        y0, x0 = int(rng.integers(0, H - 20)), int(rng.integers(0, W - 20))
        blob[b, y0:y0 + 18, x0:x0 + 18] += np.float32(9.0)
    last = zero.copy()
    last[:, H - 1, W - 1] = (3.0, 4.0)
    shift = eye.copy()
    shift[:, 0, 2], shift[:, 1, 2] = 2.5, -1.25
    big = (rng.normal(0, 1, (B, H, W, 2)) * 1e4).astype(np.float32)
    tiny = (rng.normal(0, 1, (B, H, W, 2)) * 1e-30).astype(np.float32)
    return [("random", blob, gen), ("identity_zero", zero, eye), ("constant", zero, shift), ("last_pixel", last, eye), ("1e4", big, gen),
            ("1e-30", tiny, eye)]


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}b{s[2]}")
def test_fields_image_and_windows_equal_the_restatement(size):
    W, H, B = size
    with _ctx(W, H, B) as ctx:
        for name, flows, Ms in field_cases(W, H, B, W * 7 + H):
            for optimize in (False, True):
                out = ctx.global_motion(flows, Ms, optimize=optimize, outputs=("warped", "mag", "gray"))
                for b in range(B):
                    sub = check_fields(out, b, flows[b], Ms[b], optimize, (size, name, optimize, b))
                if name == "identity_zero":
                    assert not out["gray"].any() and not out["mag"].any() and all(int(r["window"][0]) == 0 for r in out["results"])
                    assert all(float(r["max_mag"]) == 0.0 and (int(r["max_row"]), int(r["max_col"])) == (0, 0) for r in out["results"])
                if name == "constant":
                    assert (out["gray"] == 255).all() and all((int(r["max_row"]), int(r["max_col"])) == (0, 0) for r in out["results"])
                if name == "last_pixel":
                    assert all((int(r["max_row"]), int(r["max_col"]), float(r["max_mag"])) == (H - 1, W - 1, 5.0) for r in out["results"])
                if name == "1e-30":
                    assert not out["mag"].any() and np.abs(out["warped"]).max() > 0          # the squares underflow, in numpy and here
            if name == "random":                         # row 2 of a homography is not read; the optional outputs change nothing
                Ms2 = Ms.copy()
                Ms2[:, 2] = (0.5, -0.25, 3.0)
                again = ctx.global_motion(flows, Ms2, optimize=True, outputs=())
                assert again["results"].tobytes() == out["results"].tobytes() and set(again) == {"results"}
                assert ctx.global_motion(flows, Ms[:, :2], optimize=True)["results"].tobytes() == out["results"].tobytes()
        if (W, H) == (63, 80):
            assert all(tuple(r["window"]) == (0,) * 6 for r in out["results"])


@pytest.mark.parametrize("case", [str(c) for c in G["cases"]])
def test_reference_fixture_on_the_device(case):
    """The arrays the reference itself produced, without the restatement in between."""
    flow, M = G[f"{case}_flow"], G[f"{case}_M"]
    H, W = flow.shape[:2]
    with _ctx(W, H) as ctx:
        out = ctx.global_motion(flow, M, outputs=("warped", "mag", "gray"))
        assert out["warped"][0].tobytes() == G[f"{case}_warped"].tobytes() and out["mag"][0].tobytes() == G[f"{case}_mag"].tobytes()
        assert np.array_equal(out["gray"][0], G[f"{case}_image"])
        r = out["results"][0]
        assert (int(r["max_row"]), int(r["max_col"])) == tuple(int(v) for v in G[f"{case}_flow_max"])
        if f"{case}_coords" in G.files:                   # the gathered pairs are the reference's coords_new
            Hm, ok, pairs = ctx.flow_homography(flow, G[f"{case}_coords"], want_pairs=True)
            assert pairs[0].tobytes() == G[f"{case}_coords_new"].tobytes()
            He, oke = R.find_homography(G[f"{case}_coords"].astype(np.float64), G[f"{case}_coords_new"])
            assert int(ok[0]) == oke and Hm[0].tobytes() == He.tobytes(), case


def test_fit_equals_the_restatement():
    with _ctx(64, 64, 3) as ctx:
        cases = fit_cases()
        for name, src, dst, _ in cases:                   # n = 4, 5, 1000, 2666, 64; exact, noisy, far from the origin
            He, oke = R.find_homography(src, dst)
            H, ok = ctx.find_homography(src, dst)
            assert int(ok[0]) == oke == 1 and H[0].tobytes() == He.tobytes(), (name, np.abs(H[0] - He).max())
        three = [c for c in cases if len(c[1]) == 1000]   # batch 3, different data per item
        assert len(three) == 3
        H, ok = ctx.find_homography(np.stack([c[1] for c in three]), np.stack([c[2] for c in three]))
        for b, (name, src, dst, _) in enumerate(three):
            assert int(ok[b]) == 1 and H[b].tobytes() == R.find_homography(src, dst)[0].tobytes(), name


@pytest.mark.parametrize("kind", ["collinear", "repeated", "collinear_dst_axis"])
def test_degenerate_item_between_two_good_ones(kind):
    rng = np.random.default_rng(11)
    good = [(s, s + rng.normal(0, 2, s.shape).astype(np.float32)) for s in (rng.integers(0, 300, (12, 2)).astype(np.float64) for _ in range(2))]
    bad = degenerate_pairs(kind)
    items = [good[0], bad, good[1]]
    with _ctx(64, 64, 3) as ctx:
        H, ok = ctx.find_homography(np.stack([i[0] for i in items]), np.stack([i[1] for i in items]))
        assert ok.tolist() == [1, 0, 1] and not H[1].any()
        for b in (0, 2):
            assert H[b].tobytes() == R.find_homography(*items[b])[0].tobytes(), b
        with pytest.raises(ValueError):
            ctx.find_homography(items[0][0][:3], items[0][1][:3])             # fewer than 4 pairs


def test_step_equals_fit_then_subtract_and_renders():
    from mavflow import _lib
    W, H, B = 97, 71, 3
    rng = np.random.default_rng(5)
    coords = np.c_[rng.integers(5, W - 5, 200), rng.integers(5, H - 5, 200)]
    yy, xx = np.mgrid[0:H, 0:W]
    flows = np.stack([np.stack([0.01 * xx - 0.3 + 0.002 * yy, -0.008 * yy + 0.2], axis=-1) for _ in range(B)]).astype(np.float32)
    flows += rng.normal(0, 0.05, flows.shape).astype(np.float32)
    flows[0, 30:45, 50:66] += np.float32(6.0)
    flows[1, ..., 0], flows[1, ..., 1] = 7.0 - xx, 9.0 - yy          # every pair of item 1 lands on (7, 9): no homography
    flows[2, 5:20, 8:30] -= np.float32(4.0)
    with _ctx(W, H, B) as ctx:
        Hh, okh = ctx.flow_homography(flows, coords)
        assert okh.tolist() == [1, 0, 1]
        for b in range(B):
            He, oke = R.find_homography(coords.astype(np.float64), R.coords_new(coords, flows[b]))
            assert oke == int(okh[b]) and Hh[b].tobytes() == He.tobytes(), b
        n0 = W * H
        bufs = dict(flow=ctx.alloc(flows.nbytes).upload(flows), res=ctx.alloc(B * _lib.MOTION_DTYPE.itemsize), H=ctx.alloc(72 * B), ok=ctx.alloc(4 * B),
                    gray=ctx.alloc(n0 * B))
        for optimize in (False, True):
            host = ctx.global_motion(flows, Hh, optimize=optimize, outputs=("warped", "gray"))
            ctx.global_motion_step(bufs["flow"].ptr, coords, B, bufs["res"].ptr, optimize=optimize, H_ptr=bufs["H"].ptr, ok_ptr=bufs["ok"].ptr,
                                   gray_ptr=bufs["gray"].ptr)
            res = bufs["res"].download(_lib.MOTION_DTYPE, (B,))
            assert bufs["H"].download(np.float64, (B, 3, 3)).tobytes() == Hh.tobytes() and bufs["ok"].download(np.int32, (B,)).tolist() == [1, 0, 1]
            gray = bufs["gray"].download(np.uint8, (B, H, W))
            for b in (0, 2):
                assert res[b].tobytes() == host["results"][b].tobytes() and np.array_equal(gray[b], host["gray"][b]), (optimize, b)
                check_record(res[b], expected_record(R.subtract(flows[b], Hh[b])["gray"], R.subtract(flows[b], Hh[b]), optimize), (optimize, b))
            assert res[1].tobytes() == bytes(_lib.MOTION_DTYPE.itemsize)             # the failed item: an all-zero record
        # the two renderings of what the step left resident: flow_to_color of the restated fields (taken first: flow_to_color is a
        # host call of its own, after which nothing of the step is resident any more)
        subs = {b: R.subtract(flows[b], Hh[b]) for b in (0, 2)}
        refs = {b: (ctx.flow_to_color(subs[b]["warped"])[0], ctx.flow_to_color(subs[b]["global_motion"])[0]) for b in (0, 2)}
        ctx.global_motion_step(bufs["flow"].ptr, coords, B, bufs["res"].ptr)
        imgs = ctx.render_last_global_motion(B)
        for b in (0, 2):
            assert np.array_equal(imgs["warped"][b], refs[b][0]) and np.array_equal(imgs["global"][b], refs[b][1]), b
        assert set(ctx.render_last_global_motion(B, images=("global",))) == {"global"}
        ctx.flow_to_color(flows[:1])
        with pytest.raises(_lib.MavflowError):                # a later host call may have overwritten the flow
            ctx.render_last_global_motion(B)
        for buf in bufs.values():
            buf.free()


def _processor(ds, **kw):
    from mavflow.processor import Processor
    from mavflow.run_config import RunConfig
    return Processor(RunConfig(logging.getLogger("t"), ds, "", False, False, False, True, False, False, "FLOW_FOE_CLUSTERING"), **kw)


def _restated_frame(coords, flow, optimize):
    He, oke = R.find_homography(coords.astype(np.float64), R.coords_new(coords, flow))
    assert oke == 1
    sub = R.subtract(flow, He)
    return He, sub, expected_record(sub["gray"], sub, optimize)


@pytest.mark.parametrize("use_farneback", [False, True], ids=["host_flow", "device_flow"])
@pytest.mark.parametrize("optimize", [False, True], ids=["plain", "optimized"])
def test_detector_and_processor_equal_the_restated_chain(tmp_path, use_farneback, optimize):
    from mavflow import frame_source, utils
    from mavflow.detector import Detector
    from mavflow.processor import SyntheticDataset
    W, H, N = 160, 120, 6
    np.random.seed(17)
    ds = SyntheticDataset(W=W, H=H, N=N, use_farneback=use_farneback)
    p = _processor(ds, processed_path=str(tmp_path / "processed"), algorithm=Detector.Algorithm.HOMOGRAPHY)
    p.detector.use_optimization = optimize
    coords = p.detector.coords
    det = None
    try:
        assert p.run_detection() == {}
        assert sorted(p.detection_windows) == list(range(N - 1)) == sorted(p.detection_iou)
        det = Detector(ds, Detector.Algorithm.HOMOGRAPHY)
        det.coords, det.sample_x, det.sample_y = coords, coords[:, 0], coords[:, 1]
        det.use_optimization = optimize
        for i in range(N - 1):
            handle = ds.get_flow_uv(i)
            flow = np.array(handle, dtype=np.float32)
            He, sub, exp = _restated_frame(coords, flow, optimize)
            x, y, w, h = exp["opt_window"]
            win = p.detection_windows[i]
            assert (win.get_left(), win.get_top(), win.get_right(), win.get_bottom()) == (x, y, x + w, y + h), i
            assert p.detection_iou[i] == utils.Rectangle.calculate_iou(utils.Rectangle.from_points((x, y), (x + w, y + h)), ds.ground_truth[0])
            png = frame_source.imread(str(tmp_path / "processed" / f"image_{i:05d}.png"))
            assert png.shape == (H, W, 3) and all(np.array_equal(png[..., c], sub["gray"]) for c in range(3)), i
            # the two Detector calls on the same frame: a host array, and (with Farneback) the seam's device handle
            for fl in ([flow, ds.get_flow_uv(i)] if use_farneback else [flow]):
                det.get_transformation_matrix(None, fl)
                assert det.homography.tobytes() == He.tobytes() and det.confidence.shape == (len(coords), 1) and det.confidence.all()
                vis_w, cluster, mag_vis, vis_g = det.flow_vec_subtract(None, fl)
                assert np.asarray(det.flow_uv_warped).tobytes() == sub["warped"].tobytes()
                assert np.asarray(det.flow_uv_warped_mag).tobytes() == sub["mag"].tobytes()
                assert tuple(det.flow_max) == sub["flow_max"] and cluster.shape == (H, W, 3) and np.array_equal(cluster[..., 1], sub["gray"])
                assert np.array_equal(mag_vis, cluster) and det.cluster_vis is cluster
                score, rect, window, amax = det.opt_window
                assert score == exp["window"][0] and (rect.get_left(), rect.get_top(), rect.get_right(), rect.get_bottom()) == (x, y, x + w, y + h)
                assert det.iou == p.detection_iou[i]
                ctx = _ctx(W, H)
                assert np.array_equal(vis_w, ctx.flow_to_color(sub["warped"])[0]) and np.array_equal(vis_g, ctx.flow_to_color(sub["global_motion"])[0])
                ctx.close()
        assert p.detector.homography.tobytes() == He.tobytes() and tuple(p.detector.flow_max) == sub["flow_max"]
    finally:
        if det is not None:
            det._free_dev_buffers()
        p.release()


def test_float64_field_takes_the_host_arithmetic():
    from mavflow.detector import Detector

    class DS:
        capture_size = (97, 71)
        ground_truth: list = []

    np.random.seed(2)
    det = Detector(DS(), Detector.Algorithm.AFFINE)
    det.aff = G["a64_M"]
    flow = np.random.default_rng(3).normal(0, 2, (71, 97, 2))
    det.flow_vec_subtract(None, flow)
    sub = R.subtract(flow, det.aff)
    assert det.flow_uv_warped.dtype == np.float64 and det.flow_uv_warped.tobytes() == sub["warped"].tobytes()
    assert np.array_equal(det.cluster_vis[..., 0], sub["gray"]) and tuple(det.flow_max) == sub["flow_max"]
    assert det.opt_window[0] == po.analyze_pyramid(sub["gray"])[0]
