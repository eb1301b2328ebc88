"""The processed.mp4 frame (mav_overlay / mav_overlay_dev / mav_last_overlay, Processor(processed_path=...)) on the MI355X against the
numpy restatement tests/overlay_ref.py: byte for byte, with the write flag."""
import numpy as np
import pytest

import overlay_ref as ov
from mavflow import synth

pytestmark = pytest.mark.gpu


def _ctx(W, H, B):
    from mavflow import _lib
    return _lib.Context(W, H, B)


def _planted(W, H):
    """Centres: middle, on each border and corner, 1 - 10 px outside, fully outside, +-1e9 and just beyond, negative fractional."""
    c = [(W / 2, H / 2), (0.0, H / 2), (W - 1.0, H / 2), (W / 2, 0.0), (W / 2, H - 1.0), (0.0, 0.0), (W - 1.0, H - 1.0),
         (-0.7, H / 3), (W / 3, -0.7), (-0.7, -0.99), (-11.0, H / 2), (W + 10.0, H / 2), (W / 2, -50.0), (-30.5, -30.5),
         (1e9, 1e9), (-1e9, H / 2), (1e9 + 1, H / 2), (W / 2, -1e9 - 1e3), (np.inf, 0.0)]
    c += [(-float(d), H / 2 + d) for d in range(1, 11)] + [(W - 1.0 + d, H - 1.0 + d) for d in range(1, 11)]
    return c


def _frames(W, H, B, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)


def _masks(W, H, B, seed):
    rng = np.random.default_rng(seed + 1)
    m = rng.random((B, H, W)) < 0.3
    m[0] = False                                                       # empty
    if B > 1:
        m[1] = True                                                    # full
    return m


@pytest.mark.parametrize("W,H", [(1, 1), (17, 9), (58, 174), (320, 240), (1280, 720), (1920, 1080)])
def test_device_equals_the_restatement(mav, W, H):
    cs = _planted(W, H)
    B = 8
    rng = np.random.default_rng(W * 7 + H)
    with _ctx(W, H, B) as c:
        for k0 in range(0, len(cs), B):
            foe = [cs[(k0 + b) % len(cs)] for b in range(B)]
            gt = [cs[(k0 + b + 3) % len(cs)] for b in range(B)]
            if W > 20:                                               # one pair with the two discs overlapping: white over green
                gt[-1] = (foe[-1][0] + 4.6, foe[-1][1] - 3.2) if abs(foe[-1][0]) < 1e8 else (W / 2, H / 2)
            frames = _frames(W, H, B, k0)
            masks = _masks(W, H, B, k0) if k0 % 2 == 0 else rng.random((B, H, W)) < 0.001
            keep = frames.copy()
            got, written = c.overlay(frames, masks, foe, gt)
            want, wflag = ov.overlay_batch(frames, masks, foe, gt)
            assert np.array_equal(frames, keep)
            for b in range(B):
                assert np.array_equal(got[b], want[b]), (W, H, foe[b], gt[b], int((got[b] != want[b]).any(axis=2).sum()))
            assert np.array_equal(written, wflag), (W, H, foe, gt)


def test_written_flag_and_radius(mav):
    W, H, B = 64, 48, 4
    frames = _frames(W, H, B, 3)
    masks = np.zeros((B, H, W), bool)
    masks[3, 10, 10] = True
    foe = [(-11.0, 10.0), (-10.0, 10.0), (1e9 + 1, 0.0), (W + 40.0, -40.0)]
    gt = [(W / 2, H + 9.5), (np.nan, 0.0), (np.nan, np.nan), (W / 2, H + 11.0)]     # H + 9: one pixel on the last row
    with _ctx(W, H, B) as c:
        got, written = c.overlay(frames, masks, foe, gt)
        assert written.tolist() == [True, True, False, True]
        want, wflag = ov.overlay_batch(frames, masks, foe, gt)
        assert np.array_equal(got, want) and written.tolist() == wflag.tolist()
        assert np.array_equal(got[2], frames[2])                     # nothing drawn, nothing masked: the frame itself
        for r in (0, 1, 3, 25):
            got, written = c.overlay(frames, masks, [(20.3, 17.8)] * B, [(40.0, 30.0)] * B, radius=r)
            want, wflag = ov.overlay_batch(frames, masks, [(20.3, 17.8)] * B, [(40.0, 30.0)] * B, r)
            assert np.array_equal(got, want) and np.array_equal(written, wflag), r


def test_overlay_last_after_process_batch(mav):
    W, H, B = 640, 480, 4
    prev, nxt = synth.make_batch(W, H, B, distinct=B)
    smp = np.stack([synth.foe_samples(W, H, b) for b in range(B)])
    rng = np.random.default_rng(5)
    omega, dt = rng.normal(0.0, 0.02, (B, 3)), rng.uniform(0.02, 0.05, B)
    frame0 = np.array([1, 0, 0, 1], np.uint8)                        # frame-0 pairs among them
    frames = _frames(W, H, B, 11)
    gt = [(0.55 * W, 0.45 * H), (-0.7, 3.0), (np.nan, 1.0), (W + 5.0, H / 2)]
    with _ctx(W, H, B) as c:
        out = c.process_batch(prev, nxt, smp, omega=omega, dt=dt, frame0=frame0)
        last, wl = c.overlay_last(frames, gt)
        foe = [tuple(out["results"][b]["foe"]) for b in range(B)]
        fresh, wf = c.overlay(frames, out["mask_fixed"], foe, gt)
    assert np.array_equal(last, fresh) and np.array_equal(wl, wf)
    want, ww = ov.overlay_batch(frames, out["mask_fixed"], foe, gt)
    assert np.array_equal(last, want) and np.array_equal(wl, ww)
    assert any(out["mask_fixed"][b].any() for b in range(B))


def test_overlay_last_after_a_frame_step_and_overlay_dev(mav):
    from mavflow import pipeline
    W, H, B = 320, 240, 3
    prev, nxt = synth.make_batch(W, H, B, distinct=B)
    smp = np.stack([synth.foe_samples(W, H, b) for b in range(B)])
    frames = _frames(W, H, B, 21)
    gt = [(0.5 * W, 0.5 * H), (10.2, -3.0), (W - 2.0, H - 2.0)]
    with _ctx(W, H, B) as c:
        pipe = pipeline.LanedPipeline([c], B)
        try:
            t = pipe.submit(smp, prev=list(prev), nxt=list(nxt), frame0=[True, False, False])
            out = pipe.collect(t)
            last, wl = c.overlay_last(frames, gt)
            masks = np.stack([np.asarray(m) for m in out["mask_fixed"]])
            foe = np.stack([out["results"][b]["foe"] for b in range(B)])
        finally:
            pipe.close()
        fresh, wf = c.overlay(frames, masks, [tuple(f) for f in foe], gt)
        # mav_overlay_dev on device buffers
        d = {k: c.alloc(a.nbytes).upload(np.ascontiguousarray(a)) for k, a in
             dict(frames=frames, mask=masks.astype(np.uint8), foe=foe, gt=np.array(gt, np.float64)).items()}
        d_out, d_w = c.alloc(frames.nbytes), c.alloc(B)
        c.overlay_dev(d["frames"].ptr, d["mask"].ptr, d["foe"].ptr, d["gt"].ptr, B, d_out.ptr, d_w.ptr)
        c.sync()
        dev, dw = d_out.download(np.uint8, frames.shape), d_w.download(np.uint8, (B,))
    want, ww = ov.overlay_batch(frames, masks, [tuple(f) for f in foe], gt)
    for got, w in ((last, wl), (fresh, wf), (dev, dw.astype(bool))):
        assert np.array_equal(got, want) and np.array_equal(w, ww)


def test_errors(mav):
    import ctypes as C
    from mavflow import _lib
    W, H, B = 32, 24, 2
    frames = _frames(W, H, B, 1)
    masks = np.zeros((B, H, W), bool)
    foe = [(5.0, 5.0), (6.0, 6.0)]
    with _ctx(W, H, B) as c:
        with pytest.raises(_lib.MavflowError):
            c.overlay_last(frames, foe)                                # no detection call precedes: MAV_ERR_STATE
        lib, out, wr = c.lib, np.empty((B, H, W, 3), np.uint8), np.empty(B, np.uint8)
        fo = np.array(foe, np.float64)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        assert lib.mav_last_overlay(c.h, p(frames), p(fo), B, 10, p(out), p(wr)) == _lib.MAV_ERR_STATE
        mk = masks.astype(np.uint8)
        assert lib.mav_overlay(c.h, None, p(mk), p(fo), p(fo), B, 10, p(out), p(wr)) == _lib.MAV_ERR_ARG
        assert lib.mav_overlay(c.h, p(frames), p(mk), p(fo), p(fo), B, 10, p(out), None) == _lib.MAV_ERR_ARG
        assert lib.mav_overlay(c.h, p(frames), p(mk), p(fo), p(fo), B + 1, 10, p(out), p(wr)) == _lib.MAV_ERR_ARG
        assert lib.mav_overlay(c.h, p(frames), p(mk), p(fo), p(fo), 0, 10, p(out), p(wr)) == _lib.MAV_ERR_ARG
        assert lib.mav_overlay(c.h, p(frames), p(mk), p(fo), p(fo), B, -1, p(out), p(wr)) == _lib.MAV_ERR_ARG
        assert lib.mav_overlay(c.h, p(frames), p(mk), p(fo), p(fo), B, 4097, p(out), p(wr)) == _lib.MAV_ERR_ARG
        assert lib.mav_overlay_dev(c.h, None, None, None, None, B, 10, None, None) == _lib.MAV_ERR_ARG
        assert lib.mav_last_overlay(None, p(frames), p(fo), B, 10, p(out), p(wr)) == _lib.MAV_ERR_ARG
        assert lib.mav_last_overlay(c.h, p(frames), p(fo), B + 1, 10, p(out), p(wr)) == _lib.MAV_ERR_ARG
        with pytest.raises(ValueError):
            c.overlay(frames, masks, foe, [(float("nan"), 1.0), (2.0, 3.0)])     # int(nan) raises in the reference
        with pytest.raises(ValueError):
            c.overlay(frames[:, :-1], masks, foe, foe)
        flow = synth.synthetic_flow(W, H, seed=3)[None].repeat(B, 0)
        smp = np.stack([synth.foe_samples(W, H, b) for b in range(B)])
        c.detect(flow, smp, want_masks=False)
        with pytest.raises(_lib.MavflowError):
            c.overlay_last(frames, foe)                                # that call kept no fixed mask
        c.detect(flow, smp)
        with pytest.raises(_lib.MavflowError):
            c.overlay_last(frames[:1], foe[:1])                        # the batch differs
        with pytest.raises(ValueError):
            c.overlay_last(frames, [(float("nan"), 1.0), (2.0, 3.0)])
        assert c.overlay_last(frames, foe)[0].shape == (B, H, W, 3)
        c.bbox(np.zeros((B, H, W), np.uint8))                          # any other host call may overwrite the staged mask
        with pytest.raises(_lib.MavflowError):
            c.overlay_last(frames, foe)


def _processor(ds, processed_path=None, images_path=None):
    import logging
    from mavflow.processor import Processor
    from mavflow.run_config import RunConfig
    return Processor(RunConfig(logging.getLogger("t"), ds, "", False, False, False, True, False, False, "FLOW_FOE_CLUSTERING"),
                     images_path=images_path, processed_path=processed_path)


def _png(path):
    from mavflow.frame_source import decode_png
    with open(path, "rb") as f:
        px, ctype = decode_png(f.read())
    assert ctype == 2
    return px[:, :, ::-1]


def test_processor_writes_the_processed_frames(mav, tmp_path):
    """The three loops write the same processed/image_%05d.png files, byte-identical to each other and to the restatement built from
    the loop's own masks, FoEs and frames; without processed_path nothing of it appears and the JSON and result images are unchanged;
    the dataset's frames are untouched."""
    from mavflow.processor import SyntheticDataset
    W, H, N = 320, 240, 6
    dangle = (0.004, -0.002, 0.001)
    files, foes = {}, {}
    for loop in ("run_detection_staged", "run_detection", "run_detection_batched", "plain"):
        ds = SyntheticDataset(W, H, N, use_farneback=True, dangle=dangle, results_path=str(tmp_path / loop / "json"))
        np.random.seed(5)
        proc = None if loop == "plain" else str(tmp_path / loop / "processed")
        p = _processor(ds, proc, str(tmp_path / loop / "img"))
        if loop == "run_detection_batched":
            p.run_detection_batched(batch=2)
        else:
            getattr(p, "run_detection" if loop == "plain" else loop)()
        foes[loop] = {i: p.detection_results[i].foe_dense for i in range(N - 1)}
        p.release()
        for i, a in ds._bgr.items():                                  # the dataset's cached frames are untouched
            assert np.array_equal(a, np.repeat(ds._pair(i)[1][..., None], 3, axis=2)), (loop, i)
        if loop == "plain":
            assert not (tmp_path / loop / "processed").exists()
        else:
            pngs = sorted(q.name for q in (tmp_path / loop / "processed").glob("*.png"))
            files[loop] = {q: (tmp_path / loop / "processed" / q).read_bytes() for q in pngs}
    base = files["run_detection_staged"]
    assert len(base) == N - 1
    for loop in ("run_detection", "run_detection_batched", "plain"):
        assert foes[loop] == foes["run_detection_staged"], loop
    for loop in ("run_detection", "run_detection_batched"):
        assert files[loop] == base, loop
    for loop in ("run_detection", "run_detection_batched", "plain"):
        for f in sorted((tmp_path / "run_detection_staged" / "json").glob("*.json")):
            assert f.read_text() == (tmp_path / loop / "json" / f.name).read_text()
        for q in (tmp_path / "run_detection_staged" / "img").rglob("*.png"):
            assert q.read_bytes() == (tmp_path / loop / "img" / q.relative_to(tmp_path / "run_detection_staged" / "img")).read_bytes()
    # against the restatement: the staged loop's masks recomputed through the reference-named calls
    from mavflow.focus_of_expansion import FocusOfExpansion
    from mavflow.detector import Detector
    ds = SyntheticDataset(W, H, N, use_farneback=True, dangle=dangle)
    det = Detector(ds)
    fo = FocusOfExpansion(det.lucas_kanade)
    for i in range(N - 1):
        der = det.derotate(i - 1, i, np.asarray(ds.get_flow_uv(i)))
        foe = foes["run_detection_staged"][i]
        fixed, _ = fo.get_masks(der, foe, ds.get_sky_segmentation(i))
        want, written = ov.overlay(np.repeat(ds._pair(i)[1][..., None], 3, axis=2), fixed, foe, ds.get_gt_foe(i))
        assert written
        assert np.array_equal(_png(tmp_path / "run_detection_staged" / "processed" / f"image_{i:05d}.png"), want), i
    ds.release()
