"""The result images (mav_render / mav_last_render / mav_flow_to_color / mav_colormap_jet) on the MI355X against the reference's own
colour wheel (tests/golden/colorwheel.png) and the numpy restatement (tests/render_ref.py) composed with oracle/foe_oracle.py.

Bars: the colour wheel byte for byte; result and phi images exact; flow colour exact except at pixels where moving arctan2 by
+-2 ulps changes the restatement's byte (numpy's arctan2 is libm / a SIMD routine, the device's is ocml's), at most 1e-4 of them."""
import numpy as np
import pytest

import render_ref as rr
from oracle import foe_oracle as fo
from mavflow import synth

pytestmark = pytest.mark.gpu


def _ctx(W, H, B):
    from mavflow import _lib
    return _lib.Context(W, H, B)


def test_colorwheel_is_the_reference_image(mav):
    want = rr.decode_rgb(rr.COLORWHEEL_PNG)[:, :, ::-1]
    field = rr.colorwheel_field()
    flow32 = field.astype(np.float32)
    assert np.array_equal(flow32.astype(np.float64), field)          # integers: the float32 field is the same field
    with _ctx(250, 250, 1) as c:
        # a frame i >= 1 with zero rotation and dt = 1: derotate subtracts zeros in double, flow_to_color runs in double
        got = c.render(flow32, foe=(125.0, 125.0), omega=np.zeros(3), dt=1.0, images=("flow",))
        assert set(got) == {"flow"}
        assert np.array_equal(got["flow"][0], want), int((got["flow"][0] != want).any(axis=2).sum())
        promoted = c.render(flow32, foe=(125.0, 125.0), images=("flow",))["flow"][0]       # no rates: the promoted field
        assert np.array_equal(promoted, want)
        assert np.array_equal(c.flow_to_color(field)[0], want)                            # get_flow_vis of the float64 field


def _planted(W, H):
    """A flow whose phi sweeps 0..180 degrees along x (every LUT entry), zero-flow pixels (phi 90) and NaN-phi pixels (phi 0)."""
    foe = (W / 2 + 0.25, H / 2 - 0.5)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    dx, dy = xs - foe[0], ys - foe[1]
    r = np.hypot(dx, dy)
    theta = (xs + 0.37 * ys) / (W - 1) * np.pi                         # angle between the flow and p - FoE
    mag = 0.3 + 4.0 * ((ys % 7) / 6.0)
    c, s = np.cos(theta), np.sin(theta)
    u = (c * dx - s * dy) / r * mag
    v = (s * dx + c * dy) / r * mag
    flow = np.stack([u, v], axis=-1).astype(np.float32)
    flow[H // 3, ::5] = 0.0
    flow[2 * H // 3, 3::11] = np.nan
    return flow, foe


@pytest.mark.parametrize("frame0", [False, True])
def test_planted_phi_covers_every_lut_entry(mav, frame0):
    W, H = 512, 96
    flow, foe = _planted(W, H)
    lut = rr.jet_lut()
    sky = np.zeros((H, W), np.uint8)
    sky[:8] = 1
    with _ctx(W, H, 1) as c:
        got = c.render(flow, foe, sky=sky, frame0=[frame0] if frame0 else None, images=("result", "phi"))
        if frame0:
            phi, mf, _, _ = c.phi_mask(flow, foe, sky=sky)            # float32 flow: the frame-0 float32 arithmetic
        else:
            phi, mf, _, _ = c.phi_mask(flow.astype(np.float64), foe, sky=sky)
    g = rr.to_int(phi[0], max_value=180.0)
    assert len(np.unique(g)) == 256
    assert np.isnan(flow).any() and (phi[0][np.isnan(flow[..., 0])] == 0).all()
    assert np.array_equal(got["phi"][0], rr.phi_image(phi[0], lut))
    assert np.array_equal(got["result"][0], rr.result_image(mf[0]))
    assert mf[0].any()


def _rates(B, seed):
    rng = np.random.default_rng(seed)
    omega = rng.normal(0.0, 0.02, (B, 3))
    dt = rng.uniform(0.02, 0.05, B)
    return omega, dt


def _expected(flow, phi, mask_fixed, omega, dt, frame0):
    """the three images of one pair from the restatement: derotation from the oracle, phi and the fixed mask as the device
    computed them (pinned to the oracle by test_gpu_detect / test_frame0)"""
    der = fo.derotate(flow, omega, dt, 0 if frame0 else 1)
    ph = phi.astype(np.float32) if frame0 else phi                    # a frame-0 pair's phi is float32, returned widened
    return dict(result=rr.result_image(mask_fixed), phi=rr.phi_image(ph), flow=rr.flow_to_color(der)), der


def _check_flow_image(got, der, tag):
    want = rr.flow_to_color(der)
    diff = (got != want).any(axis=2)
    n = int(diff.sum())
    if n:
        sens = rr.atan2_sensitive(der, 2)
        assert not (diff & ~sens).any(), f"{tag}: {int((diff & ~sens).sum())} pixels differ outside the arctan2 band"
    print(f"{tag}: flow image differs at {n} of {diff.size} pixels (all inside the +-2 ulp arctan2 band)")
    assert n <= 1e-4 * diff.size
    return n


@pytest.mark.parametrize("W,H,B", [(640, 480, 4), (1920, 1080, 2)])
def test_process_batch_images_match_the_restatement(mav, W, H, B):
    prev, nxt = synth.make_batch(W, H, B, distinct=B)
    smp = np.stack([synth.foe_samples(W, H, b) for b in range(B)])
    omega, dt = _rates(B, W)
    frame0 = np.array([b % 2 == 0 for b in range(B)])
    sky = np.zeros((B, H, W), np.uint8)
    sky[:, : H // 10] = 1
    with _ctx(W, H, B) as c:
        out = c.process_batch(prev, nxt, smp, omega=omega, dt=dt, sky=sky, frame0=frame0, want_phi=True)
        last = c.render_last(B)
        foe = np.stack([out["results"][b]["foe"] for b in range(B)])
        fresh = c.render(out["flow"], foe, omega=omega, dt=dt, sky=sky, frame0=frame0)
    for k in ("result", "flow", "phi"):
        assert np.array_equal(last[k], fresh[k]), k
    for b in range(B):
        want, der = _expected(out["flow"][b], out["phi"][b], out["mask_fixed"][b], omega[b], dt[b], frame0[b])
        assert np.array_equal(last["result"][b], want["result"]), b
        assert np.array_equal(last["phi"][b], want["phi"]), b
        _check_flow_image(last["flow"][b], der, f"{W}x{H} pair {b} frame0={bool(frame0[b])}")
        assert last["result"][b].any() or not out["mask_fixed"][b].any()


def test_render_last_after_the_device_path_equals_render(mav):
    W, H, B = 320, 240, 3
    from mavflow import _lib
    prev, nxt = synth.make_batch(W, H, B, distinct=B)
    smp = np.stack([synth.foe_samples(W, H, b) for b in range(B)])
    omega, dt = _rates(B, 7)
    frame0 = np.array([1, 0, 0], np.uint8)
    sky = np.zeros((B, H, W), np.uint8)
    sky[:, :20] = 1
    with _ctx(W, H, B) as c:
        bufs = [c.alloc(a.nbytes).upload(a) for a in (prev, nxt, smp, omega, dt, frame0, sky)]
        d_res = c.alloc(B * _lib.RESULT_DTYPE.itemsize)
        d_prev, d_next, d_smp, d_om, d_dt, d_f0, d_sky = (b.ptr for b in bufs)
        c.process_batch_dev(d_prev, d_next, d_smp, B, d_res.ptr, omega_ptr=d_om, dt_ptr=d_dt, sky_ptr=d_sky, frame0_ptr=d_f0)
        last = c.render_last(B)                         # the flow stayed in the context's workspace (flow_ptr=None)
        res = d_res.download(_lib.RESULT_DTYPE, (B,))
        flow = np.stack([c.last_flow(b) for b in range(B)])
        foe = np.stack([res[b]["foe"] for b in range(B)])
        fresh = c.render(flow, foe, omega=omega, dt=dt, sky=sky, frame0=frame0)
        # and render_dev on the same device buffers
        d_flow = c.alloc(flow.nbytes).upload(flow)
        d_foe = c.alloc(foe.nbytes).upload(np.ascontiguousarray(foe))
        d_img = [c.alloc(B * H * W * 3) for _ in range(3)]
        c.render_dev(d_flow.ptr, d_foe.ptr, B, *(d.ptr for d in d_img), omega_ptr=d_om, dt_ptr=d_dt, frame0_ptr=d_f0, sky_ptr=d_sky)
        c.sync()
        dev = {k: d.download(np.uint8, (B, H, W, 3)) for k, d in zip(("result", "flow", "phi"), d_img)}
    for k in ("result", "flow", "phi"):
        assert np.array_equal(last[k], fresh[k]), k
        assert np.array_equal(dev[k], fresh[k]), k


def test_optional_outputs_and_errors(mav):
    from mavflow import _lib
    W, H, B = 96, 64, 2
    flow = synth.synthetic_flow(W, H, seed=3)[None].repeat(B, 0)
    foe = np.array([[40.0, 30.0], [50.5, 20.0]])
    with _ctx(W, H, B) as c:
        full = c.render(flow, foe)
        for k in ("result", "flow", "phi"):
            one = c.render(flow, foe, images=(k,))
            assert set(one) == {k} and np.array_equal(one[k], full[k])
        assert c.render(flow, foe, images=()) == {}
        with pytest.raises(ValueError):
            c.render(flow[:, :-1], foe)                                  # wrong frame size
        with pytest.raises(ValueError):
            c.render(np.concatenate([flow, flow]), np.concatenate([foe, foe]))    # batch above max_batch
        with pytest.raises(ValueError):
            c.render(flow, foe, images=("nope",))
        with pytest.raises(_lib.MavflowError):
            c.render_last(B)                                             # no detection call precedes
        smp = np.stack([synth.foe_samples(W, H, b) for b in range(B)])
        c.detect(flow, smp)
        with pytest.raises(_lib.MavflowError):
            c.render_last(1)                                             # the batch differs
        assert set(c.render_last(B, images=("phi",))) == {"phi"}
        c.bbox(np.zeros((B, H, W), np.uint8))                            # any other host call may overwrite the staged flow
        with pytest.raises(_lib.MavflowError):
            c.render_last(B)


def test_im_helpers_are_backed_by_the_kernels(mav):
    from mavflow import im_helpers
    field = rr.colorwheel_field()
    want = rr.decode_rgb(rr.COLORWHEEL_PNG)[:, :, ::-1]
    assert np.array_equal(im_helpers.get_flow_vis(field), want)
    f32 = synth.synthetic_flow(64, 48, seed=5)
    assert np.array_equal(im_helpers.get_flow_vis(f32), rr.flow_to_color(f32)) or \
        not ((im_helpers.get_flow_vis(f32) != rr.flow_to_color(f32)).any(axis=2) & ~rr.atan2_sensitive(f32)).any()
    phi = np.linspace(0.0, 180.0, 64 * 48).reshape(48, 64)
    lut = rr.jet_lut()
    rgb = im_helpers.to_rgb(phi, max_value=180.0)
    assert np.array_equal(im_helpers.apply_colormap(rgb), rr.phi_image(phi, lut))
    g = np.arange(256, dtype=np.uint8).reshape(16, 16)
    assert np.array_equal(im_helpers.apply_colormap(g), lut[g])


def _processor(ds, images_path=None):
    import logging
    from mavflow.processor import Processor
    from mavflow.run_config import RunConfig
    return Processor(RunConfig(logging.getLogger("t"), ds, "", False, False, False, True, False, False, "FLOW_FOE_CLUSTERING"),
                     images_path=images_path)


def _png(path):
    from mavflow.frame_source import decode_png
    with open(path, "rb") as f:
        px, ctype = decode_png(f.read())
    assert ctype == 2
    return px[:, :, ::-1]                                                # the file holds RGB: the BGR array reversed


def test_processor_writes_the_three_images_per_frame(mav, tmp_path):
    """All three loops write 3 x (N - 1) PNG files, the same pixels in each loop (the fast loops render behind their steps, the staged
    loop through get_flow_vis / apply_colormap / to_rgb), equal to Context.render of the frame's flow; without images_path no PNG
    appears and the JSON files are those of a run with images."""
    from mavflow import _lib
    from mavflow.processor import IMAGE_DIRS, SyntheticDataset
    W, H, N = 320, 240, 6
    dangle = (0.004, -0.002, 0.001)
    files = {}
    for loop in ("run_detection_staged", "run_detection", "run_detection_batched", "plain"):
        ds = SyntheticDataset(W, H, N, use_farneback=True, dangle=dangle, results_path=str(tmp_path / loop / "json"))
        np.random.seed(5)
        p = _processor(ds, None if loop == "plain" else str(tmp_path / loop / "img"))
        if loop == "run_detection_batched":
            p.run_detection_batched(batch=2)
        else:
            getattr(p, "run_detection" if loop == "plain" else loop)()
        if loop == "run_detection_staged":
            foes = {i: p.detection_results[i].foe_dense for i in range(N - 1)}
        p.release()
        pngs = sorted(str(q.relative_to(tmp_path / loop)) for q in tmp_path.joinpath(loop).rglob("*.png"))
        if loop == "plain":
            assert pngs == []
        else:
            assert pngs == sorted(f"img/{d}/image_{i:05d}.png" for d in IMAGE_DIRS.values() for i in range(N - 1))
            files[loop] = {(k, i): _png(tmp_path / loop / "img" / d / f"image_{i:05d}.png") for k, d in IMAGE_DIRS.items() for i in range(N - 1)}
        json_files = sorted((tmp_path / loop / "json").glob("*.json"))
        assert len(json_files) == N - 1
        if loop != "run_detection_staged":
            for f in json_files:
                assert f.read_text() == (tmp_path / "run_detection_staged" / "json" / f.name).read_text()
    base = files["run_detection_staged"]
    for loop in ("run_detection", "run_detection_batched"):
        for key, img in files[loop].items():
            assert np.array_equal(img, base[key]), (loop, key)
    # against Context.render of the frames' flow (the same Farneback field, the dataset's rates)
    ds = SyntheticDataset(W, H, N, use_farneback=True, dangle=dangle)
    with _lib.Context(W, H, 1) as c:
        for i in range(N - 1):
            flow = np.ascontiguousarray(np.asarray(ds.get_flow_uv(i)), np.float32)
            dt = ds.get_delta_time(i)
            omega = np.asarray(ds.get_angular_difference(i - 1, i), np.float64) / dt if i >= 1 else np.zeros(3)
            sky = ds.get_sky_segmentation(i)
            got = c.render(flow, foes[i], omega=omega, dt=dt if i >= 1 else 1.0, sky=sky, frame0=[i < 1])
            for k in IMAGE_DIRS:
                assert np.array_equal(got[k][0], base[(k, i)]), (k, i)
    ds.release()
