"""The device PNG encoder (mav_png_encode / mav_last_render_png / mav_last_overlay_png, Processor(png_encoder="device")) on the MI355X.

Every expected value is the input image itself: a file must inflate with zlib (no trailing bytes, the right length), decode with
frame_source.decode_png -- and with PIL where it is installed -- to exactly the pixels that went in.  Size conditions (derived in
DESIGN.md "PNG encoder"): never above mav_png_bound (<= 1.01 raw + 1024); a constant image within raw / 50 + 256 bytes per segment
(a literal-only coder needs raw / 8); the three result images of 1080p synthetic frames together no larger than the host encoder's
files of the same arrays."""
import struct
import zlib

import numpy as np
import pytest

from mavflow import synth
from mavflow.frame_source import PNG_MAGIC, decode_png, encode_png

pytestmark = pytest.mark.gpu

SEG = 24576                                                   # bytes of scanline stream per independent segment (mav_png_bound's formula)
SIZES = [(1, 1), (1, 7), (3, 2), (333, 227), (640, 480), (1920, 1080), (3840, 2160)]
CASES = [(W, H, C) for W, H in SIZES for C in (1, 3, 4) if (W, H) != (3840, 2160) or C == 3]      # 4K: 3 channels only
CONTENTS = ("zero", "c255", "c7", "noise", "checker", "hramp", "vramp", "synth")


def _ctx(W, H, B=1):
    from mavflow import _lib
    return _lib.Context(W, H, B)


def _content(name, W, H, C):
    y, x = np.mgrid[0:H, 0:W]
    if name in ("zero", "c255", "c7"):
        g = np.full((H, W, C), {"zero": 0, "c255": 255, "c7": 7}[name], np.uint8)
    elif name == "noise":
        g = np.random.default_rng(W * 31 + H * 7 + C).integers(0, 256, (H, W, C), dtype=np.uint8)
    elif name == "checker":
        g = np.repeat((((x + y) & 1) * 255).astype(np.uint8)[..., None], C, axis=2)
    elif name == "hramp":
        g = np.stack([((x * (c + 1)) // (1 + c // 2)) % 256 for c in range(C)], -1).astype(np.uint8)
    elif name == "vramp":
        g = np.stack([(y * (c + 1) + 3 * c) % 256 for c in range(C)], -1).astype(np.uint8)
    elif name == "synth":
        f = synth.make_pair(W, H, 3)[0]
        g = np.stack([np.roll(f, 5 * c, axis=1) for c in range(C)], -1)      # channels that differ: a B <-> R mix-up shows
    else:
        raise KeyError(name)
    return np.ascontiguousarray(g)


def _idat(png):
    """(W, H, colour type, the IDAT bytes) of a file with exactly IHDR, one IDAT, IEND"""
    assert png[:8] == PNG_MAGIC
    pos, chunks = 8, []
    while pos < len(png):
        (n,) = struct.unpack(">I", png[pos:pos + 4])
        chunks.append((png[pos + 4:pos + 8], png[pos + 8:pos + 8 + n]))
        pos += 12 + n
    assert pos == len(png) and [k for k, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"]
    W, H, depth, ctype, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, comp, filt, lace) == (8, 0, 0, 0)
    return W, H, ctype, chunks[1][1]


def _check_file(png, img, tag, pil=None):
    """`png` is a complete PNG file of `img` ((H, W, C) u8, C = 1 gray / 3 BGR / 4 BGRA); returns the zlib stream's size"""
    H, W, C = img.shape
    w, h, ctype, z = _idat(png)
    assert (w, h, ctype) == (W, H, {1: 0, 3: 2, 4: 6}[C]), tag
    d = zlib.decompressobj()
    raw = d.decompress(z)
    assert d.eof and d.unused_data == b"" and d.unconsumed_tail == b"", f"{tag}: the zlib stream does not end where the IDAT chunk ends"
    assert len(raw) == H * (1 + W * C), tag
    assert zlib.decompress(z) == raw
    px, ct = decode_png(png)
    want = img[:, :, 0] if C == 1 else img[:, :, [2, 1, 0] if C == 3 else [2, 1, 0, 3]]      # the file holds gray / RGB / RGBA
    assert ct == ctype and px.shape == want.shape and np.array_equal(px, want), f"{tag}: decode_png gives other pixels"
    if pil is not None:
        import io
        im = pil.open(io.BytesIO(png))
        assert im.mode == {1: "L", 3: "RGB", 4: "RGBA"}[C], tag
        assert np.array_equal(np.asarray(im), want), f"{tag}: PIL gives other pixels"
    return len(z)


def _bound(W, H, C):
    raw = H * (1 + W * C)
    return raw + 5 * -(-raw // SEG) + 6


@pytest.mark.parametrize("W,H,C", CASES)
def test_lossless_with_every_decoder(mav, W, H, C):
    raw = H * (1 + W * C)
    segments = -(-raw // SEG)
    with _ctx(W, H) as c:
        assert c.lib.mav_png_bound(W, H, C) == _bound(W, H, C) <= 1.01 * raw + 1024
        for name in CONTENTS:
            img = _content(name, W, H, C)
            (png,) = c.png_encode(img[None])
            n = _check_file(png, img, f"{W}x{H}x{C} {name}")
            print(f"{W}x{H}x{C} {name}: raw {raw}, stream {n} ({n / raw:.4f})")
            assert n <= _bound(W, H, C), f"{name}: above mav_png_bound"
            if name in ("zero", "c255", "c7"):
                assert n <= raw / 50 + 256 * segments, f"{name}: {n} bytes for {raw} constant ones: the runs are not used"


@pytest.mark.parametrize("W,H,C", CASES)
def test_lossless_with_pil(mav, W, H, C):
    Image = pytest.importorskip("PIL.Image")
    with _ctx(W, H) as c:
        for name in CONTENTS:
            img = _content(name, W, H, C)
            (png,) = c.png_encode(img[None])
            _check_file(png, img, f"{W}x{H}x{C} {name}", pil=Image)


def _rates(B, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(0.0, 0.02, (B, 3)), rng.uniform(0.02, 0.05, B)


def _bgr_of(gray):
    return np.ascontiguousarray(np.stack([gray, np.roll(gray, 3, axis=-1), 255 - gray], -1))


@pytest.mark.parametrize("W,H,B", [(640, 480, 3), (1920, 1080, 2)])
def test_rendered_images_and_overlays(mav, W, H, B):
    """The loop's own images: render_last's three and overlay_last's frames, through png_encode and through the _png calls; at 1080p
    the three result images together take no more bytes than the host encoder's files of the same arrays."""
    try:
        from PIL import Image
    except ImportError:
        Image = None
    prev, nxt = synth.make_batch(W, H, B, distinct=B)
    smp = np.stack([synth.foe_samples(W, H, b) for b in range(B)])
    omega, dt = _rates(B, W)
    frames = _bgr_of(nxt)
    gts = [(0.55 * W, 0.45 * H)] * B
    with _ctx(W, H, B) as c:
        c.process_batch(prev, nxt, smp, omega=omega, dt=dt, frame0=[b == 0 for b in range(B)])
        imgs = c.render_last(B)
        files = c.render_last_png(B)
        over, wr = c.overlay_last(frames, gts)
        over = np.array(over)
        ofiles, owr = c.overlay_last_png(frames, gts)
        again = c.render_last_png(B, images=("phi",))
        assert set(again) == {"phi"} and again["phi"] == files["phi"]
        assert c.render_last_png(B, images=()) == {}
        separate = {k: c.png_encode(v) for k, v in imgs.items()}         # host-pointer call: ends what render_last may read
        oseparate = c.png_encode(over)
    assert sorted(files) == ["flow", "phi", "result"] and np.array_equal(wr, owr) and wr.dtype == owr.dtype
    dev = host = 0
    for k in ("result", "flow", "phi"):
        assert len(files[k]) == B
        assert files[k] == separate[k], k                                # the same pixels give the same bytes
        for b in range(B):
            _check_file(files[k][b], imgs[k][b], f"{W}x{H} {k} {b}", pil=Image)
        sizes = [len(f) for f in files[k]]                               # whole files on both sides
        hsz = [len(encode_png(imgs[k][b])) for b in range(B)]
        print(f"{W}x{H} {k}: device {sizes}, host {hsz}, ratio {sum(sizes) / sum(hsz):.3f}")
        dev, host = dev + sum(sizes), host + sum(hsz)
    assert ofiles == oseparate
    osz = [_check_file(ofiles[b], over[b], f"{W}x{H} overlay {b}", pil=Image) for b in range(B)]
    ohs = [len(encode_png(over[b])) for b in range(B)]
    print(f"{W}x{H} overlay (textured, reported only): device {osz}, host {ohs}, ratio {sum(osz) / sum(ohs):.3f}")
    assert all(n <= _bound(W, H, 3) for n in osz)
    print(f"{W}x{H} result + flow + phi: device {dev}, host {host}, ratio {dev / host:.3f}")
    if (W, H) == (1920, 1080):
        assert dev <= host


def test_five_images_in_one_call_and_determinism(mav):
    W, H, C = 333, 227, 3
    imgs = np.stack([_content(n, W, H, C) for n in ("synth", "noise", "c7", "hramp", "checker")])
    from mavflow import _lib
    with _ctx(W, H) as c:
        files = c.png_encode(imgs)
        assert c.png_encode(imgs) == files and c.png_encode(imgs[2:4]) == files[2:4]
        # the raw call: index offsets ascending, streams back to back
        out = np.zeros(c.lib.mav_png_bound(W, H, C) * 5, np.uint8)
        index = np.zeros((5, 2), np.uint64)
        _lib.check(c.lib.mav_png_encode(c.h, imgs.ctypes.data, 5, C, out.ctypes.data, out.size, index.ctypes.data))
    assert len(files) == 5 and len(set(files)) == 5
    for k in range(5):
        n = _check_file(files[k], imgs[k], f"image {k}")
        assert int(index[k, 1]) == n and int(index[k, 0]) == (0 if k == 0 else int(index[k - 1].sum()))
        assert out[int(index[k, 0]):int(index[k].sum())].tobytes() == _idat(files[k])[3]
    assert not out[int(index[4].sum()):].any()                            # nothing written behind the last stream


def test_state_and_argument_errors(mav):
    from mavflow import _lib
    W, H, B = 96, 64, 2
    flow = synth.synthetic_flow(W, H, seed=3)[None].repeat(B, 0)
    smp = np.stack([synth.foe_samples(W, H, b) for b in range(B)])
    frames = np.zeros((B, H, W, 3), np.uint8)
    gts = [(10.0, 10.0)] * B
    with _ctx(W, H, B) as c:
        with pytest.raises(_lib.MavflowError):
            c.render_last_png(B)                                         # no detection call precedes
        with pytest.raises(_lib.MavflowError):
            c.overlay_last_png(frames, gts)
        c.detect(flow, smp)
        with pytest.raises(_lib.MavflowError):
            c.render_last_png(1)                                         # the batch differs
        with pytest.raises(_lib.MavflowError):
            c.overlay_last_png(frames[:1], gts[:1])
        assert set(c.render_last_png(B, images=("phi",))) == {"phi"}
        assert len(c.overlay_last_png(frames, gts)[0]) == B
        with pytest.raises(ValueError):
            c.render_last_png(B, images=("nope",))
        with pytest.raises(ValueError):
            c.overlay_last_png(frames, [(np.float64("nan"), 1.0)] * B)
        c.bbox(np.zeros((B, H, W), np.uint8))                            # any other host call may overwrite the staged flow
        with pytest.raises(_lib.MavflowError):
            c.render_last_png(B)
        with pytest.raises(_lib.MavflowError):
            c.overlay_last_png(frames, gts)
        # arguments
        img = np.zeros((1, H, W, 3), np.uint8)
        with pytest.raises(ValueError):
            c.png_encode(np.zeros((1, H, W, 2), np.uint8))               # channels = 2
        with pytest.raises(TypeError):
            c.png_encode(img.astype(np.float32))
        with pytest.raises(ValueError):
            c.png_encode(np.zeros((1, H, W + 1, 3), np.uint8))
        out = np.zeros(c.lib.mav_png_bound(W, H, 3), np.uint8)
        index = np.zeros((1, 2), np.uint64)
        rc = c.lib.mav_png_encode(c.h, img.ctypes.data, 1, 2, out.ctypes.data, out.size, index.ctypes.data)
        assert rc == _lib.MAV_ERR_ARG
        assert c.lib.mav_png_encode(c.h, img.ctypes.data, 0, 3, out.ctypes.data, out.size, index.ctypes.data) == _lib.MAV_ERR_ARG
        assert c.lib.mav_png_encode(c.h, img.ctypes.data, 1, 3, out.ctypes.data, 8, index.ctypes.data) == _lib.MAV_ERR_ARG      # short
        d_img, d_out, d_idx = c.alloc(img.nbytes).upload(img), c.alloc(out.size), c.alloc(16)
        assert c.lib.mav_png_encode_dev(c.h, d_img.ptr, 1, 3, d_out.ptr, out.size - 1, d_idx.ptr) == _lib.MAV_ERR_ARG             # below the bound
        assert c.lib.mav_png_encode_dev(c.h, d_img.ptr, 1, 3, d_out.ptr, out.size, d_idx.ptr) == 0
        c.sync()
        idx = d_idx.download(np.uint64, (1, 2))
        z = d_out.download(np.uint8, (out.size,))[:int(idx[0, 1])].tobytes()
        assert int(idx[0, 0]) == 0 and zlib.decompress(z) == (b"\x01" + bytes(3 * W)) * H
        assert c.lib.mav_png_bound(W, H, 2) == 0 and c.lib.mav_png_bound(0, H, 3) == 0


def test_workspace_is_allocated_by_the_first_encode_and_reported(mav):
    W, H = 320, 240
    with _ctx(W, H) as c:
        before = c.mem_info()["ctx_bytes"]
        c.png_encode(np.zeros((1, H, W, 3), np.uint8))
        after = c.mem_info()["ctx_bytes"]
    raw = H * (1 + 3 * W)
    assert after - before >= -(-raw // SEG) * SEG                         # the segment slots at least, plus this call's staging blocks


def _processor(ds, png_encoder=None, **paths):
    import logging
    from mavflow.processor import Processor
    from mavflow.run_config import RunConfig
    kw = {} if png_encoder is None else dict(png_encoder=png_encoder)
    return Processor(RunConfig(logging.getLogger("t"), ds, "", False, False, False, True, False, False, "FLOW_FOE_CLUSTERING"), **paths, **kw)


@pytest.mark.parametrize("loop", ["run_detection", "run_detection_batched"])
def test_processor_device_encoder_writes_the_same_pictures(mav, tmp_path, loop):
    from mavflow.processor import SyntheticDataset
    W, H, N = 320, 240, 9
    runs = {}
    for enc in (None, "device"):
        root = tmp_path / (enc or "host")
        ds = SyntheticDataset(W, H, N, use_farneback=True, dangle=(0.004, -0.002, 0.001), results_path=str(root / "json"))
        np.random.seed(5)
        p = _processor(ds, enc, images_path=str(root / "img"), processed_path=str(root / "processed"))
        assert p.png_encoder == (enc or "host")
        if loop == "run_detection_batched":
            p.run_detection_batched(batch=8)
        else:
            p.run_detection()
        res = {i: dict(vars(r)) for i, r in p.detection_results.items()}
        p.release()
        runs[enc] = (root, res)
    (hroot, hres), (droot, dres) = runs[None], runs["device"]
    names = sorted(str(q.relative_to(hroot)) for q in hroot.rglob("*") if q.is_file())
    assert names == sorted(str(q.relative_to(droot)) for q in droot.rglob("*") if q.is_file())
    pngs = [n for n in names if n.endswith(".png")]
    assert len(pngs) >= 3 * (N - 1) + 1 and len([n for n in names if n.endswith(".json")]) == N - 1
    differ = 0
    for n in names:
        a, b = (hroot / n).read_bytes(), (droot / n).read_bytes()
        if n.endswith(".json"):
            assert a == b, n
        else:
            pa, pb = decode_png(a), decode_png(b)
            assert pa[1] == pb[1] == 2 and np.array_equal(pa[0], pb[0]), n
            differ += a != b
    assert differ == len(pngs)                                            # the device's files really are its own
    assert hres.keys() == dres.keys()
    for i in hres:
        assert repr(hres[i]) == repr(dres[i]), i


def test_processor_refuses_an_unknown_encoder(mav):
    from mavflow.processor import SyntheticDataset
    with pytest.raises(ValueError):
        _processor(SyntheticDataset(64, 48, 3), "gpu")
