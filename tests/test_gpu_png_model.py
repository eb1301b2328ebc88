"""The device PNG encoder against tests/png_device_model.py, byte for byte, on the MI355X.

tests/test_gpu_png.py asks that a file inflates to its image.  Here the IDAT bytes must EQUAL what the CPU model of the format writes for
the same image -- the encoder is all integers, so there is no tolerance -- on the families of tests/png_families.py (code lengths past 15
bits, two-symbol alphabets, every run geometry at every mask-word / wave-part / segment edge, rows longer than a segment, the stored /
coded decision at equality; tests/test_png_device_model_cpu.py proves each reaches its target), on the older suite's contents, in
batches, and across more images than one workspace chunk holds."""
import time
import zlib

import numpy as np
import pytest

import png_device_model as model
import png_families as fam
from mavflow import synth
from test_gpu_png import CASES, CONTENTS, SEG, _bgr_of, _bound, _check_file, _content, _ctx, _idat, _rates

pytestmark = pytest.mark.gpu


def _img3(img):
    return img if img.ndim == 3 else img[:, :, None]


def _by_shape(cases):
    groups = {}
    for name, img in cases:
        groups.setdefault(_img3(img).shape, []).append((name, _img3(img)))
    return groups


def _encode_and_compare(c, name, img):
    """one image alone through Context.png_encode: test_gpu_png's conditions, then equality with the model; returns the file"""
    H, W, C = img.shape
    (png,) = c.png_encode(img[None])
    n = _check_file(png, img, name)
    assert n <= _bound(W, H, C) == c.lib.mav_png_bound(W, H, C), f"{name}: above mav_png_bound"
    want = model.stream_of_image(img)
    got = _idat(png)[3]
    if got != want:
        k = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        raise AssertionError(f"{name}: the device's stream ({len(got)} bytes) and the model's ({len(want)}) part at byte {k}: "
                             f"{got[k:k + 16].hex()} against {want[k:k + 16].hex()}")
    return png


@pytest.mark.parametrize("family", list(fam.FAMILIES))
def test_family_equals_the_model_byte_for_byte(mav, family):
    t0 = time.time()
    for (H, W, C), cases in _by_shape(fam.FAMILIES[family]()).items():
        with _ctx(W, H) as c:
            for name, img in cases:
                png = _encode_and_compare(c, name, img)
                print(f"{family} / {name}: {W}x{H}x{C}, stream {len(_idat(png)[3])} of raw {H * (1 + W * C)}")
    print(f"{family}: {time.time() - t0:.2f} s")


@pytest.mark.parametrize("W,H,C", [k for k in CASES if k[0] * k[1] <= 640 * 480])
def test_existing_contents_equal_the_model_byte_for_byte(mav, W, H, C):
    """the eight contents of test_gpu_png at its sizes up to 640x480, gray, BGR and BGRA: pins the B <-> R load and the RGBA path"""
    with _ctx(W, H) as c:
        for name in CONTENTS:
            _encode_and_compare(c, f"{W}x{H}x{C} {name}", _content(name, W, H, C))


@pytest.mark.parametrize("W,H,B", [(640, 480, 3), (1920, 1080, 2)])
def test_rendered_images_and_overlays_equal_the_model(mav, W, H, B):
    """the loop's own pictures (test_gpu_png.test_rendered_images_and_overlays' inputs) exist only on a GPU: their files, too, are the
    model's bytes; the deepest tree and the most limiter steps among their segments are printed"""
    prev, nxt = synth.make_batch(W, H, B, distinct=B)
    smp = np.stack([synth.foe_samples(W, H, b) for b in range(B)])
    omega, dt = _rates(B, W)
    with _ctx(W, H, B) as c:
        c.process_batch(prev, nxt, smp, omega=omega, dt=dt, frame0=[b == 0 for b in range(B)])
        imgs = c.render_last(B)
        files = c.render_last_png(B)
        over = np.array(c.overlay_last(_bgr_of(nxt), [(0.55 * W, 0.45 * H)] * B)[0])
        ofiles = c.overlay_last_png(_bgr_of(nxt), [(0.55 * W, 0.45 * H)] * B)[0]
    depth = trips = 0
    for name, pics, pngs in [(k, imgs[k], files[k]) for k in ("result", "flow", "phi")] + [("overlay", over, ofiles)]:
        assert len(pngs) == B
        for b in range(B):
            want, infos = model.stream_info(model.scanlines(pics[b]))
            assert _idat(pngs[b])[3] == want, f"{W}x{H} {name} {b}: the device's stream is not the model's"
            depth, trips = max(depth, max(i["depth"] for i in infos)), max(trips, max(i["trips"] for i in infos))
    print(f"{W}x{H} rendered + overlay: deepest unrestricted tree {depth}, most limiter steps {trips}")


@pytest.mark.parametrize("family", [f for f in fam.FAMILIES if f != "runs"])
def test_batches_equal_their_single_images(mav, family):
    """families that share an image size, stacked into one call in two orders: every file is the file of the image encoded alone"""
    stacked = 0
    for (H, W, C), cases in _by_shape(fam.FAMILIES[family]()).items():
        if len(cases) < 2:
            continue
        imgs = [img for _, img in cases]
        with _ctx(W, H) as c:
            single = [c.png_encode(img[None])[0] for img in imgs]
            n = len(imgs)
            for order in [list(range(n)), list(range(n))[::-1]] + ([list(range(1, n)) + [0]] if n > 2 else []):
                files = c.png_encode(np.stack([imgs[k] for k in order]))
                for j, k in enumerate(order):
                    assert files[j] == single[k], f"{family} {cases[k][0]}: place {j} of the stacked call {order} gives another file"
        assert len(set(single)) > 1
        stacked += 1
    assert stacked >= 1


def test_more_images_than_one_workspace_chunk(mav):
    """3840x2160x3: the workspace chunk of 256 MiB holds 10 images, the call has 11.  The second chunk reads the first one's last index
    entry (k_png_index), writes behind it (k_png_compact) and loads its images from an offset."""
    from mavflow import _lib
    W, H, C, count = 3840, 2160, 3, 11
    raw = H * (1 + W * C)
    per = -(-(-(-raw // SEG) * (SEG + 16 + 24) + 16) // 16) * 16            # slots, records and offsets of one image's segments, + 16
    per_chunk = (256 << 20) // per
    assert 1 <= per_chunk < count, f"{per_chunk} images fit one chunk: the call of {count} is not split"
    imgs = np.empty((count, H, W, C), np.uint8)
    for k in range(count):                                                   # a constant and a stripe that moves and widens: sizes differ
        imgs[k] = 40 + k
        imgs[k, :, 300 * k:300 * k + 50 + 37 * k] = (20 * k, 255 - 10 * k, k)
        imgs[k, 100 + 150 * k:140 + 160 * k, :, 1] = 7 * k
    bound = _bound(W, H, C)
    out = np.zeros(bound * count, np.uint8)
    index = np.zeros((count, 2), np.uint64)
    with _ctx(W, H) as c:
        before = c.mem_info()["ctx_bytes"]
        _lib.check(c.lib.mav_png_encode(c.h, imgs.ctypes.data, count, C, out.ctypes.data, out.size, index.ctypes.data))
        grown = c.mem_info()["ctx_bytes"] - before
        (alone,) = c.png_encode(imgs[count - 1:])
    index = index.astype(np.int64)
    assert index[0, 0] == 0 and (index[1:, 0] == index[:-1].sum(axis=1)).all(), "the streams are not back to back from offset 0"
    assert len(set(index[:, 1].tolist())) == count, "the images were meant to give streams of different sizes"
    for k in range(count):
        z = out[index[k, 0]:index[k].sum()].tobytes()
        d = zlib.decompressobj()
        assert d.decompress(z) == model.scanlines(imgs[k]) and d.eof and d.unused_data == b"", f"image {k}: not its own scanlines"
        assert len(z) <= bound
    assert not out[index[-1].sum():].any(), "bytes behind the last stream"
    assert out[index[-1, 0]:index[-1].sum()].tobytes() == _idat(alone)[3], "the last image of the call differs from the same image alone"
    # the context's ledger counts this call's three staging blocks (images, streams, index) exactly; what else it took is the workspace
    staging = imgs.nbytes + bound * count + 16 * count
    print(f"workspace per image {per}, per chunk {per_chunk}; ctx_bytes grew by {grown}, staging {staging}, workspace {grown - staging}")
    assert grown - staging == per_chunk * per < count * per, "the workspace holds every image: the call was not chunked"


@pytest.mark.parametrize("family", ["deep", "edge"])
def test_same_bytes_on_every_call(mav, family):
    runs = []
    for _ in range(2):                                                       # two contexts, two calls each
        files = []
        for (H, W, C), cases in _by_shape(fam.FAMILIES[family]()).items():
            with _ctx(W, H) as c:
                for _ in range(2):
                    files.append([c.png_encode(img[None])[0] for _, img in cases])
        runs.append(files)
    assert runs[0] == runs[1] and all(a == b for a, b in zip(runs[0][0::2], runs[0][1::2]))
