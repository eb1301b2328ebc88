"""Writes tests/golden/jpeg_frames.npz: every file of tests/jpeg_cases.py that Pillow's encoder (libjpeg-turbo) makes, and for every
valid case -- encoder-made or written by hand -- np.asarray(PIL.Image.open(file)).  Run once, on the CPU, where Pillow imports:

    python tests/make_jpeg_fixtures.py
"""
import io
import os
import sys

import numpy as np
from PIL import Image, features

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_cases as jc      # noqa: E402


def picture(W, H, q, seed):
    """textured: a colour ramp under noise; pure noise at quality 100, so that blocks are dense and samples clamp at both ends"""
    rng = np.random.default_rng(seed)
    if q == 100:
        return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    y, x = np.mgrid[0:H, 0:W]
    ramp = np.stack([(x * 5 + y * 3) % 256, (x * 2 + y * 7) % 256, (x * x + y) % 256], -1).astype(np.float64)
    return np.clip(ramp + rng.normal(0, 25 if q == 90 else 12, (H, W, 3)), 0, 255).astype(np.uint8)


def encode(img, samp, q, opt):
    kw = {"quality": q}
    if opt == "optimize":
        kw["optimize"] = True
    if opt == "rmb2":
        kw["restart_marker_blocks"] = 2
    if opt == "rmr1":
        kw["restart_marker_rows"] = 1
    if samp == "gray":
        im = Image.fromarray(img[..., 1])
    else:
        im = Image.fromarray(img)
        kw["subsampling"] = {"444": 0, "422": 1, "420": 2}[samp]
    b = io.BytesIO()
    im.save(b, "JPEG", **kw)
    return b.getvalue()


def main():
    assert features.check_feature("libjpeg_turbo")
    out = {}
    for k, (name, W, H, samp, q, opt) in enumerate(jc.pil_specs()):
        data = encode(picture(W, H, q, 100 + k), samp, q, opt)
        out["file_" + name] = np.frombuffer(data, np.uint8)
        out["px_" + name] = np.asarray(Image.open(io.BytesIO(data)))
    img = picture(24, 16, 90, 7)
    b = io.BytesIO()
    Image.fromarray(img).save(b, "JPEG", quality=90, progressive=True)
    out["file_pil_progressive"] = np.frombuffer(b.getvalue(), np.uint8)
    b = io.BytesIO()
    Image.fromarray(img).convert("CMYK").save(b, "JPEG", quality=90)
    out["file_pil_cmyk"] = np.frombuffer(b.getvalue(), np.uint8)
    for name, data, _ in jc.hand_valid():
        out["px_" + name] = np.asarray(Image.open(io.BytesIO(data)))
    np.savez_compressed(jc.GOLDEN, **out)
    print(f"{jc.GOLDEN}: {len(out)} arrays, {os.path.getsize(jc.GOLDEN)} bytes")


if __name__ == "__main__":
    main()
