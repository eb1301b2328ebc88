"""The result-image restatement (tests/render_ref.py) against the two images the reference's own code wrote, and the PNG writer.
No GPU needed.

    media/colorwheel.png   im_helpers.get_colorwheel(): flow_vis.flow_to_color of a float64 disk      (tests/golden/colorwheel.png)
    media/colorbar.png     im_helpers.plot_colorbar(): cv2.applyColorMap(JET) of the rows 0..199     (tests/golden/colorbar.png)
"""
import hashlib
import os

import numpy as np
import pytest

import render_ref as rr

SHA256 = {
    "colorwheel.png": "89f22d55939d6abdb4e7b9a93f97b29b151b918f65295238ed881ca781a1baaf",
    "colorbar.png": "d2d923ed66066ee9a9f7cb582ab5b2cf9d2b818db6a11c87a4b88db2f76f25b6",
}


@pytest.mark.parametrize("name", sorted(SHA256))
def test_fixture_bytes(name):
    with open(os.path.join(rr.GOLDEN, name), "rb") as f:
        assert hashlib.sha256(f.read()).hexdigest() == SHA256[name]


def test_colorwheel_restatement_is_byte_exact():
    want = rr.decode_rgb(rr.COLORWHEEL_PNG)[:, :, ::-1]          # the file holds RGB, cv2 wrote a BGR array
    got = rr.flow_to_color(rr.colorwheel_field())
    assert got.shape == want.shape == (250, 250, 3)
    assert np.array_equal(got, want), int((got != want).any(axis=2).sum())


def test_colorwheel_does_not_hinge_on_the_last_bits_of_atan2():
    # Moving arctan2 by up to 2 ulps (either way) changes no byte of the colour wheel, the axis and diagonal rays included: an atan2
    # within 2 ulps of the correctly rounded one reproduces the reference's image exactly (the GPU test holds the device to it).
    assert not rr.atan2_sensitive(rr.colorwheel_field(), 2).any()


def test_jet_head_matches_colorbar():
    rgb = rr.decode_rgb(rr.COLORBAR_PNG)
    lut = rr.jet_lut()
    assert lut.shape == (256, 3)
    rows = np.arange(200)
    assert np.array_equal(lut[rows], rgb[:, 0, ::-1])


def test_jet_mirror_cross_check():
    lut = rr.jet_lut().astype(int)
    B, G, R = lut[:, 0], lut[:, 1], lut[:, 2]
    i = np.arange(56, 200)
    bad_r = i[R[i] != B[255 - i]]
    assert list(bad_r) == [96] and (R[96], B[159]) == (2, 1)        # the one asymmetric entry of OpenCV's table
    assert np.array_equal(G[i], G[255 - i])
    # the restated (unpinned) tail against the mirror of the pinned entries 0..55
    j = np.arange(0, 56)
    assert np.abs(R[255 - j] - B[j]).max() <= 1
    assert np.abs(G[255 - j] - G[j]).max() <= 1
    assert np.abs(B[255 - j] - R[j]).max() <= 1


def test_result_image_semantics():
    m = np.zeros((3, 5), bool)
    assert not rr.result_image(m).any()                          # 0 / 0 -> NaN -> 0
    m[1, 2] = True
    img = rr.result_image(m)
    assert img.dtype == np.uint8 and img.shape == (3, 5, 3)
    assert (img[1, 2] == 255).all() and img.sum() == 3 * 255


def test_phi_image_rounding_and_nan():
    lut = rr.jet_lut()
    phi = np.array([[0.0, 180.0, 90.0, np.nan, 0.35294117647058826]])        # the last: 0.5 exactly after the scale -> 0 (half to even)
    g = rr.to_int(phi, max_value=180.0)
    assert list(g[0]) == [0, 255, 128, 0, 0]
    assert np.array_equal(rr.phi_image(phi, lut)[0], lut[g[0]])


@pytest.mark.parametrize("shape", [(1, 1), (3, 7), (5, 13, 3), (4, 33), (2, 9, 3), (17, 1, 3)])
def test_imwrite_round_trip(tmp_path, shape):
    from mavflow.frame_source import decode_png, imwrite
    rng = np.random.default_rng(sum(shape))
    img = rng.integers(0, 256, shape, dtype=np.uint8)
    img[0] = 0                                                   # a constant row: the filter choice sees more than noise
    path = str(tmp_path / "x.png")
    assert imwrite(path, img) is True
    with open(path, "rb") as f:
        px, ctype = decode_png(f.read())
    if img.ndim == 2:
        assert ctype == 0 and np.array_equal(px, img)
    else:
        assert ctype == 2 and np.array_equal(px, img[:, :, ::-1])   # BGR in, RGB in the file: cv2.imwrite's convention


def test_imwrite_rejects_what_cv2_would_not_write_as_8_bit(tmp_path):
    from mavflow.frame_source import imwrite
    with pytest.raises(ValueError):
        imwrite(str(tmp_path / "x.png"), np.zeros((2, 2, 3), np.float32))
    with pytest.raises(ValueError):
        imwrite(str(tmp_path / "x.png"), np.zeros((2, 2, 5), np.uint8))
    with pytest.raises(ValueError):
        imwrite(str(tmp_path / "x.jpg"), np.zeros((2, 2), np.uint8))
