"""tests/resize_ref.py (include/mavflow_resize.h in numpy) held to definitions it shares no code with: float32 linear against torch's
bilinear interpolate and a float64 bilinear written from the clipped coordinate, uint8 linear against the exact bilinear value, the
area forms against the box integral and the block mean, the 2 x 2 uint8 rounding, the linear-to-area and copy dispatch, and nearest
against its index formula.  Every tolerance is derived where it is used, from the number formats and the definition, not measured."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import resize_cases as T
import resize_ref as R

EPS32 = 2.0 ** -24                       # half an ulp of float32, relative: the error of one rounded operation
ENLARGING = [s for s in T.SHAPES if s.dst[0] >= s.src[0] and s.dst[1] >= s.src[1] and s.dst != s.src]
LINEAR_SHAPES = [s for s in T.SHAPES if R.form_of(R.F32C1, *s.src, *s.dst, R.LINEAR) == "linear"]
ids = lambda s: f"{s.src[0]}x{s.src[1]}-{s.dst[0]}x{s.dst[1]}"


def test_constants_are_the_librarys_and_cv2s(mav):
    from mavflow import resize as K, warp
    assert (K.INTER_NEAREST, K.INTER_LINEAR, K.INTER_AREA) == (R.NEAREST, R.LINEAR, R.AREA) == (0, 1, 3)
    assert (warp.WARP_U8C1, warp.WARP_U8C3, warp.WARP_F32C1, warp.WARP_F32C2) == (R.U8C1, R.U8C3, R.F32C1, R.F32C2)
    assert K.MAX_SIDE == R.MAX_SIDE == 32767


def _bilinear64(S, dw, dh):
    """float64 bilinear from the coordinate clip((d + 0.5) * scale - 0.5, 0, ssize - 1), written directly"""
    sh, sw = S.shape[:2]
    S = S.astype(np.float64)
    fx = np.clip((np.arange(dw) + 0.5) * (sw / dw) - 0.5, 0, sw - 1)
    fy = np.clip((np.arange(dh) + 0.5) * (sh / dh) - 0.5, 0, sh - 1)
    x0, y0 = np.minimum(np.floor(fx).astype(int), max(sw - 2, 0)), np.minimum(np.floor(fy).astype(int), max(sh - 2, 0))
    x1, y1 = np.minimum(x0 + 1, sw - 1), np.minimum(y0 + 1, sh - 1)
    ax, ay = (fx - x0)[None, :, None], (fy - y0)[:, None, None]
    top = S[y0][:, x0] * (1 - ax) + S[y0][:, x1] * ax
    bot = S[y1][:, x0] * (1 - ax) + S[y1][:, x1] * ax
    return top * (1 - ay) + bot * ay


# torch's kernel runs in a process of its own, once for all shapes.  torch ships its own HIP and HSA runtimes, and its libraries ask for
# them by file name, not by SONAME: imported into a process that has already loaded libmavflow.so (every test that takes `mav`), it maps
# a second HIP runtime beside the one the library is linked to, and a process with two of them has ended in glibc's "double free or
# corruption" at exit after every test had passed.  Nothing of the library is imported there.
_TORCH_WORKER = """
import sys
import numpy as np
import torch
src = np.load(sys.argv[1])
out = {}
for key in src.files:
    dh, dw = (int(v) for v in key.split("|")[1].split(","))
    S = src[key]
    t = torch.nn.functional.interpolate(torch.from_numpy(S.transpose(2, 0, 1)[None].copy()), size=(dh, dw), mode="bilinear", align_corners=False)
    out[key] = t[0].numpy().transpose(1, 2, 0)
np.savez(sys.argv[2], **out)
"""
_torch = {}


def _torch_input(fmt, shape):
    (sw, sh) = shape.src
    return T.images(fmt, sw, sh, special=False)[1].reshape(sh, sw, -1)


def _torch_bilinear(fmt, shape):
    """torch.nn.functional.interpolate(mode="bilinear", align_corners=False) of the case's image, (dh, dw, C) float32"""
    key = lambda f, s: f"{f}:{ids(s)}|{s.dst[1]},{s.dst[0]}"
    if not _torch:
        with tempfile.TemporaryDirectory() as d:
            a, b = os.path.join(d, "in.npz"), os.path.join(d, "out.npz")
            np.savez(a, **{key(f, s): _torch_input(f, s) for f in (R.F32C1, R.F32C2) for s in LINEAR_SHAPES})
            r = subprocess.run([sys.executable, "-c", _TORCH_WORKER, a, b], capture_output=True, text=True)
            assert r.returncode == 0, r.stderr[-2000:]
            with np.load(b) as z:
                _torch.update({k: z[k] for k in z.files})
    return _torch[key(fmt, shape)]


def _steps(S):
    """the largest difference of two taps a pixel blends along x and along y"""
    S = S.astype(np.float64)
    dx = np.abs(np.diff(S, axis=1)).max() if S.shape[1] > 1 else 0.0
    dy = np.abs(np.diff(S, axis=0)).max() if S.shape[0] > 1 else 0.0
    return dx, dy


@pytest.mark.parametrize("shape", LINEAR_SHAPES, ids=ids)
@pytest.mark.parametrize("fmt", [R.F32C1, R.F32C2])
def test_float32_linear_against_float64_and_torch(mav, fmt, shape):
    """The restatement differs from the exact bilinear value by (1) the coordinate's one rounding to float32, at most 2^-24 * max(sw, sh)
    pixels per axis (f < ssize, half an ulp of f), which moves the value by at most that times the largest tap difference along the axis,
    and (2) the rounding of 1 - a, 1 - b, four products and two sums, each 2^-24 relative of a term no larger than max|S|: 8 of them.
    torch's kernel takes scale and coordinate in float32: a rounded scale (2^-24 relative, times d + 0.5 <= dsize), a rounded product
    and a rounded difference, so three such coordinate errors where the restatement has one (in units of max(sw, sh, dw, dh), its
    coordinates being as large as the larger side), and its own 8 roundings of the blend."""
    (sw, sh), (dw, dh) = shape.src, shape.dst
    S = _torch_input(fmt, shape)
    got = R.resize(S, dw, dh, R.LINEAR).astype(np.float64)
    top = np.abs(S).max()
    dx, dy = _steps(S)
    coord = EPS32 * max(sw, sh, dw, dh)
    tol64 = coord * (dx + dy) + 8 * EPS32 * top
    err64 = np.abs(got - _bilinear64(S, dw, dh)).max()
    t = _torch_bilinear(fmt, shape)
    assert t.shape == got.shape and t.dtype == np.float32
    err_t = np.abs(got - t.astype(np.float64)).max()
    tol_t = 4 * coord * (dx + dy) + 16 * EPS32 * top
    print(f"{ids(shape)} fmt {fmt}: |ref - float64| {err64:.3e} (bound {tol64:.3e}), |ref - torch| {err_t:.3e} (bound {tol_t:.3e}), max|S| {top:.3g}")
    assert err64 <= tol64
    assert err_t <= tol_t


@pytest.mark.parametrize("shape", LINEAR_SHAPES, ids=ids)
@pytest.mark.parametrize("fmt", [R.U8C1, R.U8C3])
def test_uint8_linear_within_one_grey_level(mav, fmt, shape):
    """|restatement - exact float64 bilinear| < 1 grey level, from the 11-bit coefficients and the three truncating shifts:
      coefficients: c0 = rint(2048 (1 - a)), c1 = rint(2048 a) with c0 + c1 == 2048 (asserted below for this shape's tables: it fails
        only where the float32 rounding of 1.f - a lands on a tie), so their errors are e and -e, |e| <= 1/2, and the horizontal value is
        off by |e (S0 - S1)| / 2048 <= 255 / 4096 = 0.0623 grey levels; the same again for the vertical pair: 0.1246 together;
      h >> 4 drops less than 1/128 of a grey level (h is in 1/2048): 0.0079;
      the two >> 16 each drop less than one unit of 1/4 grey level, and (x + 2) >> 2 of the integer x they leave is within
        (-3/4, +1/2] of x / 4 + what they dropped: the shifts together move the result by less than 0.75 + 0.0079 down or 0.5 up.
      Sum: < 0.1246 + 0.0079 + 0.75 = 0.8825 < 1."""
    (sw, sh), (dw, dh) = shape.src, shape.dst
    for axis, (dsz, ssz) in (("x", (dw, sw)), ("y", (dh, sh))):
        _, a, _ = R.linear_table(dsz, ssz, ssz / dsz)
        c0, c1 = R.linear_coefs(a)
        assert ((c0 + c1) == 2048).all(), axis
    worst = 0.0
    for S in T.images(fmt, sw, sh):                         # the 0 / 255 checkerboard, then full-range noise
        S = S.reshape(sh, sw, -1)
        err = np.abs(R.resize(S, dw, dh, R.LINEAR).astype(np.float64) - _bilinear64(S, dw, dh)).max()
        worst = max(worst, err)
    print(f"{ids(shape)} fmt {fmt}: largest |ref - exact| {worst:.4f} grey levels (bound 0.8825 derived, 1 asserted)")
    assert worst < 1


def _box64(S, dw, dh):
    """the float64 box integral: destination cell d covers [d * scale, (d + 1) * scale) of the source's unit cells"""
    sh, sw = S.shape[:2]

    def weights(dsize, ssize):
        scale = ssize / dsize
        Wt = np.zeros((dsize, ssize))
        for d in range(dsize):
            lo, hi = d * scale, min((d + 1) * scale, ssize)
            for s in range(int(np.floor(lo)), min(int(np.ceil(hi)), ssize)):
                Wt[d, s] = max(0.0, min(hi, s + 1) - max(lo, s)) / (hi - lo)
        return Wt
    return np.einsum("ys,swc,xw->yxc", weights(dh, sh), S.astype(np.float64), weights(dw, sw))


def _dropped(dsize, ssize):
    """the largest part of a cell that area_span's 1e-3 thresholds drop at this axis, from the definition: a partial first or last cell
    narrower than 1e-3 is not a tap"""
    scale, worst = ssize / dsize, 0.0
    for d in range(dsize):
        for edge in (d * scale, d * scale + scale):
            frac = min(edge - np.floor(edge), np.ceil(edge) - edge)
            if 0 < frac <= 1e-3:
                worst = max(worst, frac)
    return worst


AREA_SHAPES = [s for s in T.SHAPES if s.dst[0] <= s.src[0] and s.dst[1] <= s.src[1] and s.dst != s.src]


@pytest.mark.parametrize("shape", AREA_SHAPES, ids=ids)
@pytest.mark.parametrize("fmt", list(R.FORMATS))
def test_area_against_the_box_integral(mav, fmt, shape):
    """Every area form is the mean of the source over the destination cell (for whole ratios the block mean, which the box integral
    then is).  float32: each of the nx + ny taps costs a rounded weight, a product and a sum (3 * 2^-24 relative of at most max|S|
    each, the weights summing to 1), the fast form fewer; a dropped sliver of a cell, at most `dropped / scale` of the weight per edge
    and four edges, moves the mean by that part of max|S|.  uint8 adds the final rounding: at most 1/2."""
    (sw, sh), (dw, dh) = shape.src, shape.dst
    form = R.form_of(fmt, sw, sh, dw, dh, R.AREA)
    assert form in ("area_2x2", "area_fast", "area_general")
    nx, ny = int(np.ceil(sw / dw)) + 1, int(np.ceil(sh / dh)) + 1
    for S in T.images(fmt, sw, sh, special=False):
        S = S.reshape(sh, sw, -1)
        top = float(np.abs(S.astype(np.float64)).max())
        tol = (3 * (nx + ny) * EPS32 + 2 * _dropped(dw, sw) / (sw / dw) + 2 * _dropped(dh, sh) / (sh / dh)) * top
        if S.dtype == np.uint8:
            tol += 0.5
        err = np.abs(R.resize(S, dw, dh, R.AREA).astype(np.float64) - _box64(S, dw, dh)).max()
        print(f"{ids(shape)} fmt {fmt} {form}: |ref - box integral| {err:.3e} (bound {tol:.3e})")
        assert err <= tol


def test_uint8_2x2_rounds_a_half_up_where_the_other_forms_round_to_even(mav):
    rng = np.random.default_rng(5)
    S = rng.integers(0, 256, (24, 32), dtype=np.uint8)
    blocks = S.reshape(12, 2, 16, 2).astype(np.int64)
    # make every block's sum 2 mod 4: a mean of k + 1/2
    fix = (2 - blocks.sum(axis=(1, 3))) % 4
    corner = blocks[:, 0, :, 0]
    blocks[:, 0, :, 0] = np.where(corner + fix > 255, corner + fix - 4, corner + fix)
    S = blocks.reshape(24, 32).astype(np.uint8)
    sums = S.reshape(12, 2, 16, 2).astype(np.int64).sum(axis=(1, 3))
    assert (sums % 4 == 2).all()
    got = R.resize(S, 16, 12, R.AREA)
    assert R.form_of(R.U8C1, 32, 24, 16, 12, R.AREA) == "area_2x2"
    assert np.array_equal(got, np.floor(sums / 4 + 0.5).astype(np.uint8))            # half up
    even = np.rint(sums / 4).astype(np.uint8)
    assert (got != even).any() and np.array_equal(got[got != even], even[got != even] + 1)      # the two roundings part, by one
    # the other u8 rule (rintf) rounds a half to even: a 3 x 2 shrink, where a block sum of 3 mod 6 is a mean of k + 1/2
    S3 = np.ascontiguousarray(S[:, :30])
    g3 = R.resize(S3, 10, 12, R.AREA)
    assert R.form_of(R.U8C1, 30, 24, 10, 12, R.AREA) == "area_fast"
    s3 = S3.reshape(12, 2, 10, 3).astype(np.int64).sum(axis=(1, 3))
    halves = s3 % 6 == 3
    assert halves.any() and np.array_equal(g3[halves], np.rint(s3[halves] / 6).astype(np.uint8))


@pytest.mark.parametrize("fmt", list(R.FORMATS))
def test_linear_at_an_exact_halving_is_the_area_result(mav, fmt):
    S = T.images(fmt, 64, 48, special=False)[1]
    lin, area = R.resize(S, 32, 24, R.LINEAR), R.resize(S, 32, 24, R.AREA)
    assert lin.tobytes() == area.tobytes()
    direct = R.linear(S.reshape(48, 64, -1), 32, 24).reshape(lin.shape)              # the bilinear table, had the dispatch not turned away
    if S.dtype == np.uint8:
        # a == b == 1/2 gives coefficients of 1024, and (1024 * ((S0 + S1) * 1024 >> 4)) >> 16 == S0 + S1 with nothing dropped: for
        # uint8 the two definitions are the same bytes, so the turn to the area form shows in the float32 formats alone
        assert direct.tobytes() == lin.tobytes()
    else:
        assert direct.tobytes() != lin.tobytes()                                     # ((a + b) + c + d) / 4 against (a/2 + b/2)/2 + ...
    block = S.reshape(24, 2, 32, 2, -1).astype(np.float64).mean(axis=(1, 3)).reshape(lin.shape)
    assert np.abs(lin.astype(np.float64) - block).max() <= (0.5 if S.dtype == np.uint8 else 6 * EPS32 * np.abs(S).max())
    # one axis alone at 2 stays linear
    assert R.form_of(fmt, 64, 48, 32, 48, R.LINEAR) == "linear" and R.form_of(fmt, 64, 48, 32, 25, R.LINEAR) == "linear"


@pytest.mark.parametrize("fmt", list(R.FORMATS))
def test_copy_form_and_nearest(mav, fmt):
    S = T.images(fmt, 20, 12)[0]
    for interp in (R.NEAREST, R.LINEAR, R.AREA):
        out = R.resize(S, 20, 12, interp)
        assert out is not S and out.tobytes() == S.tobytes()                        # bytes: the NaN's payload and the +inf included
    for shape in T.SHAPES:
        (sw, sh), (dw, dh) = shape.src, shape.dst
        if shape.dst == shape.src:
            continue
        S = T.images(fmt, sw, sh)[0]
        got = R.resize(S, dw, dh, R.NEAREST)
        for dy in (0, dh // 2, dh - 1):
            for dx in range(dw):
                sy, sx = min(int(np.floor(dy * (sh / dh))), sh - 1), min(int(np.floor(dx * (sw / dw))), sw - 1)
                assert got[dy, dx].tobytes() == S[sy, sx].tobytes(), (shape, dy, dx)


def test_one_tap_region_and_zero_weights(mav):
    """what the table's shapes are there to reach is reached: 1 x 1 is one tap everywhere; at 33 -> 65 destination column 32 has a == 0
    with two taps, so an infinite right neighbour gives NaN there; the NaN and +inf of the float inputs sit under zero weights"""
    s, a, one = R.linear_table(5, 1, 1 / 5)
    assert one.all() and (s == 0).all() and (a == 0).all()
    s, a, one = R.linear_table(7, 2, 2 / 7)
    assert (~one).any() and one.any() and (a[~one] > 0).any()
    s, a, one = R.linear_table(65, 33, 33 / 65)
    assert s[32] == 16 and a[32] == 0 and not one[32]
    S = np.ones((17, 33), np.float32)
    S[:, 17] = np.inf
    out = R.resize(S, 65, 70, R.LINEAR)
    assert np.isnan(out[:, 32]).all() and R.bits(out[:, 32]).tolist() == [0x7FC00000] * 70       # inf * 0, stored as the quiet NaN
    b = R.linear_table(70, 17, 17 / 70)[1]
    assert (b == 0).any() and np.isinf(out[b != 0, 33]).all() and np.isnan(out[b == 0, 33]).all()  # inf h * (1 - b) + inf h * b: NaN where b == 0
    for fmt in (R.F32C1, R.F32C2):
        img = T.images(fmt, 33, 17)[0].reshape(17, 33, -1)
        out = R.resize(img, 65, 70, R.LINEAR)
        ny, nx = T.nan_pixel(33, 17)
        assert nx == 1 and np.isnan(out[:, 0, 0]).any()              # the left border: S[0] * 1 + S[1] * 0 with S[1] = NaN
        iy, ix = T.inf_pixel(33, 17)
        assert iy == 1 and np.isnan(out[0, :, -1]).any()             # the top border: h(row 0) * 1 + h(row 1) * 0 with an infinite h(row 1)
        assert np.isinf(out[..., -1]).any()                          # and +inf under a non-zero weight stays +inf
