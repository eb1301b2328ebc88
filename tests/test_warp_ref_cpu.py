"""tests/warp_ref.py held to its definition (include/mavflow_warp.h) and to an independent interpolator, without a GPU: identity and
integer shifts are exact in every format on every coordinate route; INVERSE_MAP with M equals the plain call with inv(M) where the
inverse is exact; on coordinates that are exact multiples of 1/32 the uint8 result EQUALS floor(map_coordinates + 0.5) (both sides
exact there); a float32 result lies within the four-term bound gamma_4 * max|tap| (the argument of tests/test_history_ref_cpu.py); the
affine fixed-point route for x + 0.5 gives sx = x - 1, ax = 16; and the restatement shares its float32 map steps with history_ref."""
import numpy as np
import pytest
from scipy.ndimage import map_coordinates

import history_ref as HR
import warp_cases as T
import warp_ref as R

W, H = 37, 23
FMTS = [R.U8C1, R.U8C3, R.F32C1, R.F32C2]


def _img(fmt, nan=False):
    return T.images(fmt, W, H, nan=nan)[1]


def _shifted(img, dx, dy):
    """img sampled at (x + dx, y + dy), integer shifts, zero outside: the definition by slicing"""
    out = np.zeros_like(img)
    ys, xs = np.arange(H) + dy, np.arange(W) + dx
    oky, okx = (ys >= 0) & (ys < H), (xs >= 0) & (xs < W)
    out[np.ix_(np.where(oky)[0], np.where(okx)[0])] = img[np.ix_(ys[oky], xs[okx])]
    return out


@pytest.mark.parametrize("fmt", FMTS, ids=lambda f: R.FORMAT_NAMES[f])
@pytest.mark.parametrize("shift", [(0, 0), (3, -2), (-5, 4), (W, 0), (0, -H)], ids=str)
def test_identity_and_integer_shifts_are_exact_on_every_route(fmt, shift):
    img = _img(fmt)
    dx, dy = shift
    want = _shifted(img, dx, dy)
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    m = np.stack([x + dx, y + dy], axis=-1)
    flow = np.full((H, W, 2), (-dx, -dy), np.float32)
    A = np.array([[1, 0, dx], [0, 1, dy]], np.float64)
    P = np.vstack([A, [0, 0, 1]])
    got = [R.remap(img, m), R.remap_planes(img, m[..., 0], m[..., 1]), R.warp_flow(img, flow), R.warp_affine(img, A, R.INVERSE_MAP),
           R.warp_perspective(img, P, R.INVERSE_MAP)]
    Ai = np.array([[1, 0, -dx], [0, 1, -dy]], np.float64)
    got += [R.warp_affine(img, Ai, 0), R.warp_perspective(img, np.vstack([Ai, [0, 0, 1]]), 0)]
    for g in got:
        assert g.dtype == img.dtype and g.shape == img.shape and g.tobytes() == want.tobytes()


@pytest.mark.parametrize("fmt", FMTS, ids=lambda f: R.FORMAT_NAMES[f])
def test_inverse_map_equals_the_plain_call_with_the_exact_inverse(fmt):
    img = _img(fmt)
    for M, Mi in (([[2, 0, 4], [0, 0.5, -3]], [[0.5, 0, -2], [0, 2, 6]]), ([[0, 4, 1], [-0.25, 0, 2]], [[0, -4, 8], [0.25, 0, -0.25]]),
                  ([[1, 0, 7], [0, 1, -9]], [[1, 0, -7], [0, 1, 9]])):
        M, Mi = np.array(M, np.float64), np.array(Mi, np.float64)
        assert np.array_equal(np.vstack([M, [0, 0, 1]]) @ np.vstack([Mi, [0, 0, 1]]), np.eye(3))
        assert np.array_equal(R.invert_affine(M), Mi.ravel())
        assert R.warp_affine(img, M, 0).tobytes() == R.warp_affine(img, Mi, R.INVERSE_MAP).tobytes()
        P, Pi = np.vstack([M, [0, 0, 1]]), np.vstack([Mi, [0, 0, 1]])
        assert np.array_equal(R.invert_perspective(P), Pi.ravel())
        assert R.warp_perspective(img, P, 0).tobytes() == R.warp_perspective(img, Pi, R.INVERSE_MAP).tobytes()
    # a projective one: powers of two throughout
    P = np.array([[2, 0, 0], [0, 2, 0], [0.25, 0, 1]], np.float64)
    Pi = R.invert_perspective(P).reshape(3, 3)
    assert np.array_equal(P @ Pi, np.eye(3))
    assert R.warp_perspective(img, P, 0).tobytes() == R.warp_perspective(img, Pi, R.INVERSE_MAP).tobytes()
    # a zero determinant gives the zero matrix
    assert not R.invert_affine([[1, 2, 0], [2, 4, 1]]).any() and not R.invert_perspective(np.zeros((3, 3))).any()
    assert not R.invert_perspective([[1, 2, 3], [2, 4, 6], [0, 0, 1]]).any()


def _coords_32nds(seed):
    rng = np.random.default_rng(seed)
    mx = rng.integers(-2 * 32, (W + 1) * 32, (H, W)).astype(np.float32) / np.float32(32)
    my = rng.integers(-2 * 32, (H + 1) * 32, (H, W)).astype(np.float32) / np.float32(32)
    return mx, my


@pytest.mark.parametrize("fmt", [R.U8C1, R.U8C3], ids=lambda f: R.FORMAT_NAMES[f])
def test_uint8_equals_the_independent_interpolator_on_32nds(fmt):
    """weights and taps are exact on both sides: T * w sums to a multiple of 1/1024 below 2^8, exact in float64; floor(v + 0.5) is
    (v * 32768 + 16384) >> 15"""
    for seed, img in ((1, T.images(fmt, W, H)[0]), (2, T.images(fmt, W, H)[1])):
        mx, my = _coords_32nds(seed)
        got = R.remap_planes(img, mx, my).reshape(H, W, -1)
        src = img.reshape(H, W, -1).astype(np.float64)
        for c in range(src.shape[2]):
            v = map_coordinates(src[..., c], [my.astype(np.float64), mx.astype(np.float64)], order=1, mode="grid-constant", cval=0.0)
            assert np.array_equal(got[..., c], np.floor(v + 0.5).astype(np.uint8)), (seed, c)
    # the int16 table's 32767 gives the same byte as 32768 under a full weight
    t = np.arange(256, dtype=np.int64)
    assert np.array_equal((t * 32767 + 16384) >> 15, t) and np.array_equal((t * 32768 + 16384) >> 15, t)


@pytest.mark.parametrize("fmt", [R.F32C1, R.F32C2], ids=lambda f: R.FORMAT_NAMES[f])
def test_float32_lies_within_the_four_term_bound(fmt):
    """the weights are exact; four products and three sums in float32: |err| <= gamma_4 * sum |T_k| w_k <= gamma_4 * max|tap|, u = 2^-24"""
    img = _img(fmt)
    u = 2.0 ** -24
    gamma4 = 4 * u / (1 - 4 * u)
    rng = np.random.default_rng(3)
    mx = rng.uniform(-2, W + 1, (H, W)).astype(np.float32)
    my = rng.uniform(-2, H + 1, (H, W)).astype(np.float32)
    fits, qx, qy = R.q_from_map(mx, my)
    assert fits.all()
    got = R.remap_planes(img, mx, my).reshape(H, W, -1).astype(np.float64)
    src = img.reshape(H, W, -1).astype(np.float64)
    bound = gamma4 * np.abs(src).max()
    for c in range(src.shape[2]):
        v = map_coordinates(src[..., c], [qy / 32.0, qx / 32.0], order=1, mode="grid-constant", cval=0.0)
        assert np.abs(got[..., c] - v).max() <= bound + 1e-12 * np.abs(src).max()      # (the interpolator's own float64 rounding)
    assert np.abs(got).max() > 1


def test_affine_fixed_point_route_for_half_a_pixel():
    fits, qx, qy = R.q_affine([[1, 0, 0.5], [0, 1, 0.5]], 0, H, W)         # inverted: x - 0.5
    assert fits.all()
    assert np.array_equal(qx >> 5, np.broadcast_to(np.arange(W) - 1, (H, W))) and (qx & 31 == 16).all()
    assert np.array_equal(qy >> 5, np.broadcast_to(np.arange(H)[:, None] - 1, (H, W))) and (qy & 31 == 16).all()
    fits, qx, qy = R.q_affine([[1, 0, 0.5], [0, 1, 0.5]], R.INVERSE_MAP, H, W)
    assert np.array_equal(qx >> 5, np.broadcast_to(np.arange(W), (H, W))) and (qx & 31 == 16).all()
    # AB_BITS = 10, round_delta = 16: 1/64 px above a 1/32 step rounds up, just below it does not
    assert R.q_affine([[1, 0, 1 / 64], [0, 1, 0]], R.INVERSE_MAP, 1, 1)[1][0, 0] == 1
    assert R.q_affine([[1, 0, 1 / 64 - 1 / 1024], [0, 1, 0]], R.INVERSE_MAP, 1, 1)[1][0, 0] == 0
    # saturation and wrap-around
    assert list(R.sat_rint([np.nan, 1e10, -1e10, 0.5, 1.5, -0.5, 2147483646.5])) == [R.INT_MIN, R.INT_MAX, R.INT_MIN, 0, 2, 0, 2147483646]
    assert list(R.wrap32([R.INT_MAX + 16, R.INT_MIN - 1, 5])) == [R.INT_MIN + 15, R.INT_MAX, 5]


def test_perspective_per_pixel_form():
    M = np.array([[1, 0, 0], [0, 1, 0], [1, 0, -3]], np.float64)
    fits, qx, qy = R.q_perspective(M, R.INVERSE_MAP, 2, 7)
    assert fits.all() and qx[0, 3] == 0 and qy[1, 3] == 0                  # W = 0 -> 0
    assert qx[0, 4] == 4 * 32 and qx[0, 2] == -2 * 32 and qy[1, 5] == 16   # x / (x - 3), y / (x - 3)
    fits, qx, qy = R.q_perspective([[np.inf, 0, 0], [0, 1, 0], [0, 0, 1]], R.INVERSE_MAP, 1, 2)
    assert not fits[0, 0] and fits[0, 1] and qx[0, 1] == R.INT_MAX         # inf * 0 is NaN: wholly outside; inf is clamped
    fits, qx, qy = R.q_perspective([[1e12, 0, -5e12], [0, 1, 0], [0, 0, 1]], R.INVERSE_MAP, 1, 8)
    assert fits.all() and qx[0, 0] == R.INT_MIN and qx[0, 7] == R.INT_MAX and qx[0, 5] == 0


def test_the_map_steps_are_the_history_remaps():
    """a float32 2-channel image through warp_ref's remap is history_ref's remap with the float32 sum in place of the double one: the
    same cells, fractions and wholly-outside decisions, and where the double sum is exactly representable the same values"""
    img = T.images(R.F32C2, W, H, nan=False)[1]
    img = np.round(img).astype(np.float32)                                  # integers: T * w is a multiple of 1/1024, sums exact in float32
    for name, m in T.map_fields(W, H):
        tr_h, tr_w = [], []
        a = HR.remap_linear_ref(img, m[..., 0], m[..., 1], tr_h)
        b = R.remap(img, m, tr_w)
        for k in ("fits", "qx", "qy", "sx", "sy", "inside"):
            assert np.array_equal(tr_h[0][k], tr_w[-1][k]), (name, k)
        assert np.array_equal(a.astype(np.float32), b) and np.array_equal(a, b.astype(np.float64)), name


def test_warp_flow_map_is_one_float32_addition():
    flow = T.flow_fields(W, H)[-1][1]
    m = R.flow_map(flow)
    y, x = np.mgrid[0:H, 0:W]
    assert m.dtype == np.float32
    assert np.array_equal(m[..., 0], x.astype(np.float32) + (-flow[..., 0])) and np.array_equal(m[..., 1], y.astype(np.float32) + (-flow[..., 1]))
    assert np.array_equal(m[..., 0], (x.astype(np.float64) - flow[..., 0].astype(np.float64)).astype(np.float32))    # rounding through double is innocuous
    keep = flow.copy()
    R.warp_flow(T.images(R.U8C3, W, H)[1], flow)
    assert np.array_equal(keep, flow)


def test_warp_method_is_the_references_lines():
    flow = T.method_flow(W, H)[1]
    M = [m for m in T.affine_matrices(W, H) if m.name == "rotation with scale"][0].M
    diff, mag, rec = R.warp_method(flow, M, R.AFFINE)
    stable = R.warp_affine(flow, M, 0)
    want = np.where(stable == 0, np.float32(0), flow - stable)
    assert diff.tobytes() == want.astype(np.float32).tobytes()
    assert mag.tobytes() == np.sqrt(want[..., 0] ** 2.0 + want[..., 1] ** 2.0).astype(np.float32).tobytes()
    assert (rec["row"], rec["col"]) == np.unravel_index(mag.argmax(), mag.shape) and rec["pad"] == 0 and R.RECORD_DTYPE.itemsize == 16
    f = flow.copy()
    f[3, 4, 0] = np.nan
    diff, mag, rec = R.warp_method(f, [[1, 0, 0], [0, 1, 0]], R.AFFINE)
    assert np.isnan(rec["max_mag"]) and HR.bits(np.array([rec["max_mag"]]))[0] == 0x7FC00000       # a NaN ranks above every number, the first one wins
    assert (rec["row"], rec["col"]) == tuple(np.argwhere(np.isnan(mag))[0])
