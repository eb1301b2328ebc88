"""The numpy restatement of the flow history (tests/history_ref.py) held to its definition (include/mavflow.h, flow history) and to an
independent interpolator, without a GPU: identity and integer shifts are exact, the schedule is the reference's loop, a zero ring
gives zero, a constant integer flow accumulates exactly, and on coordinates that are exact multiples of 1/32 the remap agrees with
scipy.ndimage.map_coordinates(order=1, mode="grid-constant") within the rounding of the four-term sum."""
import numpy as np
import pytest

import history_ref as R


def _field(H, W, seed, dtype=np.float64):
    rng = np.random.default_rng(seed)
    return (rng.normal(0, 3, (H, W, 2)) * 10.0 ** rng.integers(-3, 4, (H, W, 1))).astype(dtype)


def _grid(H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    return xx.astype(np.float32), yy.astype(np.float32)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("W,H", [(1, 1), (7, 1), (1, 5), (13, 9)])
def test_identity_map_returns_the_source_bit_for_bit(W, H, dtype):
    src = _field(H, W, W * 31 + H, dtype)
    src[0, 0] = (0.0, 1e-310 if dtype == np.float64 else 1e-40)         # a zero and a denormal survive too
    out = R.remap_linear_ref(src, *_grid(H, W))
    want = src.astype(np.float64)
    assert out.dtype == np.float64 and np.array_equal(R.bits(out), R.bits(want))


@pytest.mark.parametrize("dx,dy", [(1, 0), (-1, 0), (0, 2), (-3, -2), (20, 0), (0, -20)])
def test_integer_shifts_are_exact_with_zeros_shifted_in(dx, dy):
    W, H = 11, 8
    src = _field(H, W, 5)
    mx, my = _grid(H, W)
    out = R.remap_linear_ref(src, mx + np.float32(dx), my + np.float32(dy))
    want = np.zeros_like(src)
    for y in range(H):
        for x in range(W):
            if 0 <= y + dy < H and 0 <= x + dx < W:
                want[y, x] = src[y + dy, x + dx]
    assert np.array_equal(out, want)
    assert not np.signbit(out[want == 0]).any()                          # what is shifted in is +0.0


def test_schedule_is_the_literal_loop_and_matches_the_table():
    for L in range(3, 25):
        for h in range(L):
            s = R.schedule(L, h)
            if h <= L - 3:
                assert s == list(range(h + 1, L)) + list(range(0, h)), (L, h)
            elif h == L - 2:
                assert s == list(range(0, L - 2)), (L, h)
            else:
                assert s == list(range(1, L)), (L, h)
            assert len(s) <= L - 1
    # the issue's table for L = 20
    assert [len(R.schedule(20, h)) for h in range(20)] == [19] * 18 + [18, 19]
    assert 19 in R.schedule(20, 19) and all(h not in R.schedule(20, h) for h in range(19))


def test_library_schedule_equals_the_literal_loop(mav):
    from mavflow import _lib
    for L in range(3, 25):
        for h in range(L):
            assert _lib.history_schedule(L, h) == R.schedule(L, h), (L, h)
    assert _lib.history_schedule(64, 63) == list(range(1, 64))


@pytest.mark.parametrize("axes", ["reference", "xy"])
def test_zero_ring_gives_exactly_zero(axes):
    ref = R.HistoryRef(6, 9, 4, np.float32, axes)
    for _ in range(9):
        out = ref.get_history(np.zeros((6, 9, 2), np.float32))
        assert out.dtype == np.float64 and not out.any() and not np.signbit(out).any()
    assert ref.get_history(np.zeros((6, 9, 2), np.float32), out="flow").dtype == np.float32


@pytest.mark.parametrize("a,b", [(1, 0), (0, 1), (2, -1), (-1, 1)])
def test_constant_integer_flow_accumulates_exactly(a, b):
    """Every field is (a, b): a pixel whose whole path stays inside collects n * (a, b), in the reference's swapped order (the flow's
    x component a moves the ROW), n = the steps of the schedule; with axes "xy" the x component moves the column."""
    H, W, L = 24, 31, 5
    for axes in ("reference", "xy"):
        ref = R.HistoryRef(H, W, L, np.float64, axes)
        flow = np.empty((H, W, 2))
        flow[...] = (a, b)
        for _ in range(L):                     # fill the ring
            ref.get_history(flow)
        for _ in range(L + 1):
            n = len(R.schedule(L, ref.history_index))
            out = ref.get_history(flow)
            dr, dc = (a, b) if axes == "reference" else (b, a)
            yy, xx = np.mgrid[0:H, 0:W]
            # the last position read is the start plus n - 1 steps; its right / lower neighbour (weight 0) may be outside
            stay = np.ones((H, W), bool)
            for k in range(n):
                stay &= (yy + k * dr >= 0) & (yy + k * dr < H) & (xx + k * dc >= 0) & (xx + k * dc < W)
            assert stay.any()
            assert np.array_equal(out[stay], np.broadcast_to(np.array([n * dr, n * dc], np.float64), out[stay].shape))


def test_float32_ring_gives_the_float64_rings_bits():
    H, W, L = 9, 14, 4
    r32, r64 = R.HistoryRef(H, W, L, np.float32), R.HistoryRef(H, W, L, np.float64)
    for i in range(2 * L + 1):
        f = (_field(H, W, 100 + i, np.float32) * np.float32(0.01)).astype(np.float32)
        assert np.array_equal(R.bits(r32.get_history(f)), R.bits(r64.get_history(f.astype(np.float64))))


U = 2.0 ** -53      # unit roundoff of float64


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("W,H", [(1, 1), (6, 1), (1, 4), (5, 3), (37, 23)])
def test_remap_agrees_with_an_independent_interpolator(W, H, dtype):
    """scipy's map_coordinates(order=1, mode="grid-constant", cval=0) is bilinear interpolation of the field padded with zeros: cv2's
    INTER_LINEAR with BORDER_CONSTANT.  On coordinates that are exact multiples of 1/32 both form the same real-valued sum
    S = sum_i t_i w_i of four taps with the same exact weights (multiples of 1/1024 that add up to 1), each in its own order.
    A four-term sum of rounded products evaluated in any order is within gamma_4 * sum_i |t_i w_i| <= gamma_4 * max_i |t_i| of S
    (gamma_k = k u / (1 - k u), Higham, Accuracy and Stability of Numerical Algorithms, section 3.1; scipy's product t * (wy * wx) rounds
    once, wy * wx being exact), so the two differ by at most 2 gamma_4 max |t_i|: eight ulp-halves of the largest tap."""
    import scipy.ndimage as ndi
    rng = np.random.default_rng(W * 100 + H)
    src = _field(H, W, 7 * W + H, dtype)
    n = 4000
    mx = (rng.integers(-3 * 32, (W + 3) * 32, n) / 32.0).astype(np.float32)
    my = (rng.integers(-3 * 32, (H + 3) * 32, n) / 32.0).astype(np.float32)
    tr = []
    got = R.remap_linear_ref(src, mx, my, tr)
    assert np.array_equal(tr[0]["px"], np.rint(tr[0]["px"]))                   # exact multiples of 1/32: nothing was rounded
    s64 = src.astype(np.float64)
    pad = np.pad(s64, ((2, 2), (2, 2), (0, 0)))                               # the zero border, for the bound's largest tap
    sx, sy = np.clip(tr[0]["sx"], -2, W) + 2, np.clip(tr[0]["sy"], -2, H) + 2
    for ch in range(2):
        want = ndi.map_coordinates(s64[..., ch], [my.astype(np.float64), mx.astype(np.float64)], output=np.float64, order=1,
                                   mode="grid-constant", cval=0.0)
        tmax = np.max(np.abs([pad[sy, sx, ch], pad[sy, sx + 1, ch], pad[sy + 1, sx, ch], pad[sy + 1, sx + 1, ch]]), axis=0)
        bound = 2 * (4 * U / (1 - 4 * U)) * tmax
        err = np.abs(got[..., ch] - want)
        assert (err <= bound).all(), (ch, float((err - bound).max()))
        assert (got[..., ch][tmax == 0] == 0).all()
