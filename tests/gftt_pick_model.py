"""CPU model in numpy of the DEVICE scheme of the Shi-Tomasi corner pick, on plain (keys, W, H, params), and
the candidate step with cv2's mask restated on lk_ref.min_eigen.  Written from DESIGN.md, not from the product; no import from it.

A candidate is the 64-bit key (float32 value bits << 32) | linear index.  The device
  1. sorts the keys in place, descending, with a bitonic network over Np = n rounded up to a power of two (zero keys as padding);
  2. walks the sorted keys in chunks of CHUNK = 1024 ranks with ONE workgroup.  Accepted corners of earlier chunks live in a grid of
     cells of ceil(min_distance) pixels with a fixed number of slots per cell.  Per chunk: candidates in range of a grid corner are
     rejected, the survivors are compacted in rank order, then ROUNDS decide them: an undecided survivor walks a pointer over the
     earlier survivors; at one in range it stops -- rejected if that one is accepted, waiting if it is undecided, on if it is rejected;
     past the last one it is accepted.  Accepted survivors take the next output places in rank order (cut at max_corners) and enter
     the grid.  The walk ends with the candidates or with max_corners corners.
The model takes every round's decisions from the states at the round's START (the slowest schedule the device may show: on the device
a state written earlier in the same round may already be seen), so its round count bounds the device's from above.

`sequential` is the rule both must equal: lk_ref.good_features's loop applied to a key list."""
import numpy as np

F = np.float32
CAPACITY = 262144          # MAV_GFTT_MAX_CANDIDATES
SORT_CHUNK = 4096          # keys a workgroup sorts in LDS
CHUNK = 1024               # ranks per pick chunk = threads of the pick's workgroup


def keys_of(values, idx):
    """(float32 value bits << 32) | linear index, uint64."""
    v = np.ascontiguousarray(values, F).view(np.uint32).astype(np.uint64)
    return (v << np.uint64(32)) | np.asarray(idx).astype(np.uint64)


def index_of(keys):
    return (np.asarray(keys, np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.int64)


# ---- the rule ------------------------------------------------------------------------------------------------------------------------
def sequential(keys, W, max_corners=2000, min_distance=7.0):
    """Keys descending, then lk_ref.good_features's loop: accept unless an accepted corner lies nearer than min_distance; stop at
    max_corners.  (n, 2) float32 (x, y)."""
    idx = index_of(np.sort(np.asarray(keys, np.uint64))[::-1])
    xs, ys = idx % W, idx // W
    md2 = float(min_distance) * float(min_distance)
    sel = np.zeros((max_corners, 2), np.int64)
    n = 0
    for k in range(len(idx)):
        if n == max_corners:
            break
        if min_distance >= 1 and n:
            d = sel[:n] - (xs[k], ys[k])
            if np.any(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] < md2):
                continue
        sel[n] = (xs[k], ys[k])
        n += 1
    return sel[:n].astype(F)


# ---- the device scheme ---------------------------------------------------------------------------------------------------------------
def sort_keys(keys):
    """The bitonic network as the device runs it: pad to Np with zero keys, steps (k, j) for k = 2 .. Np, j = k / 2 .. 1; the pair
    (i, i | j) is exchanged when (a < b) == ((i & k) == 0).  Steps with j < SORT_CHUNK run in LDS, the others one launch each: the
    network is the same.  Returns (sorted keys [:n], number of global-memory steps)."""
    keys = np.asarray(keys, np.uint64)
    n = len(keys)
    assert n <= CAPACITY
    Np = 1 if n <= 1 else 1 << int(n - 1).bit_length()
    s = np.zeros(Np, np.uint64)
    s[:n] = keys
    t = np.arange(Np // 2, dtype=np.int64)
    global_steps = 0
    k = 2
    while k <= Np:
        j = k >> 1
        while j > 0:
            i = ((t & ~(j - 1)) << 1) | (t & (j - 1))
            l = i | j
            a, b = s[i], s[l]
            swap = (a < b) == ((i & k) == 0)
            s[i], s[l] = np.where(swap, b, a), np.where(swap, a, b)
            global_steps += j >= SORT_CHUNK
            j >>= 1
        k <<= 1
    return s[:n], global_steps


def grid_shape(W, H, min_distance):
    """cell = ceil(min_distance), at most max(W, H) (one cell); slots per cell: corners pairwise >= min_distance apart inside
    cell x cell pixels (coordinates span cell - 1 < min_distance): 1 for cell 1, 2 for cell 2 (a diagonal pair), else one per quadrant."""
    cell = int(min(np.ceil(min_distance), max(W, H)))
    gw, gh = (W + cell - 1) // cell, (H + cell - 1) // cell
    return cell, gw, gh, (1 if cell == 1 else 2 if cell == 2 else 4)


def pick(sorted_keys, W, H, max_corners=2000, min_distance=7.0):
    """The chunked pick on keys already sorted descending.  Returns ((n, 2) float32 corners, stats) with stats = dict(chunks, rounds,
    max_rounds = the most rounds one chunk needed)."""
    idx = index_of(sorted_keys)
    n = len(idx)
    if min_distance < 1:
        m = min(n, max_corners)
        return np.stack([idx[:m] % W, idx[:m] // W], axis=1).astype(F).reshape(-1, 2), dict(chunks=0, rounds=0, max_rounds=0)
    md2 = float(min_distance) * float(min_distance)
    cell, gw, gh, slots = grid_shape(W, H, min_distance)
    assert gw * gh * slots <= max(W * H, 2 * ((W + 1) // 2) * ((H + 1) // 2), 4 * ((W + 2) // 3) * ((H + 2) // 3))   # the workspace it lives in
    grid = np.zeros((gh, gw, slots), np.int64)                 # linear index + 1, filled front to back
    out = []
    acc = chunks = rounds = max_rounds = 0
    base = 0
    while base < n and acc < max_corners:
        ci = idx[base:base + CHUNK]
        x, y = ci % W, ci // W
        # 1. against the grid
        alive = np.ones(len(ci), bool)
        cx, cy = x // cell, y // cell
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                yy, xx = cy + dy, cx + dx
                ok = (yy >= 0) & (yy < gh) & (xx >= 0) & (xx < gw)
                v = grid[np.clip(yy, 0, gh - 1), np.clip(xx, 0, gw - 1)]                   # (m, slots)
                ox, oy = (v - 1) % W, (v - 1) // W
                near = ((x[:, None] - ox) ** 2 + (y[:, None] - oy) ** 2).astype(np.float64) < md2
                alive &= ~(ok[:, None] & (v > 0) & near).any(axis=1)
        sx, sy = x[alive], y[alive]                                                       # survivors in rank order
        S = len(sx)
        # 2. rounds
        inr = ((sx[:, None] - sx[None, :]) ** 2 + (sy[:, None] - sy[None, :]) ** 2).astype(np.float64) < md2
        inr &= np.tri(S, S, -1, dtype=bool)                                               # only earlier survivors
        state = np.zeros(S, np.int8)                                                      # 0 undecided, 1 accepted, 2 rejected
        ptr = np.zeros(S, np.int64)
        r = 0
        while True:
            und = np.nonzero(state == 0)[0]
            if len(und):
                snap = state.copy()
                block = inr[und] & (snap != 2)[None, :] & (np.arange(S)[None, :] >= ptr[und][:, None])
                has = block.any(axis=1)
                first = np.where(has, block.argmax(axis=1), und)                           # the survivor the pointer stops at
                ptr[und] = first
                state[und[~has]] = 1
                hit = has & (snap[first] == 1)
                state[und[hit]] = 2
            r += 1
            if not (state == 0).any():
                break
        rounds += r
        max_rounds = max(max_rounds, r)
        # 3. output places in rank order, the grid
        for xa, ya in zip(sx[state == 1], sy[state == 1]):
            if acc < max_corners:
                out.append((xa, ya))
                free = np.nonzero(grid[ya // cell, xa // cell] == 0)[0]
                assert len(free), "a cell holds more corners than its slots"
                grid[ya // cell, xa // cell, free[0]] = ya * W + xa + 1
            acc += 1
        base += CHUNK
        chunks += 1
    return np.array(out, F).reshape(-1, 2), dict(chunks=chunks, rounds=rounds, max_rounds=max_rounds)


def good_features_from_keys(keys, W, H, max_corners=2000, min_distance=7.0, want_stats=False):
    """Sort and pick as the device does them."""
    s, _ = sort_keys(keys)
    out, stats = pick(s, W, H, max_corners, min_distance)
    return (out, stats) if want_stats else out


# ---- candidate families (plain key lists; values are positive float32, so their bits order as they do) ----------------------------------
def ramp(n, W, H, step=2):
    """n candidates `step` px apart along a line with falling values: along a row, down by one candidate at the row's end, back along the
    row 2 * step below, and so on (a snake).  With step < min_distance <= step * sqrt(2) every candidate is in range of its predecessor
    only, so the greedy rule decides them strictly one after the other."""
    per_row = (W - 2) // step
    assert n <= (per_row + 1) * ((H - 2) // (2 * step))
    k = np.arange(n)
    row, pos = k // (per_row + 1), k % (per_row + 1)
    turn = pos == per_row                                       # the candidate between this row's end and the next row's start
    col = np.where(turn, per_row - 1, pos)
    col = np.where(row % 2 == 0, col, per_row - 1 - col)
    idx = (1 + row * 2 * step + np.where(turn, step, 0)) * W + 1 + col * step
    return keys_of(np.linspace(2.0, 1.0, n).astype(F), idx)


def plateau(W, H, seed=0):
    """Blocks of 8-neighbours with EQUAL values (both pass a non-maximum test that uses >), a few values only."""
    rng = np.random.default_rng(seed)
    img = np.repeat(np.repeat(rng.integers(1, 5, ((H + 2) // 3, (W + 3) // 4)), 3, axis=0), 4, axis=1)[:H, :W].astype(F)
    m = rng.random((H, W)) < 0.6
    m[0, :] = m[-1, :] = False
    m[:, 0] = m[:, -1] = False
    ys, xs = np.nonzero(m)
    return keys_of(img[ys, xs], ys * W + xs)


def all_equal(W, H, every=1):
    """Every `every`-th interior pixel with one value: the order is by index alone."""
    idx = np.arange(W * H).reshape(H, W)[1:-1, 1:-1].reshape(-1)[::every]
    return keys_of(np.full(len(idx), 0.5, F), idx)


def random_set(W, H, n, seed=0, levels=0):
    """n distinct pixels with random values (levels > 0: that many distinct values, so ties abound)."""
    rng = np.random.default_rng(seed)
    idx = rng.choice(W * H, n, replace=False)
    v = rng.random(n).astype(F) + F(0.01) if not levels else (rng.integers(1, levels + 1, n) / F(levels)).astype(F)
    return keys_of(v, idx)


# ---- the candidate step with cv2's mask ------------------------------------------------------------------------------------------------
def masked_candidates(eig, mask=None, quality_level=0.2):
    """goodFeaturesToTrack's candidates with a mask, as cv2 does it: the maximum that quality_level multiplies is taken over the pixels
    where the mask is non-zero (minMaxLoc(eig, ..., mask)); the threshold and the 3 x 3 non-maximum test see the whole map (a
    masked-out neighbour still suppresses); a pixel becomes a candidate only where the mask is non-zero.  An all-zero mask: none.
    (values, linear indices) in the order of the pick, as lk_ref.corner_candidates."""
    H, W = eig.shape
    m = np.ones((H, W), bool) if mask is None else np.asarray(mask) != 0
    if not m.any():
        return np.zeros(0, F), np.zeros(0, np.int64)
    thr = F(np.float64(eig[m].max()) * quality_level)
    e = np.where(eig > thr, eig, F(0))
    p = np.pad(e, 1, mode="constant", constant_values=-np.inf)
    nb = np.max([p[j:j + H, i:i + W] for j in range(3) for i in range(3)], axis=0)
    c = (e != 0) & (e == nb) & m
    c[0, :] = c[-1, :] = False
    c[:, 0] = c[:, -1] = False
    ys, xs = np.nonzero(c)
    v, idx = e[ys, xs], ys * W + xs
    order = np.lexsort((-idx, -v))
    return v[order], idx[order]


def good_features_masked(img, mask=None, max_corners=2000, quality_level=0.2, min_distance=7, block_size=7):
    """cv2.goodFeaturesToTrack(img, max_corners, quality_level, min_distance, mask=mask, blockSize=block_size) -> (n, 2) float32."""
    import lk_ref
    eig = lk_ref.min_eigen(img, block_size)
    v, idx = masked_candidates(eig, mask, quality_level)
    return sequential(keys_of(v, idx), eig.shape[1], max_corners, min_distance)
