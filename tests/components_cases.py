"""The case table of the connected-components tests: the smallest shapes at which the passes of csrc/kernels_components.hip can go
wrong, and predicates that restate each dispatch decision of that file on a case's data, so that the CPU test notices when a form is
no longer reached.  The tile size comes from one place: mavflow._lib (held to include/mavflow.h by tests/test_abi_components.py)."""
import functools

import numpy as np

import components_ref as R
from mavflow._lib import CC_TILE_H as T_H
from mavflow._lib import CC_TILE_W as T_W

WAVE, CHUNK = 64, 256                        # lanes of a wave; pixels of a rank chunk (one workgroup of the per-pixel passes)

FRAMES = [(1, 1), (1, 37), (37, 1), (2, 2), (T_W, T_H), (T_W + 1, T_H + 1), (2 * T_W - 1, 3 * T_H + 1), (131, 67)]      # (W, H)
DENSITIES = (0.05, 0.41, 0.59, 0.90)         # 0.41 / 0.59: next to the 8- / 4-connectivity percolation thresholds


def _serpentine(W, H):
    m = np.zeros((H, W), np.uint8)
    m[0::2] = 1
    for y in range(1, H, 2):
        m[y, W - 1 if (y // 2) % 2 == 0 else 0] = 1
    return m


def _spiral(W, H):
    m = np.zeros((H, W), np.uint8)
    x = y = 0
    dx, dy = 1, 0
    m[0, 0] = 1

    def free(dx, dy):
        nx, ny = x + dx, y + dy
        if not (0 <= nx < W and 0 <= ny < H) or m[ny, nx]:
            return False
        ax, ay = nx + dx, ny + dy
        return not (0 <= ax < W and 0 <= ay < H and m[ay, ax])

    for _ in range(W * H):
        if not free(dx, dy):
            dx, dy = -dy, dx
            if not free(dx, dy):
                break
        x, y = x + dx, y + dy
        m[y, x] = 1
    return m


def _comb(W, H):
    m = np.zeros((H, W), np.uint8)
    m[:, 0::2] = 1
    m[H - 1] = 1
    return m


def _tile_checker(W, H):
    """Full tiles in a checkerboard of tiles: they touch only at tile corners, along diagonals and anti-diagonals."""
    yy, xx = np.mgrid[0:H, 0:W]
    return (((xx // T_W) + (yy // T_H)) % 2 == 0).astype(np.uint8)


def _corner_pairs(W, H):
    """Two pixels across every inner tile corner, alternately on the diagonal and the anti-diagonal, nothing next to them."""
    m = np.zeros((H, W), np.uint8)
    for j, y in enumerate(range(T_H, H, T_H)):
        for k, x in enumerate(range(T_W, W, T_W)):
            if (j + k) % 2 == 0:
                m[y - 1, x - 1] = m[y, x] = 1
            else:
                m[y - 1, x] = m[y, x - 1] = 1
    return m


def _rings(W, H):
    m = np.zeros((H, W), np.uint8)
    for k in range(0, min(W, H) // 2 + 1, 2):
        if W - 2 * k < 1 or H - 2 * k < 1:
            break
        m[k, k:W - k] = m[H - 1 - k, k:W - k] = 1
        m[k:H - k, k] = m[k:H - k, W - 1 - k] = 1
    return m


def _noise(W, H, density, seed):
    return (np.random.default_rng(seed).random((H, W)) < density).astype(np.uint8)


def patterns(W, H):
    """name -> (H, W) u8 mask, in a fixed order."""
    yy, xx = np.mgrid[0:H, 0:W]
    corners = np.zeros((H, W), np.uint8)
    corners[[0, 0, H - 1, H - 1], [0, W - 1, 0, W - 1]] = 1
    out = {
        "empty": np.zeros((H, W), np.uint8),
        "full": np.ones((H, W), np.uint8),
        "corners": corners,
        "checker": ((xx + yy) % 2 == 0).astype(np.uint8),
        "serpentine": _serpentine(W, H),
        "serpentine_t": np.ascontiguousarray(_serpentine(H, W).T),
        "spiral": _spiral(W, H),
        "comb": _comb(W, H),
        "tile_checker": _tile_checker(W, H),
        "corner_pairs": _corner_pairs(W, H),
        "rings": _rings(W, H),
        "values": _noise(W, H, 0.5, 7) * np.random.default_rng(8).choice(np.array([7, 128, 255], np.uint8), (H, W)),
    }
    for i, d in enumerate(DENSITIES):
        out[f"noise_{int(round(d * 100)):02d}"] = _noise(W, H, d, 100 + i)
    return out


class Case:
    """masks (B, H, W) u8 through one call.  max_blobs "fit": at least every image's n_components (full equality of the tables).
    cap_mb: option "cc_workspace_mb" for the call (None = the default; 0 = one image per sub-batch)."""

    def __init__(self, cid, W, H, names, connectivity, min_area=1, max_blobs="fit", cap_mb=None):
        self.id, self.W, self.H, self.names, self.connectivity, self.cap_mb = cid, W, H, tuple(names), connectivity, cap_mb
        self._min_area, self._max_blobs = min_area, max_blobs

    @functools.cached_property
    def masks(self):
        p = patterns(self.W, self.H)
        return np.stack([p[n] for n in self.names])

    @functools.cached_property
    def _full(self):
        """labels and per-image component areas with no filter: what "fit", "above" and "median" are taken from."""
        labels = np.stack([R.label(m, self.connectivity)[0] for m in self.masks])
        return labels, [np.bincount(l.ravel())[1:] for l in labels]

    @property
    def min_area(self):
        areas = np.concatenate(self._full[1] + [np.zeros(1, np.int64)])
        if self._min_area == "above":
            return int(areas.max()) + 1
        if self._min_area == "median":
            return max(2, int(np.median(areas[areas > 0])) + 1)
        return self._min_area

    @property
    def max_blobs(self):
        n = max([len(a) for a in self._full[1]] + [1])
        if self._max_blobs == "fit":
            return n
        if self._max_blobs == "half":
            return max(1, min(len(a) for a in self._full[1]) // 2)
        return self._max_blobs

    @functools.cached_property
    def expected(self):
        """(labels, counts, tables) of components_ref: computed once, shared by every test that needs it."""
        labels, areas = self._full
        counts = np.zeros(len(labels), R.COUNTS_DTYPE)
        tables = np.zeros((len(labels), self.max_blobs), R.BLOB_DTYPE)
        for b, l in enumerate(labels):
            counts[b], tables[b] = R.table_of(l, len(areas[b]), self.min_area, self.max_blobs)
        for a in (labels, counts, tables):
            a.setflags(write=False)
        return labels, counts, tables

    def sub_batches(self, per_image_bytes):
        cap = 256 if self.cap_mb is None else self.cap_mb
        sub = min(max((cap << 20) // per_image_bytes, 1), len(self.names))
        return -(-len(self.names) // sub)


def _cases():
    out = []
    for (W, H) in FRAMES:
        names = list(patterns(W, H))
        for conn in (4, 8):
            out.append(Case(f"{W}x{H}-all-c{conn}", W, H, names, conn))
    W, H = FRAMES[-1]
    W2, H2 = FRAMES[-2]
    out += [
        Case("131x67-b1-c8", W, H, ["noise_41"], 8),
        Case("131x67-b3-c4", W, H, ["noise_59", "rings", "comb"], 4),
        Case("131x67-b3-sub-c8", W, H, ["noise_41", "spiral", "tile_checker"], 8, cap_mb=0),
        Case("131x67-above-c8", W, H, ["noise_41", "corners", "empty"], 8, min_area="above"),
        Case("131x67-median-c4", W, H, ["noise_41", "noise_59", "values"], 4, min_area="median"),
        Case("131x67-median-c8", W, H, ["noise_05", "noise_41"], 8, min_area="median"),
        Case("131x67-trunc-c4", W, H, ["checker", "noise_41", "noise_59"], 4, max_blobs="half"),
        Case("131x67-trunc-one-c8", W, H, ["noise_05", "corners"], 8, max_blobs=1),
        Case(f"{W2}x{H2}-trunc-median-sub-c8", W2, H2, ["noise_41", "noise_05", "values"], 8, min_area="median", max_blobs=3, cap_mb=0),
    ]
    return out


CASES = _cases()
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)


# ---- the dispatch decisions of csrc/kernels_components.hip, restated on a case's data --------------------------------------------------
def workspace_per_image(W, H):
    """cc_workspace_per_image: two int32 planes and two counters per chunk, rounded up to 256 bytes."""
    n = W * H
    return (n * 8 + -(-n // CHUNK) * 8 + 255) & ~255


def tile_kinds(W, H):
    """{"interior", "edge"}: tiles that lie wholly inside the frame, tiles the frame cuts (k_cc_tile's bounds tests)."""
    kinds = set()
    for y0 in range(0, H, T_H):
        for x0 in range(0, W, T_W):
            kinds.add("interior" if x0 + T_W <= W and y0 + T_H <= H else "edge")
    return kinds


def merge_kinds(mask, connectivity):
    """Which unions k_cc_merge makes on one mask: "horizontal" border (up neighbour), "vertical" border (left neighbour) and, for
    8-connectivity, "corner": a diagonal across a tile corner whose straight neighbours are unset (only the diagonal joins them)."""
    m = np.asarray(mask) != 0
    H, W = m.shape
    kinds = set()
    for y in range(T_H, H, T_H):
        if (m[y] & m[y - 1]).any():
            kinds.add("horizontal")
    for x in range(T_W, W, T_W):
        if (m[:, x] & m[:, x - 1]).any():
            kinds.add("vertical")
    if connectivity == 8:
        for y in range(T_H, H, T_H):
            for x in range(T_W, W, T_W):
                if (m[y, x] and m[y - 1, x - 1] and not m[y - 1, x] and not m[y, x - 1]) or \
                        (m[y, x - 1] and m[y - 1, x] and not m[y - 1, x - 1] and not m[y, x]):
                    kinds.add("corner")
    return kinds


def stats_kinds(labels, table):
    """Which paths k_cc_stats' wave loop takes: "uniform" (the lanes of a wave that have a record share one) and "mixed" (several
    records in one wave: the peel loop runs more than once).  A wave = 64 consecutive pixels of the image's linear order."""
    slot_of = {int(r["label"]): i for i, r in enumerate(table) if r["area"] > 0}
    lin = labels.ravel()
    kinds = set()
    for w0 in range(0, lin.size, WAVE):
        slots = {slot_of[int(v)] for v in lin[w0:w0 + WAVE] if int(v) in slot_of}
        if len(slots) == 1:
            kinds.add("uniform")
        elif len(slots) > 1:
            kinds.add("mixed")
    return kinds
