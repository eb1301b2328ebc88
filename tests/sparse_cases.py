"""TEST INFRASTRUCTURE -- the frames, windows, level counts, point sets and coordinates at which every kernel of the sparse path
(csrc/kernels_lk.hip: Shi-Tomasi corners, pyramid, Scharr, the Lucas-Kanade tracker) is held to the numpy restatement (tests/lk_ref.py,
tests/gftt_pick_model.py) by tests/test_gpu_sparse_forms.py, and the form each kernel takes there.  The counterpart of
tests/stage_cases.py (flow path), tests/detect_cases.py (detection path) and tests/window_cases.py (window search).

The kernels take another path on the frame's sides against the tile, the halo and the window, on counts against a workgroup and a
sort chunk, and on where a coordinate falls against the bounds test.  Every predicate below restates one such decision and cites the
line it mirrors; tests/test_sparse_cases_cpu.py derives the forms each case reaches from these predicates and fails when a form of
FORMS is no longer reached, when a case is not what its name says (by the restatement alone), when an exit of the tracker's
iteration is no longer taken, or when a tracker case tracks too little to compare anything.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np

import lk_ref
from test_lk_ref_cpu import blurred_noise

F = np.float32
# include/mavflow.h (tests/test_sparse_cases_cpu.py holds them to mavflow._lib)
MAX_POINTS, MAX_WIN, MAX_LEVEL, MAX_CANDIDATES = 65536, 33, 7, 262144
EIG_TILE, SORT_CHUNK, SCHARR_MAX_BLOCKS = 16, 4096, 4096          # kernels_lk.hip: EIG_TILE, PICK_SORT_CHUNK, launch_lk_scharr

_LV = ("0", "coarser")
FORMS = {
    "eig.r": {"r0", "r1", "r3", "r7"},                             # block_size 1, 3, 7, 15: the LDS halo, 15 its maximum
    "eig.tile": {"full", "ragged", "narrow", "n1", "multi-reflect"},
    "eig.mask": {"none", "mask"},
    "cand": {"whole", "tail", "no-interior", "plateau"},
    "sort": {"n0", "n1", "np<=chunk", "np>chunk"},
    "pyrdown": {"odd", "even", "x-whole", "x-tail", "y-whole", "y-tail", "src<=2"},
    "scharr": {"one-pass", "grid-stride", "levels1", "levels8"},
    "track.n": {"n%4=0", "n%4=1", "n%4=2", "n%4=3", "n1", "n_max", "n_dev<n", "n_dev>n", "n_dev<0"},
    "track.win": {"npix<64", "npix%64", "max", "wide", "tall"},
    "track.levels": {"1", "rule-edge-below", "rule-edge-above", "8", "win>frame"},
    "track.exit": {f"{e}:{g}" for e in lk_ref.EXITS for g in _LV},
    "track.coord": {"x=-win", "x<-win", "x=w-1", "x<w", "x=w", "y=-win", "y<-win", "y=h-1", "y<h", "y=h", "nan", "inf", ">=2^31"},
}
# Not reached, on purpose.  Each needs an argument the host entry points refuse before anything is launched, or a count beyond a
# buffer; tests hand kernels neither:
#   k_min_eig with r > EIG_MAX_R (check_gftt_params: block_size <= 15; the LDS tile is sized for 7)
#   k_lk_track with a window above 33 x 33 (check_lk_params; the point's three planes would not fit its LDS block)
#   k_lk_track with an even window: npix % 64 == 0 is possible only then (check_lk_params: odd sides)
#   launch_lk_track with n < 1 (no launch; mav_lk_track with n = 0 returns before it)
#   the sort kernels' `n > cap` exit and the pick's negative count: more candidates than the buffer holds, which
#   tests/test_gpu_lk.py and tests/test_gpu_gftt_device.py reach at 1600 x 1400 -- a frame of 2.2 Mpx is no small case
UNTESTED = {"eig.r": {"r>7"}, "track.win": {"win>33", "npix%64=0"}, "track.n": {"n0:launch"}, "sort": {"n>cap"}}


# ---- the dispatch, restated -----------------------------------------------------------------------------------------------------
def eig_r_form(block_size: int) -> str:
    """launch_min_eig: `r = block_size / 2`."""
    return f"r{block_size // 2}"


def reflections(p: int, n: int) -> int:
    """refl101: `if (n == 1) return 0; while ((unsigned)p >= (unsigned)n) p = p < 0 ? -p : 2 * n - 2 - p;` -- how often the loop runs."""
    k = 0
    if n == 1:
        return 0
    while not 0 <= p < n:
        p = -p if p < 0 else 2 * n - 2 - p
        k += 1
    return k


def eig_tile_forms(W: int, H: int, block_size: int) -> set:
    """k_min_eig: a 16 x 16 tile per workgroup (launch_min_eig: grid (W + 15) / 16, (H + 15) / 16), `if (x < W && y < H)`; the halo
    positions -r .. n - 1 + r of an axis go through refl101.  multi-reflect: a halo position some OUTPUT pixel needs takes more than
    one turn of refl101's loop, which is n <= r (from -r to r, still outside)."""
    r = block_size // 2
    out = set()
    out.add("full" if W % EIG_TILE == 0 and H % EIG_TILE == 0 else "ragged")
    if min(W, H) < EIG_TILE:
        out.add("narrow")
    if min(W, H) == 1:
        out.add("n1")
    if any(n > 1 and max(reflections(-r, n), reflections(n - 1 + r, n)) > 1 for n in (W, H)):
        out.add("multi-reflect")
    return out


def cand_forms(W: int, H: int) -> set:
    """launch_corner_candidates: (W * H + 255) / 256 workgroups, `if (idx >= W * H) return`; k_corner_candidates:
    `if (x < 1 || x > W - 2 || y < 1 || y > H - 2) return`."""
    out = {"tail" if (W * H) % 256 else "whole"}
    if W < 3 or H < 3:
        out.add("no-interior")
    return out


def sort_form(n: int) -> str:
    """k_pick_sort_local: `Np = pick_np2(n)`, `L = Np < PICK_SORT_CHUNK ? Np : PICK_SORT_CHUNK`; launch_pick_sort's global steps act
    when `k <= Np` with k from 2 * PICK_SORT_CHUNK."""
    if n < 2:
        return f"n{n}"
    return "np<=chunk" if n <= SORT_CHUNK else "np>chunk"


def level_dims(W: int, H: int) -> list:
    """mavflow.cpp lk_level_dims: levels 0 .. MAV_LK_MAX_LEVEL, ((w + 1) / 2, (h + 1) / 2), stopping at 1 x 1."""
    out = [(W, H)]
    while len(out) <= MAX_LEVEL and out[-1] != (1, 1):
        w, h = out[-1]
        out.append(((w + 1) // 2, (h + 1) // 2))
    return out


def pyrdown_forms(W: int, H: int) -> set:
    """launch_lk_pyrdown: grid ((dw + 63) / 64, (dh + 3) / 4), `if (x >= dw || y >= dh) return`; refl101(2 x - 2 + i, sw) on a source
    side of 1 or 2 -- over every level the stage hooks build."""
    out = set()
    dims = level_dims(W, H)
    for (sw, sh), (dw, dh) in zip(dims, dims[1:]):
        for s in (sw, sh):
            out.add("odd" if s % 2 else "even")
            if s <= 2:
                out.add("src<=2")
        out.add("x-tail" if dw % 64 else "x-whole")
        out.add("y-tail" if dh % 4 else "y-whole")
    return out


def scharr_forms(W: int, H: int) -> set:
    """launch_lk_scharr: `blocks = (w0 * h0 + 255) / 256; if (blocks > 4096) blocks = 4096`, grid (blocks, levels); the stage hook
    runs it with level + 1 levels, for level 0 up to the frame's last."""
    out = {"grid-stride" if (W * H + 255) // 256 > SCHARR_MAX_BLOCKS else "one-pass", "levels1"}
    if len(level_dims(W, H)) == MAX_LEVEL + 1:
        out.add("levels8")
    return out


def track_levels(W: int, H: int, win, max_level: int) -> int:
    """mavflow.cpp lk_levels_for: `while (n <= max_level && n < dims.n && dims.w[n] > win_w && dims.h[n] > win_h) n++`."""
    d = level_dims(W, H)
    n = 1
    while n <= max_level and n < len(d) and d[n][0] > win[0] and d[n][1] > win[1]:
        n += 1
    return n


def track_level_forms(W: int, H: int, win, max_level: int) -> set:
    """What ends lk_levels_for's loop.  rule-edge: the first level not built misses the window rule by one pixel on a side (and on
    no side by more), or the last level built passes it by exactly one."""
    d = level_dims(W, H)
    n = track_levels(W, H, win, max_level)
    out = set()
    if n == 1:
        out.add("1")
    if n == MAX_LEVEL + 1:
        out.add("8")
    if W < win[0] or H < win[1]:
        out.add("win>frame")
    if n <= max_level and n < len(d):
        gaps = [d[n][0] - win[0], d[n][1] - win[1]]
        if min(gaps) == 0:
            out.add("rule-edge-below")
    if n > 1 and min(d[n - 1][0] - win[0], d[n - 1][1] - win[1]) == 1:
        out.add("rule-edge-above")
    return out


def track_win_forms(win) -> set:
    """k_lk_track: `for (k = lane; k < npix; k += 64)`; lk_track_lds_bytes = 4 * 3 * npix * 2."""
    npix = win[0] * win[1]
    out = set()
    if npix < 64:
        out.add("npix<64")
    elif npix % 64:
        out.add("npix%64")
    else:
        out.add("npix%64=0")
    if win == (MAX_WIN, MAX_WIN):
        out.add("max")
    if win[0] == MAX_WIN and win[1] <= 5:
        out.add("wide")
    if win[1] == MAX_WIN and win[0] <= 5:
        out.add("tall")
    return out


def track_n_forms(n: int) -> set:
    """launch_lk_track: (n + 3) / 4 workgroups of four waves, `p = blockIdx.x * 4 + wv; if (p >= n) return`."""
    out = {f"n%4={n % 4}"}
    if n == 1:
        out.add("n1")
    if n == MAX_POINTS:
        out.add("n_max")
    return out


def n_dev_form(n_dev: int, n_max: int) -> str:
    """k_lk_track: `if (a.n_dev) { m = *a.n_dev; n = m < n ? m : n; }`."""
    if n_dev < 0:
        return "n_dev<0"
    return "n_dev<n" if n_dev < n_max else ("n_dev>n" if n_dev > n_max else "n_dev=n")


# ---- images --------------------------------------------------------------------------------------------------------------------------
def checkerboard(W: int, H: int) -> np.ndarray:
    """2 x 2 squares of 0 and 255: one local maximum per square corner, equal values side by side (tests/test_gpu_lk.py's overflow image)."""
    yy, xx = np.mgrid[0:H, 0:W]
    return ((((yy // 2) + (xx // 2)) & 1) * 255).astype(np.uint8)


def one_corner(W: int, H: int) -> np.ndarray:
    """A flat frame with one bright quadrant whose vertex lies at the frame's middle: a single corner."""
    img = np.full((H, W), 40, np.uint8)
    img[H // 2:, W // 2:] = 220
    return img


@functools.lru_cache(maxsize=None)
def image(kind: str, W: int, H: int, seed: int = 0) -> np.ndarray:
    from mavflow import synth
    if kind == "pair0":
        img = synth.make_pair(W, H, seed)[0]
    elif kind == "pair1":
        img = synth.make_pair(W, H, seed)[1]
    elif kind == "blurred":
        img = blurred_noise(W, H, 3 + seed)
    elif kind == "blurred-moved":              # the blurred texture one row down and two columns right (wrap-around)
        img = np.roll(blurred_noise(W, H, 3 + seed), (1, 2), axis=(0, 1))
    elif kind == "noise":
        img = np.random.default_rng(1000 + 7 * W + H + seed).integers(0, 256, (H, W), dtype=np.uint8)
    elif kind.startswith("rng"):               # uniform noise of that very seed: "rng2789" is a 3 x 3 frame whose one interior pixel is a corner
        img = np.random.default_rng(int(kind[3:])).integers(0, 256, (H, W), dtype=np.uint8)
    elif kind == "flat":
        img = np.full((H, W), 200, np.uint8)
    elif kind == "checker":
        img = checkerboard(W, H)
    elif kind == "corner":
        img = one_corner(W, H)
    else:
        raise KeyError(kind)
    img = np.ascontiguousarray(img)
    img.setflags(write=False)
    return img


def mask_of(W: int, H: int) -> np.ndarray:
    """cv2's mask, a different value per region: the left part 255, a lattice of 1 on the right, the rest 0."""
    m = np.zeros((H, W), np.uint8)
    m[:, :(W + 1) // 2] = 255
    m[::2, 1::3] = 1
    return m


# ---- frames: stage hooks, candidates, corners ------------------------------------------------------------------------------------------
BLOCK_SIZES = (1, 3, 7, 15)
MIN_DISTANCES = (1, 2.5, 7)


def _f(*names):
    return frozenset(names)


@dataclass(frozen=True)
class Frame:
    W: int
    H: int
    kinds: tuple = ("pair0", "blurred", "noise", "flat")
    expects: frozenset = field(default_factory=frozenset)       # forms this frame is here to reach

    @property
    def name(self) -> str:
        return f"{self.W}x{self.H}"

    def images(self) -> dict:
        return {k: image(k, self.W, self.H) for k in self.kinds}


FRAMES = [
    Frame(1, 1, kinds=("pair0", "noise", "flat"), expects=_f("n1", "no-interior", "n0")),
    Frame(1, 9, expects=_f("n1", "no-interior", "src<=2")),
    Frame(9, 1, expects=_f("n1", "no-interior", "src<=2")),
    Frame(2, 2, expects=_f("multi-reflect", "no-interior", "src<=2")),
    Frame(3, 3, kinds=("pair0", "noise", "flat", "rng2789"), expects=_f("narrow", "multi-reflect", "n1")),     # one interior pixel
    Frame(5, 3, kinds=("pair0", "noise", "flat", "rng30"), expects=_f("narrow", "multi-reflect", "n1")),
    Frame(17, 9, kinds=("pair0", "blurred", "noise", "flat", "corner"), expects=_f("narrow", "ragged", "n1")),
    Frame(42, 42, expects=_f("ragged")),
    Frame(43, 43, expects=_f("ragged", "odd")),
    Frame(43, 41, expects=_f("ragged")),
    Frame(257, 19, expects=_f("x-tail", "y-tail", "tail")),                        # dw = 129, dh = 10
    Frame(161, 123, kinds=("pair0", "blurred", "noise", "flat", "checker"), expects=_f("ragged", "plateau", "np>chunk", "levels8")),
    Frame(320, 240, expects=_f("full", "whole", "y-whole")),
    Frame(384, 384, kinds=("pair0", "noise"), expects=_f("full", "even", "x-whole")),
    Frame(385, 385, kinds=("pair0", "noise"), expects=_f("ragged", "odd")),
    Frame(1283, 821, kinds=("pair0", "noise"), expects=_f("grid-stride", "np>chunk")),   # 1 053 343 px
]
FRAME_IDS = [f.name for f in FRAMES]


def frame(W: int, H: int) -> Frame:
    return next(f for f in FRAMES if (f.W, f.H) == (W, H))


@functools.lru_cache(maxsize=None)
def eigen(kind: str, W: int, H: int, block_size: int = 7) -> np.ndarray:
    e = lk_ref.min_eigen(image(kind, W, H), block_size)
    e.setflags(write=False)
    return e


@functools.lru_cache(maxsize=None)
def candidates(kind: str, W: int, H: int):
    """lk_ref's candidates of an image at the default block size and quality level: (values, linear indices) in key order."""
    return lk_ref.corner_candidates(eigen(kind, W, H))


def has_plateau(idx: np.ndarray, v: np.ndarray, W: int) -> bool:
    """two candidates that are 8-neighbours and carry the same value"""
    where = dict(zip(idx.tolist(), v.tolist()))
    return any(where.get(i + d) == val for i, val in where.items() for d in (1, W - 1, W, W + 1))


def frame_forms(f: Frame) -> set:
    out = set()
    for bs in BLOCK_SIZES:
        out.add(("eig.r", eig_r_form(bs)))
        out |= {("eig.tile", t) for t in eig_tile_forms(f.W, f.H, bs)}
    out |= {("eig.mask", "none"), ("eig.mask", "mask")}               # every frame runs good_features with and without mask_of
    out |= {("cand", c) for c in cand_forms(f.W, f.H)}
    out |= {("pyrdown", p) for p in pyrdown_forms(f.W, f.H)}
    out |= {("scharr", s) for s in scharr_forms(f.W, f.H)}
    for kind in f.kinds:
        v, idx = candidates(kind, f.W, f.H)
        out.add(("sort", sort_form(len(idx))))
        if len(idx) <= MAX_POINTS and has_plateau(idx, v, f.W):
            out.add(("cand", "plateau"))
    return out


# ---- tracker ---------------------------------------------------------------------------------------------------------------------------
def inside_points(W: int, H: int, n: int, seed: int = 11) -> np.ndarray:
    """n points at fractional coordinates anywhere inside the frame"""
    return (np.random.default_rng(seed).random((n, 2)) * (max(W - 1, 0), max(H - 1, 0))).astype(F)


def border_points(W: int, H: int, win=(21, 21), seed: int = 12) -> np.ndarray:
    """Points within a window of each border, the four vertices, points outside the frame near and far, NaN and infinities
    (tests/test_gpu_lk.py planted_points, for any frame size)."""
    rng = np.random.default_rng(seed)
    bx, by = min(win[0] // 2 + 2, W - 1), min(win[1] // 2 + 2, H - 1)
    pts = []
    for x0, x1, y0, y1 in ((0, bx, 0, H - 1), (W - 1 - bx, W - 1, 0, H - 1), (0, W - 1, 0, by), (0, W - 1, H - 1 - by, H - 1)):
        pts.append(np.stack([rng.uniform(x0, x1, 6), rng.uniform(y0, y1, 6)], axis=1))
    pts.append(np.array([[0, 0], [W - 1, H - 1], [W - 1, 0], [0.5, H - 1.5], [W / 2, H / 2], [W / 2 + 0.25, H / 2 + 0.75]]))
    pts.append(np.array([[-5.5, H / 3], [-win[0] - 0.5, -win[1] - 0.5], [-2 * win[0], H / 2], [W + 9.9, H / 4], [W + 40, H + 40],
                         [W / 3, -win[1] / 2 - 0.01], [W / 3, H + win[1] / 2 + 0.2], [1e7, 5], [-3e9, 4e9], [1e30, 1e30]]))
    pts.append(np.array([[np.nan, 10], [10, np.nan], [np.nan, np.nan], [np.inf, 10], [10, -np.inf]]))
    return np.concatenate(pts).astype(F)


N_BORDER = 24 + 6                            # border_points' leading points that lie inside the frame


def _aim(target: np.float32, half: np.float32) -> np.float32:
    """The float32 coordinate p with float32(p - half) == target exactly (k_lk_track: `px = ptx * sc; px -= halfx` at level 0, sc = 1),
    as stage_cases._aim finds a displacement: the sum must need no more than 24 bits."""
    p = F(target) + F(half)
    assert F(p - F(half)) == F(target) and float(p) == float(target) + float(half), (target, half)
    return p


def coord_targets(n: int, win_side: int, half) -> dict:
    """label -> the float32 coordinate p whose floor(p - half) sits at an edge of the bounds test `fx >= -win && fx < n` (k_lk_track)
    along an axis of n pixels, as stage_cases.edge_targets lists the dense path's: p - half exactly -win (inside), the float below it
    (outside), exactly n - 1 (inside), exactly n (outside), and the largest p whose difference stays below n (inside, floor n - 1)."""
    half = F(half)
    return {"=-win": _aim(F(-win_side), half), "<-win": _aim(np.nextafter(F(-win_side), F(-np.inf)), half), "=n-1": _aim(F(n - 1), half),
            "<n": np.nextafter(F(n) + half, F(-np.inf)), "=n": _aim(F(n), half)}


def coord_points(W: int, H: int, win=(21, 21)):
    """([label], (n, 2) float32): each target on one axis, the other axis in the middle of the frame; then NaN, infinities and
    magnitudes from 2^31 up (the int conversion of their floor is never taken)."""
    hx, hy = F((win[0] - 1) * 0.5), F((win[1] - 1) * 0.5)
    labels, pts = [], []
    for name, p in coord_targets(W, win[0], hx).items():
        labels.append("x" + name.replace("=n", "=w").replace("<n", "<w")); pts.append((p, F(H // 2 + 0.25)))
    for name, p in coord_targets(H, win[1], hy).items():
        labels.append("y" + name.replace("=n", "=h").replace("<n", "<h")); pts.append((F(W // 2 + 0.75), p))
    for name, p in (("nan", (np.nan, 5)), ("nan", (5, np.nan)), ("inf", (np.inf, 5)), ("inf", (5, -np.inf)), (">=2^31", (2.0 ** 31, 5)),
                    (">=2^31", (5, -2.0 ** 31)), (">=2^31", (-2.0 ** 31 - 256, 3e9)), (">=2^31", (3.4e38, -3.4e38))):
        labels.append(name); pts.append(p)
    return labels, np.array(pts, F)


def coord_claims(W: int, H: int, win=(21, 21)) -> dict:
    """label -> the restatement's status at level 0 alone must be this ("in": the bounds test passes, "out": status 0)"""
    return {"x=-win": "in", "x<-win": "out", "x=w-1": "in", "x<w": "in", "x=w": "out", "y=-win": "in", "y<-win": "out", "y=h-1": "in",
            "y<h": "in", "y=h": "out", "nan": "out", "inf": "out", ">=2^31": "out"}


@dataclass(frozen=True)
class Track:
    """One tracker call: the window, maxLevel, the point set and the remaining parameters."""
    points: str = "mixed"                      # "mixed" (inside + border_points), "inside", "coords", "detected"
    n: int = 0                                 # "inside": that many points; "mixed": that many inside points before the border set
    win: tuple = (21, 21)
    max_level: int = 3
    kw: tuple = ()                             # ((name, value), ...) of lk_ref.lk_track's other parameters
    moved: str = ""                            # the second frame, when not the case's own

    @property
    def label(self) -> str:
        return f"{self.points}{self.n or ''} win={self.win[0]}x{self.win[1]} L={self.max_level} {dict(self.kw) or ''} {self.moved}".strip()

    def params(self) -> dict:
        return dict(win=self.win, max_level=self.max_level, **dict(self.kw))


@dataclass(frozen=True)
class Case:
    W: int
    H: int
    kinds: tuple                               # the two frames
    tracks: tuple
    expects: frozenset = field(default_factory=frozenset)

    @property
    def name(self) -> str:
        return f"{self.W}x{self.H}"

    def frames(self, t: Track = None):
        a = image(self.kinds[0], self.W, self.H)
        if t is not None and t.moved == "far":             # 40 px of motion: beyond the pyramid's reach, points run into maxCount
            return a, np.roll(a, (0, min(40, self.W // 2)), axis=(0, 1))
        if t is not None and t.moved == "flat":            # a flat region in both frames: the min-eigenvalue test rejects points inside
            b = image(self.kinds[1], self.W, self.H)
            a, b = a.copy(), b.copy()
            y0, y1, x0, x1 = self.H // 4, self.H // 4 + self.H // 3, self.W // 3, self.W // 3 + self.W // 3
            a[y0:y1, x0:x1] = 90
            b[y0:y1, x0:x1] = 90
            return a, b
        return a, image(self.kinds[1], self.W, self.H)

    def points(self, t: Track) -> np.ndarray:
        if t.points == "inside":
            return inside_points(self.W, self.H, t.n)
        if t.points == "coords":
            return coord_points(self.W, self.H, t.win)[1]
        if t.points == "detected":
            pts = lk_ref.good_features(image(self.kinds[0], self.W, self.H))
            if t.moved == "flat":              # and points in the middle of the flat region
                cx, cy = self.W // 3 + self.W // 6, self.H // 4 + self.H // 6
                pts = np.concatenate([np.array([[cx, cy], [cx - 9.5, cy - 9.75], [cx + 1, cy + 0.5]], F), pts])
            return pts[:t.n] if t.n else pts
        return np.concatenate([inside_points(self.W, self.H, t.n or 60), border_points(self.W, self.H, t.win)])

    def n_inside(self, t: Track) -> int:
        """the leading points of points(t) that were placed inside the frame"""
        if t.points == "mixed":
            return (t.n or 60) + N_BORDER
        return 0 if t.points == "coords" else len(self.points(t))


PAIR = ("pair0", "pair1")
MOVED = ("blurred", "blurred-moved")
TINY = (Track(n=5), Track(n=6, win=(3, 3)), Track(points="coords"), Track(points="coords", win=(3, 3), max_level=0))
CASES = [
    # frames narrower than the window (and than one tile): every level-0 window leaves the frame on both sides
    Case(1, 1, PAIR, TINY, expects=_f("win>frame", "1")),
    Case(1, 9, PAIR, TINY, expects=_f("win>frame")),
    Case(9, 1, PAIR, TINY, expects=_f("win>frame")),
    Case(2, 2, PAIR, TINY, expects=_f("win>frame")),
    Case(3, 3, PAIR, TINY, expects=_f("win>frame")),
    Case(5, 3, PAIR, TINY + (Track(n=7, win=(5, 3)),), expects=_f("win>frame")),
    Case(17, 9, MOVED, TINY + (Track(n=9, win=(5, 5)), Track(n=10, win=(7, 7), max_level=2)), expects=_f("win>frame", "npix<64")),
    # the window rule with 21 x 21: level 1 is 21 (not built), 22 (built), 22 x 21 (not built)
    Case(42, 42, MOVED, (Track(n=30), Track(points="coords")), expects=_f("rule-edge-below", "1")),
    Case(43, 43, MOVED, (Track(n=30), Track(points="coords"), Track(n=31, max_level=1)), expects=_f("rule-edge-above")),
    Case(43, 41, MOVED, (Track(n=30),), expects=_f("rule-edge-below", "1")),
    Case(257, 19, MOVED, (Track(n=33, win=(33, 5)), Track(n=34, win=(5, 5)), Track(n=35, win=(21, 5), max_level=7), Track(points="coords", win=(33, 5))),
         expects=_f("wide")),
    # ragged tiles; every window form; every residue of n against a workgroup's four waves; one point; the point buffer full
    Case(161, 123, PAIR, (Track(n=60), Track(points="coords"), Track(points="coords", max_level=0), Track(points="inside", n=1),
                          Track(points="inside", n=61), Track(points="inside", n=62), Track(points="inside", n=63), Track(points="inside", n=64),
                          Track(n=40, win=(3, 3)), Track(n=41, win=(5, 5)), Track(n=42, win=(7, 7)), Track(n=43, win=(9, 9)),
                          Track(n=44, win=(33, 33)), Track(n=45, win=(33, 5)), Track(n=46, win=(5, 33)), Track(points="coords", win=(5, 33)),
                          Track(points="coords", win=(33, 33), max_level=0), Track(points="coords", win=(3, 3), max_level=0),
                          Track(points="inside", n=MAX_POINTS, win=(5, 5), max_level=1, kw=(("max_count", 10),))),
         expects=_f("n1", "n_max", "n%4=0", "n%4=1", "n%4=2", "n%4=3", "npix<64", "npix%64", "max", "wide", "tall")),
    # the baseline: detected corners, the flat region, 40 px of motion, the termination criteria at their ends
    Case(320, 240, PAIR, (Track(points="detected"), Track(n=60), Track(points="detected", n=43, moved="flat"),
                          Track(points="detected", n=200, moved="far"), Track(n=60, moved="far"), Track(n=100, kw=(("max_count", 3),)),
                          Track(n=100, kw=(("max_count", 0),)), Track(n=100, kw=(("epsilon", 0.3),)), Track(n=100, kw=(("min_eig_threshold", 0.05),)),
                          Track(points="detected", n=150, kw=(("max_count", 1000), ("epsilon", 0.0))),
                          Track(n=100, max_level=0), Track(n=100, max_level=0, kw=(("max_count", 0),)),
                          Track(n=100, max_level=0, moved="far"), Track(n=100, max_level=0, moved="flat")),
         expects=_f(*(f"{e}:{g}" for e in lk_ref.EXITS for g in _LV))),
    # 3 x 3 window, maxLevel 7: 7 levels (level 7 would be 3 wide) and 8 (4 wide)
    Case(384, 384, PAIR, (Track(n=50, win=(3, 3), max_level=7), Track(n=50, win=(5, 5), max_level=7)), expects=_f("npix<64")),
    Case(385, 385, PAIR, (Track(n=50, win=(3, 3), max_level=7), Track(n=50, win=(7, 7), max_level=7)), expects=_f("8", "rule-edge-above")),
    Case(1283, 821, PAIR, (Track(n=100), Track(n=50, win=(9, 9), max_level=7)), expects=_f()),
]
CASE_IDS = [c.name for c in CASES]
# the frames from which a tracker case must track at least half of the points placed inside it
MIN_TRACKED_SIDE = 43
# the enqueue-only forms (mav_lk_track_ex_dev), on one ragged frame: (count on the device, n_max)
N_DEV_FRAME = (161, 123)
N_DEV_CALLS = ((37, 90), (90, 37), (-7, 90), (90, 90))


def case_of(W: int, H: int) -> Case:
    return next(c for c in CASES if (c.W, c.H) == (W, H))


@functools.lru_cache(maxsize=None)
def reference(case_name: str, i: int):
    """lk_ref's answer for track i of a case: (points, next points, status, iteration histogram, exits)"""
    c = next(c for c in CASES if c.name == case_name)
    t = c.tracks[i]
    a, b = c.frames(t)
    pts = c.points(t)
    out, status, hist, exits = lk_ref.lk_track(a, b, pts, want_hist=True, want_exits=True, **t.params())
    return pts, out, status, hist, exits


def track_forms(c: Case, t: Track, with_exits: bool = True) -> set:
    out = {("track.win", f) for f in track_win_forms(t.win)}
    out |= {("track.levels", f) for f in track_level_forms(c.W, c.H, t.win, t.max_level)}
    out |= {("track.n", f) for f in track_n_forms(len(c.points(t)))}
    if t.points == "coords":
        out |= {("track.coord", l) for l in coord_points(c.W, c.H, t.win)[0] if l in FORMS["track.coord"]}
    if with_exits:
        exits = reference(c.name, c.tracks.index(t))[4]
        out |= {("track.exit", f"{e}:{g}") for (e, g), k in exits.items() if k}
    return out


def case_forms(c: Case) -> set:
    out = set()
    for t in c.tracks:
        out |= track_forms(c, t)
    return out


def other_forms() -> set:
    return {("track.n", n_dev_form(m, n)) for m, n in N_DEV_CALLS if n_dev_form(m, n) in FORMS["track.n"]}
