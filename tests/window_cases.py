"""TEST INFRASTRUCTURE -- the frames, images and start windows at which every kernel of the window search (csrc/kernels_window.hip:
the INTER_AREA pyramid, the window scan, the summed-area table, optimize_window) is held to oracle/pyramid_oracle.py by
tests/test_gpu_window_forms.py, and the form each kernel takes there.  The counterpart of tests/stage_cases.py (flow path),
tests/detect_cases.py (detection path) and tests/sparse_cases.py (sparse path).

Every predicate below restates one decision of a kernel or a launcher and cites the line it mirrors; tests/test_window_cases_cpu.py
derives the forms each case reaches from these predicates and from the oracle's own walk, and fails when a form of FORMS is no longer
reached, when an image is not what its name says, or when a walk of optimize_window comes near the kernel's step cap.
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass, field

import numpy as np

from oracle import pyramid_oracle as po

WIN, STEP = po.WIN, po.STEP
FORMS = {
    "area.first": {"first", "no-first"},                # AreaSpan.first: a partial first source cell
    "area.last": {"last", "no-last"},
    "area.clamp": {"clamp"},                            # s2 cut at ssize - 1
    "area.scale": {"1.5", "other"},
    "scan": {"none", "none:frame", "one", "nwx<=256", "nwx>256", "nwx>256:wins", "level>0-wins", "level>0-wins:b>0", "tie:levels", "tie:level", "tie:window"},
    "sat": {"w<256", "w%256", "w=k*256", "h1"},
    "opt": {"clip-left", "clip-top", "clip-right", "clip-bottom", "wrap", "outside", "empty", "zero-image", "long-walk"},
}
# Not reached, on purpose:
#   k_optimize_window's loop ending at max_steps = 4 (W + H) + 64: every step strictly raises a sum bounded by the image, and the
#   longest walk there is (a uniform image) takes about W + H steps; tests/test_window_cases_cpu.py holds every case below the cap.
#   A walk that reached it would be a kernel bug to fix, not an input to keep.
#   k_area_resize's clamp of rintf(sum) to [0, 255]: the weights of a destination pixel sum to 1 within rounding, so a u8 source
#   cannot leave the range by half a unit.
UNTESTED = {"opt": {"max_steps"}, "area.clamp": {"saturate"}}


# ---- the dispatch, restated -----------------------------------------------------------------------------------------------------
def area_spans(ssize: int, dsize: int) -> list:
    """area_span for every destination index of an axis: `s1 = ceil(f1), s2 = floor(f2); s2 = min(s2, ssize - 1); s1 = min(s1, s2);
    first = s1 - f1 > 1e-3; last = f2 - s2 > 1e-3` with launch_area_resize's `scale = 1.0 / ((double)dsize / ssize)`:
    [(s1, s2, first, last, clamped)]."""
    scale = 1.0 / (dsize / ssize)
    out = []
    for d in range(dsize):
        f1 = d * scale
        f2 = f1 + scale
        s1, s2 = math.ceil(f1), math.floor(f2)
        clamped = s2 > ssize - 1
        s2 = min(s2, ssize - 1)
        s1 = min(s1, s2)
        out.append((s1, s2, s1 - f1 > 1e-3, f2 - s2 > 1e-3, clamped))
    return out


def area_forms(ssize: int, dsize: int) -> set:
    out = {("area.scale", "1.5" if 1.0 / (dsize / ssize) == 1.5 else "other")}
    for s1, s2, first, last, clamped in area_spans(ssize, dsize):
        out.add(("area.first", "first" if first else "no-first"))
        out.add(("area.last", "last" if last else "no-last"))
        if clamped:
            out.add(("area.clamp", "clamp"))
    return out


def windows_of(w: int, h: int):
    """launch_level_scan: `nwx = W >= 64 ? (W - 64) / 16 + 1 : 0`, the same for nwy; no launch unless both are positive."""
    return ((w - WIN) // STEP + 1 if w >= WIN else 0), ((h - WIN) // STEP + 1 if h >= WIN else 0)


def scan_form(w: int, h: int) -> str:
    """k_level_scan: one workgroup per window row, `for (wx = tid; wx < nwx; wx += 256)`."""
    nwx, nwy = windows_of(w, h)
    if nwx == 0 or nwy == 0:
        return "none"
    if nwx * nwy == 1:
        return "one"
    return "nwx>256" if nwx > 256 else "nwx<=256"


def sat_forms(W: int, H: int) -> set:
    """k_sat_rows: `chunk = (W + 255) / 256, x0 = tid * chunk, x1 = min(x0 + chunk, W)`: below 256 columns the threads from W on have
    empty chunks, at a multiple of 256 every chunk is whole, otherwise the last ones are short or empty."""
    out = {"w<256" if W < 256 else ("w=k*256" if W % 256 == 0 else "w%256")}
    if H == 1:
        out.add("h1")
    return out


def step_cap(W: int, H: int) -> int:
    """k_optimize_window: `max_steps = 4 * (W + H) + 64`."""
    return 4 * (W + H) + 64


def _slice(a: int, n: int, events: set, side: str) -> int:
    """slice_index: `if (a < 0) a += n; return a < 0 ? 0 : (a > n ? n : a)` -- and which way it went"""
    if a < 0:
        a += n
        events.add("wrap" if a >= 0 else "clip-" + side[0])
    if a > n:
        events.add("clip-" + side[1])
    return min(max(a, 0), n)


def walk(img: np.ndarray, window):
    """optimize_window (detector.py:314-358) once more, with the bookkeeping the oracle has no need for: (score, (x, y, w, h), steps,
    events of slice_index over every candidate of every step).  tests/test_window_cases_cpu.py holds its result to the oracle's."""
    img = np.asarray(img)
    H, W = img.shape
    ii = np.zeros((H + 1, W + 1), np.int64)
    ii[1:, 1:] = np.cumsum(np.cumsum(img.astype(np.int64), axis=0), axis=1)
    x, y, w, h = (int(v) for v in window)
    res_score, res, steps, events = 0, (x, y, x + w, y + h), 0, set()
    while True:
        l, t, r, b = res
        best_s, best = 0, res
        for hh in (0, 1):
            for i in (-1, 1):
                for j in (-1, 1):
                    cl, ct, cr, cb = (l + i, t + j, r, b) if hh == 0 else (l, t, r + i, b + j)
                    x0, x1 = _slice(cl, W, events, ("left", "right")), _slice(cr, W, events, ("left", "right"))
                    y0, y1 = _slice(ct, H, events, ("top", "bottom")), _slice(cb, H, events, ("top", "bottom"))
                    s = 3 * int(ii[y1, x1] - ii[y0, x1] - ii[y1, x0] + ii[y0, x0]) if y0 < y1 and x0 < x1 else 0
                    if s > best_s:
                        best_s, best = s, (cl, ct, cr, cb)
        if best_s <= res_score:
            break
        res_score, res, steps = best_s, best, steps + 1
    l, t, r, b = res
    return res_score, (l, t, r - l, b - t), steps, events


# ---- images --------------------------------------------------------------------------------------------------------------------------
DOTS = ((30, 30), (100, 30), (30, 100), (100, 100))       # 70 px apart: a level-0 window holds one of them, a level-1 window all four
BAND = 24                                                  # the darker band's width: no multiple of the stride


@functools.lru_cache(maxsize=None)
def image(kind: str, W: int, H: int) -> np.ndarray:
    if kind == "noise":
        img = np.random.default_rng(500 + 3 * W + H).integers(0, 256, (H, W), dtype=np.uint8)
    elif kind == "uniform":
        img = np.full((H, W), 255, np.uint8)
    elif kind == "band":                                   # uniform 255 with a darker left band
        img = np.full((H, W), 255, np.uint8)
        img[:, :BAND] = 200
    elif kind == "right":                                  # dim noise, the last 70 columns at 255: the last window of a row wins
        img = np.random.default_rng(600 + 3 * W + H).integers(0, 128, (H, W), dtype=np.uint8)
        img[:, W - 70:] = 255
    elif kind == "zero":
        img = np.zeros((H, W), np.uint8)
    elif kind == "dots":                                   # tests/test_gpu_window.py's four dots
        img = np.zeros((H, W), np.uint8)
        for cx, cy in DOTS:
            img[cy:cy + 6, cx:cx + 6] = 255
    else:
        raise KeyError(kind)
    img.setflags(write=False)
    return img


def _f(*names):
    return frozenset(names)


@dataclass(frozen=True)
class Case:
    W: int
    H: int
    kinds: tuple                                            # the images of the batch, in this order
    opt: tuple = ()                                         # names of START_WINDOWS run on every image of the batch
    expects: frozenset = field(default_factory=frozenset)

    @property
    def name(self) -> str:
        return f"{self.W}x{self.H}"

    def batch(self) -> np.ndarray:
        return np.stack([image(k, self.W, self.H) for k in self.kinds])

    def dims(self) -> list:
        return po.pyramid_dims(self.W, self.H)


def start_windows(W: int, H: int) -> dict:
    """name -> (x, y, w, h) of the start windows of optimize_window"""
    return {
        "inside": (W // 3, H // 3, min(8, W), min(8, H)),
        "clip-right-bottom": (W - 30, H - 30, 64, 64),                   # sticks out of the image: the slice ends clip
        "wrap": (-5, -3, 20, 20),                                        # negative starts wrap once, as Python's slices do
        "clip-left": (-W - 10, 0, W + 40, min(20, H)),                   # still negative after the wrap: clipped to 0
        "clip-top": (0, -H - 10, min(20, W), H + 40),
        "outside": (W + 10, H + 10, 20, 20),                             # wholly outside: no neighbour has a positive sum, 0 steps
        "empty": (W // 2, H // 2, 0, 0),                                 # a 0 x 0 window grows from nothing
        "middle": (W // 2 - 4, H // 2 - 4, 8, 8),                        # on a uniform image: the long walk to the whole frame
        "corner": (0, 0, 1, 1),                                          # only the bottom-right corner can move: max(W, H) - 1 steps
    }


ALL_OPT = ("inside", "clip-right-bottom", "wrap", "clip-left", "clip-top", "outside", "empty", "middle")
CASES = [
    Case(63, 100, ("noise", "uniform"), expects=_f("none", "none:frame")),
    Case(64, 64, ("noise", "uniform"), expects=_f("one", "tie:window")),
    Case(80, 64, ("noise", "uniform", "band"), opt=("inside", "empty"), expects=_f("nwx<=256", "tie:level")),          # two windows
    Case(96, 96, ("noise", "uniform", "zero"), expects=_f("one", "1.5", "tie:levels", "no-first", "no-last")),        # level 1 is 64 x 64
    Case(97, 146, ("noise", "band", "uniform"), opt=ALL_OPT, expects=_f("other", "clamp", "w<256")),
    Case(333, 217, ("noise", "dots", "band", "zero"), opt=ALL_OPT, expects=_f("level>0-wins", "level>0-wins:b>0", "w%256", "zero-image")),
    Case(4176, 100, ("noise", "uniform", "band", "right"), expects=_f("nwx>256", "nwx>256:wins")),      # 258 windows per row at level 0, 171 at level 1
    Case(256, 70, ("noise", "uniform"), opt=("inside", "clip-right-bottom", "middle", "corner"), expects=_f("w=k*256")),
    Case(512, 70, ("noise", "uniform"), opt=("inside", "wrap", "middle", "corner"), expects=_f("w=k*256")),
    Case(100, 70, ("noise", "uniform"), opt=("inside", "clip-left", "middle", "corner"), expects=_f("w<256")),
    Case(70, 1, ("noise",), opt=("inside", "empty"), expects=_f("h1")),
    Case(1000, 70, ("uniform", "noise"), opt=("middle", "empty", "corner"), expects=_f("long-walk", "w%256")),
    Case(70, 1000, ("uniform", "noise"), opt=("middle", "empty", "corner"), expects=_f("long-walk", "w<256")),
]
CASE_IDS = [c.name for c in CASES]


@functools.lru_cache(maxsize=None)
def levels(kind: str, W: int, H: int) -> tuple:
    """the oracle's pyramid of an image"""
    out = tuple(po.pyramid(image(kind, W, H)))
    for l in out:
        l.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def analysis(kind: str, W: int, H: int) -> tuple:
    """(the oracle's analyze_pyramid, the levels that hold a window of the best score, how many windows of the winning level hold
    it, how often the winning window holds its maximum)"""
    best = po.analyze_pyramid(image(kind, W, H))
    if best[0] == 0:
        return best, 0, 0, 0
    per_level = [[s for s, _, _ in po._scan(im)] for im in levels(kind, W, H)]
    at = [lv for lv, ss in enumerate(per_level) if best[0] in ss]
    s, x, y, lv = best[:4]
    w = levels(kind, W, H)[lv][y:y + WIN, x:x + WIN]
    return best, len(at), per_level[lv].count(s), int((w == w.max()).sum())


def window_max_reference(kind: str, W: int, H: int) -> tuple:
    """(score, x, y) of the level-0 scan alone: the first window with the strictly largest sum, zeros when none is positive"""
    best = (0, 0, 0)
    for s, x, y in po._scan(image(kind, W, H)):
        if best[0] < s:
            best = (s, x, y)
    return best


def opt_pairs(c: Case) -> list:
    """[(kind, start)] of the case's optimize_window calls: every start window on every image of the batch"""
    return [(k, s) for k in c.kinds for s in c.opt]


@functools.lru_cache(maxsize=None)
def opt_reference(kind: str, W: int, H: int, start: str):
    """(score, window, steps, events) of walk() from a named start window"""
    return walk(image(kind, W, H), start_windows(W, H)[start])


def opt_forms(kind: str, W: int, H: int, start: str) -> set:
    score, win, steps, events = opt_reference(kind, W, H, start)
    out = set(events)
    if start in ("outside", "empty"):
        out.add(start)
    if kind == "zero":
        out.add("zero-image")
    if steps > min(W, H):
        out.add("long-walk")
    return out


def case_forms(c: Case) -> set:
    out = set()
    dims = c.dims()
    for (sw, sh), (dw, dh) in zip(dims, dims[1:]):
        out |= area_forms(sw, dw) | area_forms(sh, dh)
    for w, h in dims:
        out.add(("scan", scan_form(w, h)))
    if all(scan_form(w, h) == "none" for w, h in dims):        # no launch of k_level_scan at all: the key stays 0, k_pyramid_finalize writes zeros
        out.add(("scan", "none:frame"))
    for b, kind in enumerate(c.kinds):
        best, n_levels, n_windows, n_pixels = analysis(kind, c.W, c.H)
        if best[0] and best[1] // STEP >= 256:                 # the winner is a window of the loop's second turn (wx >= 256)
            out.add(("scan", "nwx>256:wins"))
        if best[3] > 0:
            out.add(("scan", "level>0-wins"))
            if b > 0:
                out.add(("scan", "level>0-wins:b>0"))
        if n_levels > 1:
            out.add(("scan", "tie:levels"))
        if n_windows > 1:
            out.add(("scan", "tie:level"))
        if n_pixels > 1:
            out.add(("scan", "tie:window"))
        for start in c.opt:
            out |= {("opt", f) for f in opt_forms(kind, c.W, c.H, start)}
    if c.opt:
        out |= {("sat", f) for f in sat_forms(c.W, c.H)}
    return out
