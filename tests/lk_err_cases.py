"""TEST INFRASTRUCTURE -- the inputs at which the tracker's `err` form and the Harris score are held to tests/lk_err_ref.py, shared by
tests/test_lk_err_ref_cpu.py and tests/test_gpu_lk_err.py; every reference is computed once per process and handed out read-only."""
from __future__ import annotations

import functools

import numpy as np

import lk_err_ref as er
import sparse_cases as sc
from test_lk_ref_cpu import blurred_noise

F = np.float32

# ---- the final bounds test: points whose last position leaves the bounds while lk_ref keeps them at status 1 ---------------------------
FINAL_W = FINAL_H = 43
FINAL_WIN = (21, 21)
FINAL_KW = dict(win=FINAL_WIN, min_eig_threshold=0, max_count=1)
FINAL_RUNS = ((6, 0), (6, 3), (-6, 0), (-6, 3))              # (shift of the second frame along x, max_level)
# points lk_ref leaves at status 1 whose final position is outside the bounds, per run (the restatement's own count)
FINAL_OUTSIDE = {(6, 0): 5, (6, 3): 3, (-6, 0): 18, (-6, 3): 7}


def final_points() -> np.ndarray:
    """80 points: 40 whose window starts within 3 px of the level's right end, 40 within 3 px of -win_w on the left"""
    W, H, win = FINAL_W, FINAL_H, FINAL_WIN
    halfx = (win[0] - 1) * 0.5
    xs = np.concatenate([W - 1 + halfx - np.linspace(0, 3, 40), -win[0] + halfx + np.linspace(0, 3, 40)])
    ys = np.tile(np.linspace(5, H - 6, 8), 10)
    return np.stack([xs, ys], axis=1).astype(F)


@functools.lru_cache(maxsize=None)
def final_frames(shift: int):
    a = blurred_noise(FINAL_W, FINAL_H, 3)
    b = np.ascontiguousarray(np.roll(a, shift, axis=1))
    for x in (a, b):
        x.setflags(write=False)
    return a, b


def _frozen(res):
    for x in res:
        if isinstance(x, np.ndarray):
            x.setflags(write=False)
    return res


@functools.lru_cache(maxsize=None)
def final_reference(shift: int, max_level: int, flags: int = 0):
    a, b = final_frames(shift)
    return _frozen(er.lk_track_err(a, b, final_points(), flags=flags, max_level=max_level, want_sums=True, **FINAL_KW))


# ---- sparse_cases' tracks through the err form ---------------------------------------------------------------------------------------------
def tracks_of(c: sc.Case):
    """(index, track) of a case without the full point buffer (65 536 points: lk_ref's minutes, and nothing the err form adds)"""
    return [(i, t) for i, t in enumerate(c.tracks) if not (t.points == "inside" and t.n == sc.MAX_POINTS)]


@functools.lru_cache(maxsize=None)
def reference(case_name: str, i: int, flags: int = 0, want_err: bool = True):
    """lk_err_ref's answer for track i of a sparse_cases case: (out, status, err, hist, exits, sums)"""
    c = next(c for c in sc.CASES if c.name == case_name)
    t = c.tracks[i]
    a, b = c.frames(t)
    return _frozen(er.lk_track_err(a, b, c.points(t), flags=flags, want_err=want_err, want_sums=True, **t.params()))


# the GPU table: frames and tracks of sparse_cases the err form runs on the device
GPU_CASES = ((17, 9), (43, 43), (161, 123), (320, 240))


# ---- Harris ----------------------------------------------------------------------------------------------------------------------------------
HARRIS_KS = (0.04, 0.15)
HARRIS_FRAMES = ((1, 1), (1, 9), (2, 2), (3, 3), (5, 3), (17, 9), (43, 41), (161, 123), (320, 240))
STEP_W, STEP_H = 161, 123


def step_image() -> np.ndarray:
    """a single vertical step 40 | 220 at the middle column: an edge, no corner"""
    img = np.full((STEP_H, STEP_W), 40, np.uint8)
    img[:, STEP_W // 2:] = 220
    return img


@functools.lru_cache(maxsize=None)
def harris(kind: str, W: int, H: int, block_size: int, k: float) -> np.ndarray:
    r = er.harris_response(sc.image(kind, W, H), block_size, k)
    r.setflags(write=False)
    return r
