"""The cases of the robust affine fit (include/mavflow_affine.h), shared by tests/test_affine_ref_cpu.py (the restatement against the
definition) and tests/test_gpu_affine.py (the device against the restatement, byte for byte).  Shapes are the smallest at which the kernels
can go wrong: n around the wavefront (63, 64, 65), the minimum (3, 4), the detector's 1000 and one LDS chunk + 1; max_iters around the
choice kernel's block of 64 and the default 2000; batch 1 and 3 with different data per item.  A case's reference is computed once
(reference()) and never written again."""
import os
import re
from collections import namedtuple

import numpy as np

import affine_ref as R

CHUNK = 1024                               # AFF_CHUNK of csrc/kernels_affine.hip
SIZES = (3, 4, 63, 64, 65, 1000, CHUNK + 1)
ITERS = (1, 63, 64, 65, 2000)
CONFIDENCES = (0.5, 0.99, 0.999)
TIE_SIZES = (3, 4, 5, 63, 64, 65, 257, 1000, 4097)
FLOW_FRAMES = ((66, 33), (131, 67))
TRUE_M = np.array([[1.02, -0.03, 4.5], [0.025, 0.98, -2.25]])

KERNELS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mav-detection_amd", "csrc", "kernels_affine.hip")
CAP_BATCH = 16                             # max_batch and batch of the calls whose score grid is capped
CAP_ITERS = (2049, 4096)                   # the first max_iters at which launch_affine_score's grid is capped at batch 16, and twice the cap


def source_constants(text=None) -> dict:
    """the constants of launch_affine_score as kernels_affine.hip defines them, read as text"""
    if text is None:
        with open(KERNELS) as f:
            text = f.read()
    out = {k: int(re.search(rf"^#define {k} (\d+)\b", text, re.M).group(1)) for k in ("AFF_THREADS", "AFF_CHUNK", "AFF_HYP_PER_WAVE", "AFF_GRID_CAP")}
    assert re.search(r"^#define AFF_WAVES \(AFF_THREADS / 64\)", text, re.M)
    out["AFF_WAVES"] = out["AFF_THREADS"] // 64
    out["text"] = text
    return out


def score_blocks(max_iters: int, B: int, c=None) -> tuple:
    """launch_affine_score: `per = ceil(max_iters / (AFF_WAVES * AFF_HYP_PER_WAVE)); cap = max(1, AFF_GRID_CAP / B)` -> (per, cap); the
    grid is min(per, cap) workgroups per item"""
    c = c or source_constants()
    g = c["AFF_WAVES"] * c["AFF_HYP_PER_WAVE"]
    return (max_iters + g - 1) // g, max(1, c["AFF_GRID_CAP"] // B)


def score_grid(max_iters: int, B: int, c=None) -> str:
    """"per-item": every workgroup has its AFF_WAVES * AFF_HYP_PER_WAVE hypotheses; "capped": fewer workgroups than that, a longer stride"""
    per, cap = score_blocks(max_iters, B, c)
    return "capped" if per > cap else "per-item"


# dev_only: the host form refuses the case (bad triples) or the case is stated for the _dev form (non-finite pairs)
Case = namedtuple("Case", "name src dst triples threshold confidence refine dev_only")


def triples_for(seed, n, max_iters, batch):
    """the draw of mavflow.affine.sample_triples, restated (tests/test_affine_ref_cpu.py holds the two equal)"""
    u = np.random.default_rng(seed).random(batch * max_iters * 3).reshape(batch, max_iters, 3)
    i0 = np.floor(u[..., 0] * n).astype(np.int64)
    i1 = np.floor(u[..., 1] * (n - 1)).astype(np.int64)
    i2 = np.floor(u[..., 2] * (n - 2)).astype(np.int64)
    i1 = i1 + (i1 >= i0)
    i2 = i2 + (i2 >= np.minimum(i0, i1))
    i2 = i2 + (i2 >= np.maximum(i0, i1))
    return np.stack([i0, i1, i2], -1).astype(np.int32)


def scene(n, seed, outliers=0.3, noise=0.0, patch=False, M=TRUE_M):
    """(src, dst, true inlier flags): points in a 640 x 480 frame under M; a share of gross outliers; with `patch`, the points of a 24 x 24
    patch move by their own vector (the MAV)"""
    rng = np.random.default_rng(seed)
    src = np.column_stack([rng.uniform(0, 640, n), rng.uniform(0, 480, n)])
    dst = src @ M[:, :2].T + M[:, 2]
    if noise:
        dst = dst + rng.normal(0, noise, dst.shape)
    good = np.ones(n, bool)
    if n >= 8 and outliers:
        bad = rng.permutation(n)[:int(n * outliers)]
        dst[bad] = np.column_stack([rng.uniform(0, 640, len(bad)), rng.uniform(0, 480, len(bad))])
        good[bad] = False
    if patch:
        inside = (np.abs(src[:, 0] - 320) < 12) & (np.abs(src[:, 1] - 240) < 12)
        dst[inside] += (9.0, -7.0)
        good[inside] = False
    return src, dst, good


def _batch(n, max_iters, B, seed, **kw):
    s = [scene(n, seed + 10 * b, M=TRUE_M + 0.01 * b, **kw) for b in range(B)]
    return np.stack([x[0] for x in s]), np.stack([x[1] for x in s]), triples_for(seed + 1, n, max_iters, B)


def _grid(n, shift=(5.0, 7.0)):
    """integer points of a grid, no three sampled ones forced collinear, under a pure integer translation: every error is exactly 0"""
    k = np.arange(n)
    src = np.column_stack([(k * 7) % 31, (k * 11) % 29 + k // 31]).astype(np.float64)
    return src, src + np.asarray(shift)


def _special():
    out = []
    n, mi = 65, 65
    # all-inlier data: the first valid hypothesis has count n and need[n] = 0 ends the loop
    src, dst = _grid(n)
    out.append(Case("all_inliers", src[None], dst[None], triples_for(5, n, mi, 1), 3.0, 0.99, 1, False))
    # no valid hypothesis: every point on one line
    line = np.column_stack([np.arange(n, dtype=np.float64), 2.0 * np.arange(n) + 1.0])
    out.append(Case("all_collinear", line[None], (line + 3.0)[None], triples_for(6, n, mi, 1), 3.0, 0.99, 1, False))
    # equal counts: two halves under two translations; hypotheses alternate between the halves, the first wins
    src, dst = _grid(64)
    dst = dst.copy()
    dst[32:] += (40.0, -30.0)
    t = triples_for(7, 32, 64, 1)
    t[0, 0::2] += 32                        # hypotheses 0, 2, ... sample the second half: the second half's model comes first
    out.append(Case("equal_counts", src[None], dst[None], t, 3.0, 0.5, 1, False))
    # exactly on the threshold: offset (3, 0) has error exactly 9.0 and is an inlier, (3, 1) has 10.0 and is none
    src, dst = _grid(n)
    dst = dst.copy()
    dst[10] += (3.0, 0.0)
    dst[11] += (3.0, 1.0)
    t = triples_for(8, n - 12, mi, 1) + 12  # samples avoid the two moved pairs
    out.append(Case("on_threshold", src[None], dst[None], t, 3.0, 0.99, 0, False))
    # threshold 0: exact integer data has error exactly 0
    src, dst = _grid(n)
    dst = dst.copy()
    dst[20] += (0.0, 1.0)
    out.append(Case("threshold_0", src[None], dst[None], triples_for(9, n, mi, 1), 0.0, 0.99, 1, False))
    # refinement on and off on the same noisy data
    for refine in (0, 1):
        src, dst, t = _batch(257, 130, 3, 40, noise=0.5)
        out.append(Case(f"noisy_refine{refine}", src, dst, t, 3.0, 0.99, refine, False))
    # refinement refused by the rank test: every inlier on the line y = 0 but one, 2^-17 above it; the triple (0, 1, 2) is a valid
    # right-angled sliver, the second-moment matrix has an eigenvalue ratio near 1e-17
    src = np.column_stack([np.arange(40) * 25.0, np.zeros(40)])
    src[2] = (0.0, 2.0 ** -17)
    t = np.array([[[0, 1, 2]] * 3], np.int32)
    out.append(Case("rank_refused", src[None], (src + (5.0, 7.0))[None], t, 3.0, 0.99, 1, False))
    # NaN, infinity and 1e300 in the pairs, sampled and unsampled (_dev form)
    src, dst, t = _batch(130, 130, 3, 50, noise=0.3)
    src, dst, t = src.copy(), dst.copy(), t.copy()
    src[0, 5, 0], dst[0, 6, 1], src[1, 7, 1], dst[1, 8, 0], src[2, 9, 0], dst[2, 10, 1] = np.nan, np.inf, -np.inf, 1e300, 1e300, np.nan
    src[2, 11], dst[2, 11] = (1e300, -1e300), (1e300, 1e300)
    for b, ks in enumerate(((5, 6), (7, 8), (9, 10, 11))):
        for j, k in enumerate(ks):
            t[b, 3 * j, j % 3] = k          # ... and some hypotheses sample them
            if len(set(t[b, 3 * j])) < 3:
                t[b, 3 * j] = (k, (k + 20) % 130, (k + 40) % 130)
    out.append(Case("non_finite", src, dst, t, 3.0, 0.99, 1, True))
    # out-of-range and repeated indices in the triples (_dev form): invalid hypotheses, nothing read through them
    src, dst, t = _batch(65, 65, 3, 60)
    t = t.copy()
    t[0, 0], t[0, 1], t[0, 2], t[0, 3] = (-1, 2, 3), (1, 65, 3), (1, 2, 2 ** 31 - 1), (-2 ** 31, 0, 1)
    t[1, 0], t[1, 1], t[1, 2] = (4, 4, 5), (4, 5, 4), (5, 4, 4)
    t[2, :, 0] = 10 ** 6                    # a whole item without a valid hypothesis
    out.append(Case("bad_triples", src, dst, t, 3.0, 0.99, 1, True))
    return out


def _table():
    out = []
    for n in SIZES:                         # every size at max_iters 65, batch 3
        src, dst, t = _batch(n, 65, 3, 100 + n, noise=0.2 if n >= 8 else 0.0)
        out.append(Case(f"n{n}_it65_b3", src, dst, t, 3.0, 0.99, 1, False))
    for mi in ITERS:                        # every max_iters at n = 1000, batch 1; 40 % outliers keep the loop running
        src, dst, t = _batch(1000, mi, 1, 200 + mi, noise=0.4, outliers=0.4)
        out.append(Case(f"n1000_it{mi}_b1", src, dst, t, 3.0, 0.99, 1, False))
    src, dst, t = _batch(CHUNK + 1, 2000, 1, 300, noise=0.4, outliers=0.5)
    out.append(Case(f"n{CHUNK + 1}_it2000_b1", src, dst, t, 2.0, 0.999, 1, False))
    return out + _special()


def late_winner(n, max_iters, B, seed, tail=6, **kw):
    """_batch's scenes with the triples rearranged: every hypothesis but the last `tail` samples gross outliers alone (few inliers, need[]
    stays above max_iters, the loop keeps running), the last `tail` sample true inliers alone -- the winner's count is one of the last the
    score kernel writes"""
    s = [scene(n, seed + 10 * b, M=TRUE_M + 0.01 * b, **kw) for b in range(B)]
    t = triples_for(seed + 2, n, max_iters, B)
    for b in range(B):
        bad_i, good_i = np.flatnonzero(~s[b][2]), np.flatnonzero(s[b][2])
        t[b, :max_iters - tail] = bad_i[triples_for(seed + 3 + b, len(bad_i), max_iters - tail, 1)[0]]
        t[b, max_iters - tail:] = good_i[triples_for(seed + 4 + b, len(good_i), tail, 1)[0]]
    return np.stack([x[0] for x in s]), np.stack([x[1] for x in s]), t


def _cap_table():
    """batch 16 on a context of max_batch 16, different data per item, 40 % outliers: the score grid is capped (score_grid).  The drawn
    triples at every (max_iters, n), and at two of them the same scenes with the winner among the last hypotheses"""
    out = []
    for mi in CAP_ITERS:
        for n in (65, CHUNK + 1):
            src, dst, t = _batch(n, mi, CAP_BATCH, 400 + n + mi, noise=0.4, outliers=0.4)
            out.append(Case(f"n{n}_it{mi}_b{CAP_BATCH}", src, dst, t, 3.0, 0.99, 1, False))
    for mi, n in ((CAP_ITERS[0], 65), (CAP_ITERS[1], CHUNK + 1)):
        src, dst, t = late_winner(n, mi, CAP_BATCH, 400 + n + mi, noise=0.4, outliers=0.4)
        out.append(Case(f"n{n}_it{mi}_b{CAP_BATCH}_late", src, dst, t, 3.0, 0.99, 1, False))
    return out


CASES = _table()
CAP_CASES = _cap_table()
BY_NAME = {c.name: c for c in CASES + CAP_CASES}
assert len(BY_NAME) == len(CASES) + len(CAP_CASES)
_refs = {}


def reference(name):
    """the restatement's result of a case: dict(M, inliers, records), computed once, read-only"""
    if name not in _refs:
        c = BY_NAME[name]
        out = R.estimate(c.src, c.dst, c.triples, c.threshold, c.confidence, bool(c.refine))
        for a in out.values():
            a.setflags(write=False)
        _refs[name] = out
    return _refs[name]


def flow_case(W, H, B, seed=70, n=48, max_iters=65):
    """float32 fields of an affine motion with noise and a moving patch; coords with the four corners and border points among them"""
    rng = np.random.default_rng(seed + W)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    flow = np.empty((B, H, W, 2), np.float32)
    for b in range(B):
        M = TRUE_M + 0.004 * b
        flow[b, ..., 0] = M[0, 0] * xs + M[0, 1] * ys + M[0, 2] - xs + rng.normal(0, 0.2, (H, W))
        flow[b, ..., 1] = M[1, 0] * xs + M[1, 1] * ys + M[1, 2] - ys + rng.normal(0, 0.2, (H, W))
        flow[b, H // 3:H // 3 + 8, W // 3:W // 3 + 8] += (6.0, -5.0)
    coords = np.column_stack([rng.integers(0, W, n), rng.integers(0, H, n)]).astype(np.int32)
    coords[:6] = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (W // 2, 0), (W - 1, H // 2)]
    return flow, coords, triples_for(seed + 1, n, max_iters, B)
