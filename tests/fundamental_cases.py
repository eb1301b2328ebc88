"""The cases of the robust fundamental-matrix fit and the dense epipolar residual (include/mavflow_fundamental.h), shared by
tests/test_fundamental_ref_cpu.py (the restatement against the definition) and tests/test_gpu_fundamental.py (the device against the
restatement, byte for byte).  Shapes are the smallest at which the kernels can go wrong: n at the minimum (7, 8), around the wavefront
(63, 64, 65), the detector's 1000 and one LDS chunk + 1; max_iters around the choice kernel's block of 64 slots (21, 22: three slots per
iteration), around 64 iterations and the default 1000; batch 1 and 3 with different data per item.  A case's reference is computed once
(reference()) and never written again."""
import os
import re
from collections import namedtuple

import numpy as np

import fundamental_ref as R

CHUNK = 1024                               # FM_CHUNK of csrc/kernels_fundamental.hip
SIZES = (7, 8, 63, 64, 65, 1000, CHUNK + 1)
ITERS = (1, 21, 22, 63, 64, 65, 1000)
CONFIDENCES = (0.5, 0.99, 0.999)
TIE_SIZES = (7, 8, 63, 64, 65, 257, 1000, 1025)
FLOW_FRAMES = ((66, 33), (131, 67))
K_CAM = np.array([[500.0, 0.0, 320.0], [0.0, 500.0, 240.0], [0.0, 0.0, 1.0]])

KERNELS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mav-detection_amd", "csrc", "kernels_fundamental.hip")
CAP_BATCH = 16                             # max_batch and batch of the calls whose score grid is capped
CAP_ITERS = 683                            # the first max_iters at which launch_fm_score's grid is capped at batch 16
EPI_FRAME, EPI_BATCH = (397, 331), 2       # the dense pass past its cap: 131 407 px = 512 * 256 + 335


def source_constants(text=None) -> dict:
    """the constants of launch_fm_score and launch_epipolar_residual as kernels_fundamental.hip defines them, read as text"""
    if text is None:
        with open(KERNELS) as f:
            text = f.read()
    out = {k: int(re.search(rf"^#define {k} (\d+)\b", text, re.M).group(1)) for k in ("FM_THREADS", "FM_CHUNK", "FM_SLOTS_PER_WAVE", "FM_GRID_CAP", "EPI_WG", "EPI_CAP")}
    assert re.search(r"^#define FM_WAVES \(FM_THREADS / 64\)", text, re.M)
    out["FM_WAVES"] = out["FM_THREADS"] // 64
    out["text"] = text
    return out


def score_blocks(max_iters: int, B: int, c=None) -> tuple:
    """launch_fm_score: `slots = 3 * max_iters; per = ceil(slots / (FM_WAVES * FM_SLOTS_PER_WAVE)); cap = max(1, FM_GRID_CAP / B)`
    -> (per, cap); the grid is min(per, cap) workgroups per item"""
    c = c or source_constants()
    g = c["FM_WAVES"] * c["FM_SLOTS_PER_WAVE"]
    return (3 * max_iters + g - 1) // g, max(1, c["FM_GRID_CAP"] // B)


def score_grid(max_iters: int, B: int, c=None) -> str:
    """"per-item": every workgroup has its FM_WAVES * FM_SLOTS_PER_WAVE slots; "capped": fewer workgroups than that, a longer stride"""
    per, cap = score_blocks(max_iters, B, c)
    return "capped" if per > cap else "per-item"


def epi_stride_forms(n0: int, c=None) -> set:
    """k_epipolar_residual's `for (p = blockIdx.x * EPI_WG + threadIdx.x; p < n0; p += gridDim.x * EPI_WG)` under at most EPI_CAP workgroups"""
    c = c or source_constants()
    need = (n0 + c["EPI_WG"] - 1) // c["EPI_WG"]
    T = ((need if need else 1) if need < c["EPI_CAP"] else c["EPI_CAP"]) * c["EPI_WG"]
    trips = (n0 + T - 1) // T
    if trips <= 1:
        return {"1"}
    return {">1"} | ({">1:partial-last"} if n0 % T else set())


# dev_only: the host form refuses the case (bad subsets) or the case is stated for the _dev form (non-finite pairs)
Case = namedtuple("Case", "name src dst subsets threshold confidence dev_only")


def subsets_for(seed, n, max_iters, batch):
    """the draw of mavflow.fundamental.sample_subsets, restated (tests/test_fundamental_ref_cpu.py holds the two equal)"""
    u = np.random.default_rng(seed).random(batch * max_iters * 7).reshape(batch, max_iters, 7)
    out = np.empty((batch, max_iters, 7), np.int64)
    for b in range(batch):
        for it in range(max_iters):
            picks = []
            for j in range(7):
                i = int(np.floor(u[b, it, j] * (n - j)))
                for p in sorted(picks):
                    if i >= p:
                        i += 1
                picks.append(i)
            out[b, it] = picks
    return out.astype(np.int32)


def rotation(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def true_F(K, Rm, t):
    """K^-T [t]x R K^-1 of unit Frobenius norm"""
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    Ki = np.linalg.inv(K)
    Fm = Ki.T @ tx @ Rm @ Ki
    return Fm / np.sqrt((Fm * Fm).sum())


def pose(k=0):
    """a small rotation and a translation with a forward component; k varies it per item"""
    return rotation(0.010 + 0.002 * k, -0.020, 0.015 - 0.003 * k), np.array([0.30 + 0.05 * k, 0.05, 0.20])


def scene(n, seed, outliers=0.3, noise=0.0, k=0):
    """(src, dst, true inlier flags, true F): 3-D points of spread depth seen by a camera that turns a little and moves sideways and
    forward; a share of gross outliers (n >= 8)"""
    rng = np.random.default_rng(seed)
    Rm, t = pose(k)
    src = np.column_stack([rng.uniform(0, 640, n), rng.uniform(0, 480, n)])
    depth = rng.uniform(4.0, 20.0, n)
    P = (np.linalg.inv(K_CAM) @ np.column_stack([src, np.ones(n)]).T) * depth
    Q = K_CAM @ (Rm @ P + t[:, None])
    dst = (Q[:2] / Q[2]).T
    if noise:
        dst = dst + rng.normal(0, noise, dst.shape)
    good = np.ones(n, bool)
    if n >= 8 and outliers:
        bad = rng.permutation(n)[:int(n * outliers)]
        dst[bad] = np.column_stack([rng.uniform(0, 640, len(bad)), rng.uniform(0, 480, len(bad))])
        good[bad] = False
    return src, dst, good, true_F(K_CAM, Rm, t)


def _batch(n, max_iters, B, seed, **kw):
    s = [scene(n, seed + 10 * b, k=b, **kw) for b in range(B)]
    return np.stack([x[0] for x in s]), np.stack([x[1] for x in s]), subsets_for(seed + 1, n, max_iters, B)


def _special():
    out = []
    n, mi = 65, 65
    # all-inlier data: the first valid slot has count n, need[n] = 0 ends the loop, the iteration's later slots are still visited
    src, dst, _, _ = scene(n, 5, outliers=0)
    out.append(Case("all_inliers", src[None], dst[None], subsets_for(5, n, mi, 1), 3.0, 0.99, False))
    # no valid hypothesis: dst == src on small integers times powers of two makes three pairs of columns of the system equal; a pivot
    # taken in one of a pair leaves the other exactly zero, and the seventh step finds nothing but exact zeros
    k = np.arange(n)
    pts = np.column_stack([((k * 7) % 31) * 2.0 ** (k % 3), ((k * 11) % 29 + k // 31) * 2.0 ** (k % 2)])
    out.append(Case("no_valid", pts[None], pts[None].copy(), subsets_for(6, n, mi, 1), 3.0, 0.99, False))
    # equal counts: every odd hypothesis repeats the even one before it; the first wins
    src, dst, _, _ = scene(64, 7, outliers=0.4)
    t = subsets_for(7, 64, 64, 1)
    t[0, 1::2] = t[0, 0::2]
    out.append(Case("equal_counts", src[None], dst[None], t, 3.0, 0.5, False))
    # either side of the threshold: two pairs moved off their epipolar lines along the normal by 2.5 and 3.5 pixels; no sample has them
    src, dst, _, Ft = scene(n, 8, outliers=0)
    dst = dst.copy()
    for kk, d in ((10, 2.5), (11, 3.5)):
        l = Ft @ np.array([src[kk, 0], src[kk, 1], 1.0])
        dst[kk] += d * l[:2] / np.hypot(l[0], l[1])
    t = subsets_for(8, n - 12, mi, 1) + 12
    out.append(Case("beside_threshold", src[None], dst[None], t, 3.0, 0.99, False))
    # threshold 0: only an error of exactly 0 counts
    src, dst, _, _ = scene(n, 9, outliers=0)
    out.append(Case("threshold_0", src[None], dst[None], subsets_for(9, n, mi, 1), 0.0, 0.99, False))
    # NaN, infinity and 1e300 in the pairs, sampled and unsampled (_dev form)
    src, dst, t = _batch(130, 66, 3, 50, noise=0.1)
    src, dst, t = src.copy(), dst.copy(), t.copy()
    src[0, 5, 0], dst[0, 6, 1], src[1, 7, 1], dst[1, 8, 0], src[2, 9, 0], dst[2, 10, 1] = np.nan, np.inf, -np.inf, 1e300, 1e300, np.nan
    src[2, 11], dst[2, 11] = (1e300, -1e300), (1e300, 1e300)
    for b, ks in enumerate(((5, 6), (7, 8), (9, 10, 11))):
        for j, kk in enumerate(ks):
            t[b, 3 * j] = [(kk + 17 * q) % 130 for q in range(7)]      # ... and some hypotheses sample them
    out.append(Case("non_finite", src, dst, t, 3.0, 0.99, True))
    # out-of-range and repeated indices in the subsets (_dev form): invalid hypotheses, nothing read through them
    src, dst, t = _batch(65, 65, 3, 60)
    t = t.copy()
    t[0, 0, 0], t[0, 1, 6], t[0, 2, 3], t[0, 3, 2] = -1, 65, 2 ** 31 - 1, -2 ** 31
    t[1, 0, 1], t[1, 1, 6], t[1, 2, 5] = t[1, 0, 0], t[1, 1, 0], t[1, 2, 4]
    t[2, :, 4] = 10 ** 6                    # a whole item without a valid subset
    out.append(Case("bad_subsets", src, dst, t, 3.0, 0.99, True))
    return out


def _table():
    out = []
    for n in SIZES:                         # every size at max_iters 65, batch 3
        src, dst, t = _batch(n, 65, 3, 100 + n, noise=0.2 if n >= 8 else 0.0)
        out.append(Case(f"n{n}_it65_b3", src, dst, t, 3.0, 0.99, False))
    for mi in ITERS:                        # every max_iters at n = 1000, batch 1; 40 % outliers keep the loop running
        src, dst, t = _batch(1000, mi, 1, 200 + mi, noise=0.4, outliers=0.4)
        out.append(Case(f"n1000_it{mi}_b1", src, dst, t, 3.0, 0.99, False))
    src, dst, t = _batch(CHUNK + 1, 200, 1, 300, noise=0.4, outliers=0.5)
    out.append(Case(f"n{CHUNK + 1}_it200_b1", src, dst, t, 2.0, 0.999, False))
    return out + _special()


def late_winner(n, max_iters, B, seed, tail=6, **kw):
    """_batch's scenes with the subsets rearranged: every hypothesis but the last `tail` samples gross outliers alone (few inliers, need[]
    stays above max_iters, the loop keeps running), the last `tail` sample true inliers alone -- the winner's count is one of the last the
    score kernel writes"""
    s = [scene(n, seed + 10 * b, k=b, **kw) for b in range(B)]
    t = subsets_for(seed + 2, n, max_iters, B)
    for b in range(B):
        good = s[b][2]
        bad_i, good_i = np.flatnonzero(~good), np.flatnonzero(good)
        t[b, :max_iters - tail] = bad_i[subsets_for(seed + 3 + b, len(bad_i), max_iters - tail, 1)[0]]
        t[b, max_iters - tail:] = good_i[subsets_for(seed + 4 + b, len(good_i), tail, 1)[0]]
    return np.stack([x[0] for x in s]), np.stack([x[1] for x in s]), t


def _cap_table():
    """batch 16 on a context of max_batch 16, different data per item, 40 % outliers: the score grid is capped (score_grid).  Per n the
    drawn subsets, and at n = CHUNK + 1 (a count added to across two chunks) the same scenes with the winner among the last
    hypotheses"""
    out = []
    for n in (65, CHUNK + 1):
        src, dst, t = _batch(n, CAP_ITERS, CAP_BATCH, 400 + n, noise=0.4, outliers=0.4)
        out.append(Case(f"n{n}_it{CAP_ITERS}_b{CAP_BATCH}", src, dst, t, 3.0, 0.99, False))
        if n == CHUNK + 1:
            src, dst, t = late_winner(n, CAP_ITERS, CAP_BATCH, 400 + n, noise=0.4, outliers=0.4)
            out.append(Case(f"n{n}_it{CAP_ITERS}_b{CAP_BATCH}_late", src, dst, t, 3.0, 0.99, False))
    return out


CASES = _table()
CAP_CASES = _cap_table()
BY_NAME = {c.name: c for c in CASES + CAP_CASES}
assert len(BY_NAME) == len(CASES) + len(CAP_CASES)
_refs = {}


def reference(name):
    """the restatement's result of a case: dict(F, inliers, records), computed once, read-only"""
    if name not in _refs:
        c = BY_NAME[name]
        out = R.find(c.src, c.dst, c.subsets, c.threshold, c.confidence)
        for a in out.values():
            a.setflags(write=False)
        _refs[name] = out
    return _refs[name]


PATCH = 8


def dense_scene(W, H, B, seed=70, noise=0.05):
    """float32 flow fields (B, H, W, 2) of a static scene with smoothly varying depth under a small camera motion, float32 noise of
    sigma `noise`, and (where the frame has room) an 8 x 8 patch that moves on its own; returns (flow, (row, col) of the patch or None)"""
    rng = np.random.default_rng(seed + W)
    K = np.array([[100.0, 0.0, (W - 1) / 2], [0.0, 100.0, (H - 1) / 2], [0.0, 0.0, 1.0]])
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    flow = np.empty((B, H, W, 2), np.float32)
    at = (H // 3, W // 3) if W >= 3 * PATCH and H >= 3 * PATCH else None
    for b in range(B):
        Rm, t = pose(b)
        depth = 6.0 + 2.0 * np.sin(xs / 9.0 + b) + 1.5 * np.cos(ys / 7.0)
        P = (np.linalg.inv(K) @ np.stack([xs.ravel(), ys.ravel(), np.ones(W * H)])) * depth.ravel()
        Q = K @ (Rm @ P + 0.5 * t[:, None])
        flow[b, ..., 0] = (Q[0] / Q[2]).reshape(H, W) - xs + rng.normal(0, noise, (H, W))
        flow[b, ..., 1] = (Q[1] / Q[2]).reshape(H, W) - ys + rng.normal(0, noise, (H, W))
        if at:
            flow[b, at[0]:at[0] + PATCH, at[1]:at[1] + PATCH] += np.float32((-2.0, 5.0))
    return flow, at


def flow_case(W, H, B, seed=70, n=96, max_iters=130):
    """dense_scene's fields; coords with the four corners and border points among them, none in the patch"""
    flow, at = dense_scene(W, H, B, seed)
    rng = np.random.default_rng(seed + W + 1)
    coords = np.column_stack([rng.integers(0, W, 4 * n), rng.integers(0, H, 4 * n)]).astype(np.int32)
    if at:
        inside = (coords[:, 1] >= at[0]) & (coords[:, 1] < at[0] + PATCH) & (coords[:, 0] >= at[1]) & (coords[:, 0] < at[1] + PATCH)
        coords = coords[~inside]
    coords = np.ascontiguousarray(coords[:n])
    coords[:6] = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (W // 2, 0), (W - 1, H // 2)]
    return flow, coords, subsets_for(seed + 1, n, max_iters, B)


# ---- the dense pass past its cap -------------------------------------------------------------------------------------------------------------
def epi_cap_inputs(kind):
    """(flow (EPI_BATCH, H, W, 2) float32, F (EPI_BATCH, 3, 3), threshold) at EPI_FRAME.  "noise": noise fields with NaN and infinite vectors
    planted either side of pixel EPI_CAP * EPI_WG, item 1 with one long vector past it (its unique maximum); "zero_F": the zero matrix"""
    w, h = EPI_FRAME
    c = source_constants()
    thr = c["EPI_CAP"] * c["EPI_WG"]
    flow = np.random.default_rng(77).normal(0, 1.5, (EPI_BATCH, h, w, 2)).astype(np.float32)
    K = np.array([[100.0, 0, (w - 1) / 2], [0, 100.0, (h - 1) / 2], [0, 0, 1]])
    Fm = np.stack([true_F(K, *pose(b)) for b in range(EPI_BATCH)])
    flat = flow.reshape(EPI_BATCH, w * h, 2)
    for b in range(EPI_BATCH):
        for p, v in ((3 + b, (np.nan, 0)), (thr - 300, (0, np.inf)), (thr - 1, (np.nan, np.nan)), (thr, (-np.inf, 1)), (thr + 257 + b, (1, np.nan)), (w * h - 1, (np.inf, np.inf))):
            flat[b, p] = v
    flat[1, thr + 200] = (300.0, -400.0)
    if kind == "zero_F":
        Fm = np.zeros_like(Fm)
    return flow, Fm, 6.0                                     # leaves movers and still pixels on both sides (the residuals grow towards the last row)


_epi_refs = {}


def epi_cap_reference(kind):
    """(flow, F, threshold, the restatement's dict), computed once, read-only"""
    if kind not in _epi_refs:
        flow, Fm, t = epi_cap_inputs(kind)
        want = R.epipolar_residual(flow, Fm, t)
        for a in (flow, Fm) + tuple(want.values()):
            a.setflags(write=False)
        _epi_refs[kind] = (flow, Fm, t, want)
    return _epi_refs[kind]
