"""The cases of the robust essential-matrix fit (include/mavflow_essential.h), shared by tests/test_essential_ref_cpu.py (the restatement
against the definition) and tests/test_gpu_essential.py (the device against the restatement, byte for byte).  Shapes are the smallest at
which the kernels can go wrong: n at the minimum (5, 6), around the wavefront (63, 64, 65), the detector's 1000 and one LDS chunk + 1;
max_iters around the choice kernel's block of 64 slots (6, 7: ten slots per iteration), around 32 and 64 hypotheses (the models kernel's
workgroup, the wavefront) and the default 1000; batch 1 and 3 with different data per item.  Scenes have fundamental_cases.scene's
geometry, under the proper camera K_CAM and under the reference's literal camera (focal 1 / tan(pi / 4), pp (0, 0)) on pixel
coordinates.  A case's reference is computed once (reference()) and never written again."""
import os
import re
from collections import namedtuple

import numpy as np

import essential_ref as R
import fundamental_cases as FC

CHUNK = 1024                               # EM_CHUNK of csrc/kernels_essential.hip
SIZES = (5, 6, 63, 64, 65, 1000, CHUNK + 1)
ITERS = (1, 6, 7, 63, 64, 65, 1000)
FLOW_FRAMES = ((66, 33), (131, 67))
K_CAM = FC.K_CAM
CAM = (500.0, 500.0, 320.0, 240.0)         # K_CAM as (fx, fy, cx, cy)
LITERAL = (1.0 / np.tan(np.pi / 4), 1.0 / np.tan(np.pi / 4), 0.0, 0.0)     # the reference's focal_length, pp (0, 0)
STRONG = (FC.rotation(0.1, -0.15, 0.12), np.array([3.0, 0.5, 1.0]))          # a strong camera motion

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = os.path.join(ROOT, "mav-detection_amd", "csrc", "kernels_essential.hip")
INTERNAL = os.path.join(ROOT, "mav-detection_amd", "csrc", "mavflow_internal.h")
CAP_BATCH = 16                             # max_batch and batch of the calls whose score grid is capped
CAP_ITERS = 205                            # the first max_iters at which launch_em_score's grid is capped at batch 16


def source_constants(text=None) -> dict:
    """the constants of launch_em_score as kernels_essential.hip (and, EM_SLOTS, mavflow_internal.h) define them, read as text"""
    if text is None:
        with open(KERNELS) as f:
            text = f.read()
    out = {k: int(re.search(rf"^#define {k} (\d+)\b", text, re.M).group(1)) for k in ("EM_THREADS", "EM_CHUNK", "EM_SLOTS_PER_WAVE", "EM_GRID_CAP")}
    assert re.search(r"^#define EM_WAVES \(EM_THREADS / 64\)", text, re.M)
    out["EM_WAVES"] = out["EM_THREADS"] // 64
    with open(INTERNAL) as f:
        out["EM_SLOTS"] = int(re.search(r"^#define EM_SLOTS (\d+)\b", f.read(), re.M).group(1))
    out["text"] = text
    return out


def score_blocks(max_iters: int, B: int, c=None) -> tuple:
    """launch_em_score: `slots = EM_SLOTS * max_iters; per = ceil(slots / (EM_WAVES * EM_SLOTS_PER_WAVE)); cap = max(1, EM_GRID_CAP / B)`
    -> (per, cap); the grid is min(per, cap) workgroups per item"""
    c = c or source_constants()
    g = c["EM_WAVES"] * c["EM_SLOTS_PER_WAVE"]
    return (c["EM_SLOTS"] * max_iters + g - 1) // g, max(1, c["EM_GRID_CAP"] // B)


def score_grid(max_iters: int, B: int, c=None) -> str:
    """"per-item": every workgroup has its EM_WAVES * EM_SLOTS_PER_WAVE slots; "capped": fewer workgroups than that, a longer stride"""
    per, cap = score_blocks(max_iters, B, c)
    return "capped" if per > cap else "per-item"


# dev_only: the host form refuses the case (bad subsets) or the case is stated for the _dev form (non-finite pairs)
Case = namedtuple("Case", "name src dst subsets threshold confidence camera dev_only")


def subsets_for(seed, n, max_iters, batch):
    """the draw of mavflow.essential.sample_subsets, restated (tests/test_essential_ref_cpu.py holds the two equal)"""
    u = np.random.default_rng(seed).random(batch * max_iters * 5).reshape(batch, max_iters, 5)
    out = np.empty((batch, max_iters, 5), np.int64)
    for b in range(batch):
        for it in range(max_iters):
            picks = []
            for j in range(5):
                i = int(np.floor(u[b, it, j] * (n - j)))
                for p in sorted(picks):
                    if i >= p:
                        i += 1
                picks.append(i)
            out[b, it] = picks
    return out.astype(np.int32)


def true_E(Rm, t):
    """[t]x R of unit Frobenius norm"""
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    E = tx @ Rm
    return E / np.sqrt((E * E).sum())


def scene(n, seed, outliers=0.3, noise=0.0, k=0, motion=None, K=K_CAM):
    """fundamental_cases.scene's geometry under camera K and (optionally) another motion: (src, dst, true inlier flags, (R, t))"""
    rng = np.random.default_rng(seed)
    Rm, t = FC.pose(k) if motion is None else motion
    src = np.column_stack([rng.uniform(0, 640, n), rng.uniform(0, 480, n)])
    depth = rng.uniform(4.0, 20.0, n)
    P = (np.linalg.inv(K) @ np.column_stack([src, np.ones(n)]).T) * depth
    Q = K @ (Rm @ P + np.asarray(t, np.float64)[:, None])
    dst = (Q[:2] / Q[2]).T
    if noise:
        dst = dst + rng.normal(0, noise, dst.shape)
    good = np.ones(n, bool)
    if n >= 8 and outliers:
        bad = rng.permutation(n)[:int(n * outliers)]
        dst[bad] = np.column_stack([rng.uniform(0, 640, len(bad)), rng.uniform(0, 480, len(bad))])
        good[bad] = False
    return src, dst, good, (Rm, t)


def planar_scene(seed, nplane=56, noff=12, nout=12):
    """(src, dst) under the strong motion: `nplane` points of one plane first, then `noff` points off it, then `nout` gross outliers"""
    n = nplane + noff + nout
    rng = np.random.default_rng(seed)
    Rm, t = STRONG
    src = np.column_stack([rng.uniform(0, 640, n), rng.uniform(0, 480, n)])
    rays = np.linalg.inv(K_CAM) @ np.column_stack([src, np.ones(n)]).T
    depth = 9.0 / (np.array([0.2, -0.1, 1.0]) @ rays)
    depth[nplane:] = rng.uniform(4.0, 20.0, n - nplane)
    Q = K_CAM @ (Rm @ (rays * depth) + t[:, None])
    dst = (Q[:2] / Q[2]).T
    dst[nplane + noff:] = np.column_stack([rng.uniform(0, 640, nout), rng.uniform(0, 480, nout)])
    return src, dst


K_LITERAL = np.array([[LITERAL[0], 0.0, 0.0], [0.0, LITERAL[1], 0.0], [0.0, 0.0, 1.0]])


def _batch(n, max_iters, B, seed, **kw):
    s = [scene(n, seed + 10 * b, k=b, **kw) for b in range(B)]
    return np.stack([x[0] for x in s]), np.stack([x[1] for x in s]), subsets_for(seed + 1, n, max_iters, B)


def _special():
    out = []
    n, mi = 65, 65
    # all-inlier data under a strong motion: a slot of iteration 0 has count n, need[n] = 0 ends the loop, all ten slots are still visited
    src, dst, _, _ = scene(n, 5, outliers=0, motion=STRONG)
    out.append(Case("all_inliers", src[None], dst[None], subsets_for(5, n, mi, 1), 1.0, 0.999, CAM, False))
    # no valid hypothesis: every pair is (1, 1) -> (1, 1) under the default camera: the system's rows are all ones, the second
    # elimination step finds exact zeros only
    pts = np.ones((1, n, 2))
    out.append(Case("no_valid", pts, pts.copy(), subsets_for(6, n, mi, 1), 1.0, 0.999, R.CAMERA, False))
    # equal counts: every odd hypothesis repeats the even one before it; the first wins
    src, dst, _, _ = scene(64, 7, outliers=0.4)
    t = subsets_for(7, 64, 64, 1)
    t[0, 1::2] = t[0, 0::2]
    out.append(Case("equal_counts", src[None], dst[None], t, 1.0, 0.5, CAM, False))
    # either side of the threshold: two pairs moved off their epipolar lines along the normal by 1 and 2 pixels (a Sampson error of about
    # half the squared displacement: 0.5 and 2 against 1); no sample has them
    src, dst, _, (Rm, tt) = scene(n, 8, outliers=0, motion=STRONG)
    Ft = FC.true_F(K_CAM, Rm, tt)
    dst = dst.copy()
    for kk, d in ((10, 1.0), (11, 2.0)):
        l = Ft @ np.array([src[kk, 0], src[kk, 1], 1.0])
        dst[kk] += d * l[:2] / np.hypot(l[0], l[1])
    t = subsets_for(8, n - 12, mi, 1) + 12
    out.append(Case("beside_threshold", src[None], dst[None], t, 1.0, 0.999, CAM, False))
    # threshold 0: only an error of exactly 0 counts
    src, dst, _, _ = scene(n, 9, outliers=0)
    out.append(Case("threshold_0", src[None], dst[None], subsets_for(9, n, mi, 1), 0.0, 0.999, CAM, False))
    # NaN, infinity and 1e300 in the pairs, sampled and unsampled (_dev form)
    src, dst, t = _batch(130, 66, 3, 50, noise=0.1)
    src, dst, t = src.copy(), dst.copy(), t.copy()
    src[0, 5, 0], dst[0, 6, 1], src[1, 7, 1], dst[1, 8, 0], src[2, 9, 0], dst[2, 10, 1] = np.nan, np.inf, -np.inf, 1e300, 1e300, np.nan
    src[2, 11], dst[2, 11] = (1e300, -1e300), (1e300, 1e300)
    for b, ks in enumerate(((5, 6), (7, 8), (9, 10, 11))):
        for j, kk in enumerate(ks):
            t[b, 3 * j] = [(kk + 17 * q) % 130 for q in range(5)]      # ... and some hypotheses sample them
    out.append(Case("non_finite", src, dst, t, 1.0, 0.999, CAM, True))
    # out-of-range and repeated indices in the subsets (_dev form): invalid hypotheses, nothing read through them
    src, dst, t = _batch(65, 65, 3, 60)
    t = t.copy()
    t[0, 0, 0], t[0, 1, 4], t[0, 2, 3], t[0, 3, 2] = -1, 65, 2 ** 31 - 1, -2 ** 31
    t[1, 0, 1], t[1, 1, 4], t[1, 2, 3] = t[1, 0, 0], t[1, 1, 0], t[1, 2, 2]
    t[2, :, 4] = 10 ** 6                    # a whole item without a valid subset
    out.append(Case("bad_subsets", src, dst, t, 1.0, 0.999, CAM, True))
    # the choice across the 64-slot block boundary: iterations 0 .. 5 sample gross outliers only (counts far below any cut of niters);
    # iteration 6 (slots 60 .. 69) samples five points of a PLANE, for which a second essential matrix fits every point of the plane:
    # its slot 61 holds the plane's 56 pairs, need[56] = 4 cuts niters below the running iteration, and slot 64 -- in the next block --
    # holds all 68 true pairs and must still win; iteration 7 must not begin
    src, dst = planar_scene(0)
    t = np.array([[68 + (i + 2 * q) % 12 for q in range(5)] for i in range(6)] + [[41, 14, 27, 26, 55], [10, 3, 15, 46, 51]], np.int32)
    out.append(Case("across_blocks", src[None], dst[None], t[None], 1.0, 0.5, CAM, False))
    # a pure rotation (t = 0): every E = [t]x R fits; whatever the restatement returns, the device returns the same bytes
    src, dst, _, _ = scene(n, 11, outliers=0.2, noise=0.1, motion=(FC.rotation(0.02, -0.03, 0.01), np.zeros(3)))
    out.append(Case("pure_rotation", src[None], dst[None], subsets_for(11, n, mi, 1), 1.0, 0.999, CAM, False))
    return out


def _table():
    out = []
    for n in SIZES:                         # every size at max_iters 65, batch 3
        src, dst, t = _batch(n, 65, 3, 100 + n, noise=0.2 if n >= 8 else 0.0)
        out.append(Case(f"n{n}_it65_b3", src, dst, t, 1.0, 0.999, CAM, False))
    for mi in ITERS:                        # every max_iters at n = 1000, batch 1; 40 % outliers keep the loop running
        src, dst, t = _batch(1000, mi, 1, 200 + mi, noise=0.4, outliers=0.4)
        out.append(Case(f"n1000_it{mi}_b1", src, dst, t, 1.0, 0.999, CAM, False))
    src, dst, t = _batch(CHUNK + 1, 200, 1, 300, noise=0.4, outliers=0.5, motion=STRONG)
    out.append(Case(f"n{CHUNK + 1}_it200_b1", src, dst, t, 2.0, 0.99, CAM, False))
    # the reference's literal camera on pixel coordinates: the scene is one of a camera with that focal length, seen in "pixels" of size 1
    src, dst, t = _batch(200, 33, 3, 400, noise=0.0, outliers=0.3, motion=STRONG, K=K_LITERAL)
    out.append(Case("literal_n200_it33_b3", src, dst, t, 1.0, 0.999, LITERAL, False))
    return out + _special()


def late_winner(n, max_iters, B, seed, tail=6, **kw):
    """_batch's scenes with the subsets rearranged: every hypothesis but the last `tail` samples gross outliers alone (few inliers, need[]
    stays above max_iters, the loop keeps running), the last `tail` sample true inliers alone -- the winner's count is one of the last the
    score kernel writes"""
    s = [scene(n, seed + 10 * b, k=b, **kw) for b in range(B)]
    t = subsets_for(seed + 2, n, max_iters, B)
    for b in range(B):
        bad_i, good_i = np.flatnonzero(~s[b][2]), np.flatnonzero(s[b][2])
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
        out.append(Case(f"n{n}_it{CAP_ITERS}_b{CAP_BATCH}", src, dst, t, 1.0, 0.999, CAM, False))
        if n == CHUNK + 1:
            src, dst, t = late_winner(n, CAP_ITERS, CAP_BATCH, 400 + n, noise=0.4, outliers=0.4)
            out.append(Case(f"n{n}_it{CAP_ITERS}_b{CAP_BATCH}_late", src, dst, t, 1.0, 0.999, CAM, False))
    return out


CASES = _table()
CAP_CASES = _cap_table()
BY_NAME = {c.name: c for c in CASES + CAP_CASES}
assert len(BY_NAME) == len(CASES) + len(CAP_CASES)
_refs = {}


def reference(name):
    """the restatement's result of a case: dict(E, F, inliers, records), computed once, read-only"""
    if name not in _refs:
        c = BY_NAME[name]
        out = R.find(c.src, c.dst, c.subsets, c.threshold, c.confidence, c.camera)
        for a in out.values():
            a.setflags(write=False)
        _refs[name] = out
    return _refs[name]


def flow_case(W, H, B, seed=70, n=96, max_iters=130):
    """fundamental_cases.flow_case's fields and coords, with subsets of five; the camera is dense_scene's"""
    flow, coords, _ = FC.flow_case(W, H, B, seed, n, max_iters)
    return flow, coords, subsets_for(seed + 1, n, max_iters, B), (100.0, 100.0, (W - 1) / 2, (H - 1) / 2)
