"""include/mavflow_fundamental.h in numpy and plain Python floats, in the header's order: every operation float64 and rounded on its own
(neither numpy nor Python fuses anything), sums in plain index order.  The device must equal this byte for byte; this file is held to the
definition by tests/test_fundamental_ref_cpu.py.  Nothing here is pinned against cv2."""
import math

import numpy as np

MAX_PAIRS, MAX_ITERS = 65536, 4096
RECORD_DTYPE = np.dtype([("ok", np.int32), ("inliers", np.int32), ("best_iter", np.int32), ("best_slot", np.int32), ("iters_run", np.int32),
                         ("valid", np.int32), ("sq_error", np.float64)])
EPI_DTYPE = np.dtype([("max_residual", np.float32), ("max_row", np.int32), ("max_col", np.int32), ("movers", np.int32),
                      ("not_finite", np.int32), ("pad", np.int32, (3,))])
assert RECORD_DTYPE.itemsize == 32 and EPI_DTYPE.itemsize == 32
F64 = np.float64
DBL_MIN = np.finfo(np.float64).tiny
INF = float("inf")


def need_quotient(n: int, g: int, confidence: float):
    """(ln, ld) of need[g], or None where no quotient is taken (g < 7, or den < DBL_MIN)"""
    if g < 7:
        return None
    w = g / n
    w2 = w * w
    w4 = w2 * w2
    den = 1.0 - (w4 * w2) * w
    if den < DBL_MIN:
        return None
    return math.log(1.0 - confidence), math.log(den)


def need_table(n: int, confidence: float, max_iters: int) -> np.ndarray:
    """need[g], g = 0 .. n: RANSACUpdateNumIters(confidence, (n - g) / n, 7, max_iters)"""
    need = np.empty(n + 1, np.int32)
    for g in range(n + 1):
        if g < 7:
            need[g] = max_iters
            continue
        q = need_quotient(n, g, confidence)
        if q is None:
            need[g] = 0
            continue
        ln, ld = q
        need[g] = max_iters if (ld >= 0.0 or -ln >= max_iters * (-ld)) else int(np.rint(ln / ld))
    return need


def _finite(v) -> bool:
    return v - v == 0.0


def _div(a, b):
    """IEEE division of Python floats (Python raises where IEEE gives an infinity or a NaN)"""
    with np.errstate(all="ignore"):
        return float(F64(a) / F64(b))


def det3(m):
    return (m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6])) + m[2] * (m[3] * m[7] - m[4] * m[6])


def null_vectors(src, dst, subset):
    """steps 1 - 4: (f1, f2) as lists of nine floats, or None for an invalid hypothesis"""
    n = len(src)
    idx = [int(v) for v in subset]
    if any(i < 0 or i >= n for i in idx) or len(set(idx)) != 7:
        return None
    A = []
    for i in idx:
        x, y, X, Y = float(src[i][0]), float(src[i][1]), float(dst[i][0]), float(dst[i][1])
        A.append([X * x, X * y, X, Y * x, Y * y, Y, x, y, 1.0])
    perm = list(range(9))
    for k in range(7):
        pv, pr, pc = 0.0, k, k
        for r in range(k, 7):
            for c in range(k, 9):
                v = abs(A[r][c])
                if v > pv:
                    pv, pr, pc = v, r, c
        if not (pv > 0.0 and _finite(pv)):
            return None
        A[k], A[pr] = A[pr], A[k]
        for r in range(7):
            A[r][k], A[r][pc] = A[r][pc], A[r][k]
        perm[k], perm[pc] = perm[pc], perm[k]
        p = A[k][k]
        for c in range(k + 1, 9):
            A[k][c] = A[k][c] / p
        for r in range(7):
            if r == k:
                continue
            m = A[r][k]
            for c in range(k + 1, 9):
                A[r][c] = A[r][c] - m * A[k][c]
    f1, f2 = [0.0] * 9, [0.0] * 9
    for i in range(7):
        f1[perm[i]] = -A[i][7]
        f2[perm[i]] = -A[i][8]
    f1[perm[7]] = 1.0
    f2[perm[8]] = 1.0
    return f1, f2


def cubic(f1, f2):
    """step 5: (c3, c2, c1, c0)"""
    def swapped(a, b, i):
        m = list(a)
        m[3 * i:3 * i + 3] = b[3 * i:3 * i + 3]
        return m
    c3, c0 = det3(f1), det3(f2)
    c2 = (det3(swapped(f1, f2, 0)) + det3(swapped(f1, f2, 1))) + det3(swapped(f1, f2, 2))
    c1 = (det3(swapped(f2, f1, 0)) + det3(swapped(f2, f1, 1))) + det3(swapped(f2, f1, 2))
    return c3, c2, c1, c0


def real_roots(c3, c2, c1, c0):
    """step 6: the real roots in ascending order (at most three); [] where there is no model"""
    if c3 == 0.0 or not (_finite(c3) and _finite(c2) and _finite(c1) and _finite(c0)):
        return []
    q2, q1, q0 = abs(_div(c2, c3)), abs(_div(c1, c3)), abs(_div(c0, c3))
    mx = q2
    mx = q1 if q1 > mx else mx
    mx = q0 if q0 > mx else mx
    R = 1.0 + mx
    if not _finite(R):
        return []

    def horner(l):
        with np.errstate(all="ignore"):
            return float(((F64(c3) * F64(l) + F64(c2)) * F64(l) + F64(c1)) * F64(l) + F64(c0))
    with np.errstate(all="ignore"):
        disc = float(F64(c2) * F64(c2) - (F64(3.0) * F64(c3)) * F64(c1))
    e = [-R, R]
    if disc > 0.0:
        q = math.sqrt(disc)
        u, v = _div(-c2 - q, 3.0 * c3), _div(-c2 + q, 3.0 * c3)
        ta, tb = (u, v) if u < v else (v, u)
        clamp = lambda t: -R if t < -R else (R if t > R else t)
        e = [-R, clamp(ta), clamp(tb), R]
    val = [horner(t) for t in e]
    roots = []
    for j in range(len(e)):
        if val[j] == 0.0 and len(roots) < 3:
            roots.append(e[j])
        if j + 1 < len(e) and ((val[j] < 0.0 and val[j + 1] > 0.0) or (val[j] > 0.0 and val[j + 1] < 0.0)) and len(roots) < 3:
            lo, hi, neg = e[j], e[j + 1], val[j] < 0.0
            for _ in range(128):
                mid = 0.5 * (lo + hi)
                if mid == lo or mid == hi:
                    break
                fm = horner(mid)
                if fm == 0.0:
                    lo = mid
                    break
                if (fm < 0.0) == neg:
                    lo = mid
                else:
                    hi = mid
            roots.append(lo)
    return roots


def slot_model(l, f1, f2):
    """step 7: nine floats, or None for an invalid slot"""
    with np.errstate(all="ignore"):
        Fm = F64(l) * np.array(f1, F64) + np.array(f2, F64)
        q = F64(0.0)
        for j in range(9):
            q = q + Fm[j] * Fm[j]
        nrm = np.sqrt(q)
        if not (nrm > 0.0 and _finite(nrm)):
            return None
        Fm = Fm / nrm
        big, at = F64(0.0), 0
        for j in range(9):
            if abs(Fm[j]) > big:
                big, at = abs(Fm[j]), j
        if Fm[at] < 0.0:
            Fm = -Fm
    return Fm


def models(src, dst, subset):
    """the three slots of one hypothesis: a list of three entries, each nine float64 or None"""
    nv = null_vectors(src, dst, subset)
    out = [None, None, None]
    if nv is None:
        return out
    f1, f2 = nv
    for s, l in enumerate(real_roots(*cubic(f1, f2))):
        out[s] = slot_model(l, f1, f2)
    return out


def errors(f, x, y, X, Y):
    """the symmetric squared epipolar distance, elementwise over arrays of float64"""
    with np.errstate(all="ignore"):
        a = (f[0] * x + f[1] * y) + f[2]
        b = (f[3] * x + f[4] * y) + f[5]
        c = (f[6] * x + f[7] * y) + f[8]
        d2 = (X * a + Y * b) + c
        s2 = 1.0 / (a * a + b * b)
        a_ = (f[0] * X + f[3] * Y) + f[6]
        b_ = (f[1] * X + f[4] * Y) + f[7]
        c_ = (f[2] * X + f[5] * Y) + f[8]
        d1 = (x * a_ + y * b_) + c_
        s1 = 1.0 / (a_ * a_ + b_ * b_)
        e1, e2 = (d1 * d1) * s1, (d2 * d2) * s2
        return np.where((e1 > e2) | (e1 != e1), e1, e2)


def pair_errors(f, src, dst):
    return errors(np.asarray(f, F64).ravel(), src[:, 0], src[:, 1], dst[:, 0], dst[:, 1])


def counts(src, dst, subsets, threshold):
    """count[it][slot] (max_iters, 3) int32, -1 for an invalid slot, and the models (a list of lists)"""
    t2 = F64(threshold) * F64(threshold)
    out = np.full((len(subsets), 3), -1, np.int32)
    ms = []
    for it, sub in enumerate(subsets):
        m3 = models(src, dst, sub)
        ms.append(m3)
        for s, f in enumerate(m3):
            if f is not None:
                out[it, s] = int(np.count_nonzero(pair_errors(f, src, dst) <= t2))
    return out, ms


def choose(count: np.ndarray, need: np.ndarray):
    """The sequential loop over (max_iters, 3) counts: (best_iter, best_slot, iters_run, valid, best_count)"""
    niters, best, best_count, it = len(count), (-1, -1), 6, 0
    while it < niters:
        for s in range(3):
            if count[it, s] > best_count:
                best, best_count = (it, s), int(count[it, s])
                niters = min(niters, int(need[best_count]))
        it += 1
    ran = it
    return best[0], best[1], ran, int(np.count_nonzero(count[:ran] >= 0)), best_count if best[0] >= 0 else 0


def find_one(src, dst, subsets, threshold=3.0, confidence=0.99, count=None) -> dict:
    """One item: dict(F (3, 3), inliers (n,) uint8, record (RECORD_DTYPE scalar), count (max_iters, 3))"""
    src, dst = np.ascontiguousarray(src, F64), np.ascontiguousarray(dst, F64)
    subsets = np.asarray(subsets, np.int32).reshape(-1, 7)
    n, max_iters = src.shape[0], subsets.shape[0]
    t2 = F64(threshold) * F64(threshold)
    ms = None
    if count is None:
        count, ms = counts(src, dst, subsets, threshold)
    bi, bs, ran, valid, g = choose(count, need_table(n, confidence, max_iters))
    rec = np.zeros((), RECORD_DTYPE)
    rec["best_iter"], rec["best_slot"], rec["iters_run"], rec["valid"] = bi, bs, ran, valid
    if bi < 0:
        return dict(F=np.zeros((3, 3)), inliers=np.zeros(n, np.uint8), record=rec, count=count)
    f = ms[bi][bs] if ms is not None else models(src, dst, subsets[bi])[bs]
    err = pair_errors(f, src, dst)
    inl = err <= t2
    rec["ok"], rec["inliers"] = 1, g
    rec["sq_error"] = np.cumsum(np.where(inl, err, 0.0))[-1]           # left to right, one accumulator
    return dict(F=np.array(f, F64).reshape(3, 3), inliers=inl.astype(np.uint8), record=rec, count=count)


def find(src, dst, subsets, threshold=3.0, confidence=0.99) -> dict:
    """A batch: src, dst (B, n, 2), subsets (B, max_iters, 7) -> dict(F (B, 3, 3), inliers (B, n) uint8, records (B,) RECORD_DTYPE)"""
    src, dst, subsets = np.asarray(src, F64), np.asarray(dst, F64), np.asarray(subsets, np.int32)
    items = [find_one(s, d, t, threshold, confidence) for s, d, t in zip(src, dst, subsets)]
    return dict(F=np.stack([i["F"] for i in items]), inliers=np.stack([i["inliers"] for i in items]),
                records=np.array([i["record"] for i in items], RECORD_DTYPE))


def flow_pairs(flow, coords):
    """detector.py:126-128 from float32 fields (B, H, W, 2) and (n, 2) integer (x, y): src, dst (B, n, 2) float64"""
    flow, coords = np.asarray(flow, np.float32), np.asarray(coords)
    src = np.broadcast_to(coords.astype(F64), (flow.shape[0],) + coords.shape)
    return np.ascontiguousarray(src), src + flow[:, coords[:, 1], coords[:, 0]].astype(F64)


def epipolar_residual(flow, Fm, threshold=1.0) -> dict:
    """The dense pass: flow (B, H, W, 2) float32, Fm (B, 3, 3) -> dict(residual (B, H, W) float32, mask uint8, records (B,) EPI_DTYPE)"""
    flow, Fm = np.asarray(flow, np.float32), np.asarray(Fm, F64)
    B, H, W = flow.shape[:3]
    ys, xs = np.mgrid[0:H, 0:W].astype(F64)
    res, mask, rec = np.zeros((B, H, W), np.float32), np.zeros((B, H, W), np.uint8), np.zeros(B, EPI_DTYPE)
    t2 = F64(threshold) * F64(threshold)
    for b in range(B):
        err = errors(Fm[b].ravel(), xs, ys, xs + flow[b, ..., 0].astype(F64), ys + flow[b, ..., 1].astype(F64))
        with np.errstate(all="ignore"):
            fin = err - err == 0.0
            res[b] = np.where(fin, np.sqrt(np.where(fin, err, 0.0)).astype(np.float32), np.float32(0))
            mask[b] = np.where(fin & (err > t2), 255, 0)
        rec[b]["movers"], rec[b]["not_finite"] = np.count_nonzero(mask[b]), np.count_nonzero(~fin)
        if fin.any():
            at = int(np.argmax(np.where(fin, res[b], np.float32(-1)).ravel()))     # argmax: the first of equals
            rec[b]["max_residual"], rec[b]["max_row"], rec[b]["max_col"] = res[b].ravel()[at], at // W, at % W
        else:
            rec[b]["max_row"], rec[b]["max_col"] = -1, -1
    return dict(residual=res, mask=mask, records=rec)
