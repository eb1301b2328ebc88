"""include/mavflow_affine.h in numpy, in the header's order: every operation float64 and rounded on its own (numpy fuses nothing), sums
in plain index order (np.cumsum adds left to right).  The device must equal this byte for byte; this file is held to the definition by
tests/test_affine_ref_cpu.py.  Nothing here is pinned against cv2."""
import math

import numpy as np

MAX_PAIRS, MAX_ITERS, RANK_RATIO = 65536, 4096, 1e-12
RECORD_DTYPE = np.dtype([("ok", np.int32), ("inliers", np.int32), ("best_iter", np.int32), ("iters_run", np.int32), ("valid", np.int32),
                         ("refined", np.int32), ("sq_error", np.float64)])
assert RECORD_DTYPE.itemsize == 32
F = np.float64
COS2 = F(0.996) * F(0.996)
DBL_MIN = np.finfo(np.float64).tiny


def need_quotient(n: int, g: int, confidence: float):
    """(ln, ld) of need[g], or None where no quotient is taken (g < 3, or den < DBL_MIN)"""
    if g < 3:
        return None
    w = g / n
    den = 1.0 - (w * w) * w
    if den < DBL_MIN:
        return None
    return math.log(1.0 - confidence), math.log(den)


def need_table(n: int, confidence: float, max_iters: int) -> np.ndarray:
    """need[g], g = 0 .. n: RANSACUpdateNumIters(confidence, (n - g) / n, 3, max_iters)"""
    need = np.empty(n + 1, np.int32)
    for g in range(n + 1):
        if g < 3:
            need[g] = max_iters
            continue
        q = need_quotient(n, g, confidence)
        if q is None:
            need[g] = 0
            continue
        ln, ld = q
        need[g] = max_iters if (ld >= 0.0 or -ln >= max_iters * (-ld)) else int(np.rint(ln / ld))
    return need


def _flat(a, b, c) -> bool:
    d1x, d1y, d2x, d2y = b[0] - c[0], b[1] - c[1], a[0] - c[0], a[1] - c[1]
    l1, l2, dot = d1x * d1x + d1y * d1y, d2x * d2x + d2y * d2y, d1x * d2x + d1y * d2y
    return bool(l1 == 0.0 or l2 == 0.0 or dot * dot > COS2 * (l1 * l2))


def model(src: np.ndarray, dst: np.ndarray, tri):
    """The model through the three pairs of one triple: (6 float64, valid)"""
    n = src.shape[0]
    i0, i1, i2 = (int(v) for v in tri)
    zero = np.zeros(6)
    if not (0 <= i0 < n and 0 <= i1 < n and 0 <= i2 < n) or i0 == i1 or i0 == i2 or i1 == i2:
        return zero, False
    with np.errstate(all="ignore"):
        a, b, c, A, B, C = src[i0], src[i1], src[i2], dst[i0], dst[i1], dst[i2]
        if _flat(a, b, c) or _flat(A, B, C):
            return zero, False
        dx1, dy1, dx2, dy2 = b[0] - a[0], b[1] - a[1], c[0] - a[0], c[1] - a[1]
        det = dx1 * dy2 - dx2 * dy1
        if not det != 0.0:
            return zero, False
        dX1, dX2, dY1, dY2 = B[0] - A[0], C[0] - A[0], B[1] - A[1], C[1] - A[1]
        m00 = (dX1 * dy2 - dX2 * dy1) / det
        m01 = (dx1 * dX2 - dx2 * dX1) / det
        m02 = (A[0] - m00 * a[0]) - m01 * a[1]
        m10 = (dY1 * dy2 - dY2 * dy1) / det
        m11 = (dx1 * dY2 - dx2 * dY1) / det
        m12 = (A[1] - m10 * a[0]) - m11 * a[1]
    m = np.array([m00, m01, m02, m10, m11, m12], F)
    if not np.all(np.isfinite(m)):
        return zero, False
    return m, True


def errors(m, src, dst) -> np.ndarray:
    with np.errstate(all="ignore"):
        e0 = ((m[0] * src[:, 0] + m[1] * src[:, 1]) + m[2]) - dst[:, 0]
        e1 = ((m[3] * src[:, 0] + m[4] * src[:, 1]) + m[5]) - dst[:, 1]
        return e0 * e0 + e1 * e1


def counts(src, dst, triples, threshold) -> np.ndarray:
    """count[it] for every hypothesis; -1 marks an invalid one (whose count is 0)"""
    t2 = F(threshold) * F(threshold)
    out = np.empty(len(triples), np.int32)
    for it, tri in enumerate(triples):
        m, valid = model(src, dst, tri)
        out[it] = int(np.count_nonzero(errors(m, src, dst) <= t2)) if valid else -1
    return out


def choose(count: np.ndarray, need: np.ndarray):
    """The sequential loop: (best, niters, valid hypotheses among those run, best_count)"""
    niters, best, best_count, it = len(count), -1, 2, 0
    while it < niters:
        if count[it] > best_count:
            best, best_count = it, int(count[it])
            niters = min(niters, int(need[best_count]))
        it += 1
    return best, niters, int(np.count_nonzero(count[:niters] >= 0)), best_count if best >= 0 else 0


def _sum(terms: np.ndarray):
    return np.cumsum(terms)[-1]                # left to right, one accumulator; an accumulator that starts at +0.0 adds the same bits


def refine_fit(src, dst, inl):
    """The least-squares map over the inliers: (6 float64, accepted by the rank test)"""
    with np.errstate(all="ignore"):
        z = lambda t: np.where(inl, t, 0.0)
        g = F(np.count_nonzero(inl))
        x, y, X, Y = src[:, 0], src[:, 1], dst[:, 0], dst[:, 1]
        mx, my, mX, mY = _sum(z(x)) / g, _sum(z(y)) / g, _sum(z(X)) / g, _sum(z(Y)) / g
        u, v, P, Q = x - mx, y - my, X - mX, Y - mY
        Suu, Suv, Svv = _sum(z(u * u)), _sum(z(u * v)), _sum(z(v * v))
        SuP, SvP, SuQ, SvQ = _sum(z(u * P)), _sum(z(v * P)), _sum(z(u * Q)), _sum(z(v * Q))
        D, T = Suu * Svv - Suv * Suv, Suu + Svv
        r00 = (SuP * Svv - SvP * Suv) / D
        r01 = (Suu * SvP - Suv * SuP) / D
        r02 = (mX - r00 * mx) - r01 * my
        r10 = (SuQ * Svv - SvQ * Suv) / D
        r11 = (Suu * SvQ - Suv * SuQ) / D
        r12 = (mY - r10 * mx) - r11 * my
        r = np.array([r00, r01, r02, r10, r11, r12], F)
        return r, bool(D > F(RANK_RATIO) * (T * T)) and bool(np.all(np.isfinite(r)))


def estimate_one(src, dst, triples, threshold=3.0, confidence=0.99, refine=True, count=None) -> dict:
    """One item: dict(M (2, 3), inliers (n,) uint8, record (RECORD_DTYPE scalar), count (max_iters,))"""
    src, dst = np.ascontiguousarray(src, F), np.ascontiguousarray(dst, F)
    triples = np.asarray(triples, np.int32).reshape(-1, 3)
    n, max_iters = src.shape[0], triples.shape[0]
    t2 = F(threshold) * F(threshold)
    count = counts(src, dst, triples, threshold) if count is None else np.asarray(count, np.int32)
    best, niters, valid, g = choose(count, need_table(n, confidence, max_iters))
    rec = np.zeros((), RECORD_DTYPE)
    rec["best_iter"], rec["iters_run"], rec["valid"] = best, niters, valid
    if best < 0:
        return dict(M=np.zeros((2, 3)), inliers=np.zeros(n, np.uint8), record=rec, count=count)
    m, _ = model(src, dst, triples[best])
    inl = errors(m, src, dst) <= t2
    M, refined = m, 0
    if refine:
        r, accepted = refine_fit(src, dst, inl)
        if accepted:
            M, refined = r, 1
    rec["ok"], rec["inliers"], rec["refined"] = 1, g, refined
    rec["sq_error"] = _sum(np.where(inl, errors(M, src, dst), 0.0))
    return dict(M=M.reshape(2, 3).copy(), inliers=inl.astype(np.uint8), record=rec, count=count)


def estimate(src, dst, triples, threshold=3.0, confidence=0.99, refine=True) -> dict:
    """A batch: src, dst (B, n, 2), triples (B, max_iters, 3) -> dict(M (B, 2, 3), inliers (B, n) uint8, records (B,) RECORD_DTYPE)"""
    src, dst, triples = np.asarray(src, F), np.asarray(dst, F), np.asarray(triples, np.int32)
    items = [estimate_one(s, d, t, threshold, confidence, refine) for s, d, t in zip(src, dst, triples)]
    return dict(M=np.stack([i["M"] for i in items]), inliers=np.stack([i["inliers"] for i in items]),
                records=np.array([i["record"] for i in items], RECORD_DTYPE))


def flow_pairs(flow, coords):
    """detector.py:126-128 from float32 fields (B, H, W, 2) and (n, 2) integer (x, y): src, dst (B, n, 2) float64"""
    flow, coords = np.asarray(flow, np.float32), np.asarray(coords)
    src = np.broadcast_to(coords.astype(F), (flow.shape[0],) + coords.shape)
    return np.ascontiguousarray(src), src + flow[:, coords[:, 1], coords[:, 0]].astype(F)
