"""include/mavflow_essential.h in numpy, in the header's order, vectorised ACROSS HYPOTHESES: every operation is an element-wise float64
operation rounded on its own (numpy fuses nothing), so a column of an array sees exactly the scalar loop's sequence of operations; the
bisections of all hypotheses and intervals run in lock-step under masks.  Sums are in plain index order.  The device must equal this byte
for byte; this file is held to the definition by tests/test_essential_ref_cpu.py.  Nothing here is pinned against cv2."""
import math

import numpy as np

MAX_PAIRS, MAX_ITERS, SLOTS = 65536, 4096, 10
RECORD_DTYPE = np.dtype([("ok", np.int32), ("inliers", np.int32), ("best_iter", np.int32), ("best_slot", np.int32), ("iters_run", np.int32),
                         ("valid", np.int32), ("sq_error", np.float64)])
assert RECORD_DTYPE.itemsize == 32
F64 = np.float64
DBL_MIN = np.finfo(np.float64).tiny
CAMERA = (1.0, 1.0, 0.0, 0.0)              # fx, fy, cx, cy of mav_essential_defaults

# exponents (of x, y, z) of the monomials of a linear form, of Q and of C, in the header's orders
LIN = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0))
QUAD = ((2, 0, 0), (1, 1, 0), (1, 0, 1), (1, 0, 0), (0, 2, 0), (0, 1, 1), (0, 1, 0), (0, 0, 2), (0, 0, 1), (0, 0, 0))
CUBE = ((3, 0, 0), (0, 3, 0), (2, 1, 0), (1, 2, 0), (2, 0, 1), (2, 0, 0), (0, 2, 1), (0, 2, 0), (1, 1, 1), (1, 1, 0),
        (1, 0, 2), (1, 0, 1), (1, 0, 0), (0, 1, 2), (0, 1, 1), (0, 1, 0), (0, 0, 3), (0, 0, 2), (0, 0, 1), (0, 0, 0))
_add = lambda a, b: tuple(p + q for p, q in zip(a, b))
M2 = [[QUAD.index(_add(LIN[i], LIN[j])) for j in range(4)] for i in range(4)]
M3 = [[CUBE.index(_add(QUAD[i], LIN[j])) for j in range(4)] for i in range(10)]


def need_quotient(n: int, g: int, confidence: float):
    """(ln, ld) of need[g], or None where no quotient is taken (g < 5, or den < DBL_MIN)"""
    if g < 5:
        return None
    w = g / n
    w2 = w * w
    den = 1.0 - (w2 * w2) * w
    if den < DBL_MIN:
        return None
    return math.log(1.0 - confidence), math.log(den)


def need_table(n: int, confidence: float, max_iters: int) -> np.ndarray:
    """need[g], g = 0 .. n: RANSACUpdateNumIters(confidence, (n - g) / n, 5, max_iters)"""
    need = np.empty(n + 1, np.int32)
    for g in range(n + 1):
        if g < 5:
            need[g] = max_iters
            continue
        q = need_quotient(n, g, confidence)
        if q is None:
            need[g] = 0
            continue
        ln, ld = q
        need[g] = max_iters if (ld >= 0.0 or -ln >= max_iters * (-ld)) else int(np.rint(ln / ld))
    return need


def _finite(v):
    with np.errstate(all="ignore"):
        return v - v == 0.0


def normalised(pts, camera):
    """(x, y) of (..., 2) pixels"""
    fx, fy, cx, cy = (F64(v) for v in camera)
    with np.errstate(all="ignore"):
        return (pts[..., 0] - cx) / fx, (pts[..., 1] - cy) / fy


def mul2(a, b):
    q = np.zeros((a.shape[0], 10))
    for i in range(4):
        for j in range(4):
            q[:, M2[i][j]] = q[:, M2[i][j]] + a[:, i] * b[:, j]
    return q


def mul3(q, l):
    c = np.zeros((q.shape[0], 20))
    for i in range(10):
        for j in range(4):
            c[:, M3[i][j]] = c[:, M3[i][j]] + q[:, i] * l[:, j]
    return c


def conv(a, b):
    """polynomials in z, ascending degree, (H, da + 1) and (H, db + 1)"""
    o = np.zeros((a.shape[0], a.shape[1] + b.shape[1] - 1))
    for i in range(a.shape[1]):
        for j in range(b.shape[1]):
            o[:, i + j] = o[:, i + j] + a[:, i] * b[:, j]
    return o


def horner(a, t):
    """a (H, d + 1) ascending; t (H,) or (H, w)"""
    col = (lambda j: a[:, j]) if t.ndim == 1 else (lambda j: a[:, j, None])
    v = np.broadcast_to(col(a.shape[1] - 1), t.shape)
    for j in range(a.shape[1] - 2, -1, -1):
        v = v * t + col(j)
    return v


def null_vectors(x, y, X, Y, subsets):
    """steps 1 - 4 for (H, 5) subsets of n normalised pairs: ok (H,) bool and e (H, 4, 9)"""
    n, H = len(x), len(subsets)
    sub = np.asarray(subsets, np.int64)
    ok = ((sub >= 0) & (sub < n)).all(1)
    for j in range(5):
        for i in range(j):
            ok &= sub[:, i] != sub[:, j]
    sub = np.where(ok[:, None], sub, 0)
    x, y, X, Y = x[sub], y[sub], X[sub], Y[sub]
    A = np.stack([X * x, X * y, X, Y * x, Y * y, Y, x, y, np.ones_like(x)], -1)          # (H, 5, 9)
    perm = np.tile(np.arange(9), (H, 1))
    hh = np.arange(H)
    for k in range(5):
        v = np.abs(A[:, k:, k:])
        v = np.where(v != v, -1.0, v).reshape(H, -1)                                      # a NaN never wins
        at = np.argmax(v, 1)                                                              # the first of equals
        pv = v[hh, at]
        ok &= (pv > 0.0) & _finite(pv)
        pr, pc = k + at // (9 - k), k + at % (9 - k)
        pr, pc = np.where(pv > 0.0, pr, k), np.where(pv > 0.0, pc, k)
        t = A[hh, k].copy(); A[hh, k] = A[hh, pr]; A[hh, pr] = t
        t = A[hh, :, k].copy(); A[hh, :, k] = A[hh, :, pc]; A[hh, :, pc] = t
        t = perm[hh, k].copy(); perm[hh, k] = perm[hh, pc]; perm[hh, pc] = t
        p = A[:, k, k].copy()
        A[:, k, k + 1:] = A[:, k, k + 1:] / p[:, None]
        for r in range(5):
            if r != k:
                m = A[:, r, k].copy()
                A[:, r, k + 1:] = A[:, r, k + 1:] - m[:, None] * A[:, k, k + 1:]
    e = np.zeros((H, 4, 9))
    for j in range(4):
        for i in range(5):
            e[hh, j, perm[:, i]] = -A[:, i, 5 + j]
        e[hh, j, perm[:, 5 + j]] = 1.0
    return ok, e


def cubics(e):
    """step 5: M (H, 10, 20)"""
    E = [np.ascontiguousarray(e[:, :, m]) for m in range(9)]                              # the linear form of entry m: (H, 4)
    M = np.empty((e.shape[0], 10, 20))
    P0 = mul2(E[4], E[8]) - mul2(E[5], E[7])
    P1 = mul2(E[3], E[8]) - mul2(E[5], E[6])
    P2 = mul2(E[3], E[7]) - mul2(E[4], E[6])
    M[:, 0] = (mul3(P0, E[0]) - mul3(P1, E[1])) + mul3(P2, E[2])
    S = [[None] * 3 for _ in range(3)]
    for i in range(3):
        for j in range(i, 3):
            S[i][j] = (mul2(E[3 * i], E[3 * j]) + mul2(E[3 * i + 1], E[3 * j + 1])) + mul2(E[3 * i + 2], E[3 * j + 2])
            S[j][i] = S[i][j]
    h = 0.5 * ((S[0][0] + S[1][1]) + S[2][2])
    L = [[S[i][j] - h if i == j else S[i][j] for j in range(3)] for i in range(3)]
    for i in range(3):
        for j in range(3):
            M[:, 1 + 3 * i + j] = (mul3(L[i][0], E[j]) + mul3(L[i][1], E[3 + j])) + mul3(L[i][2], E[6 + j])
    return M


def reduced(M, ok):
    """step 6, in place: ok narrowed"""
    H = M.shape[0]
    hh = np.arange(H)
    for k in range(10):
        v = np.abs(M[:, k:, k])
        v = np.where(v != v, -1.0, v)
        at = np.argmax(v, 1)
        pv = v[hh, at]
        ok = ok & (pv > 0.0) & _finite(pv)
        pr = np.where(pv > 0.0, k + at, k)
        t = M[hh, k].copy(); M[hh, k] = M[hh, pr]; M[hh, pr] = t
        p = M[:, k, k].copy()
        M[:, k, k + 1:] = M[:, k, k + 1:] / p[:, None]
        for r in range(10):
            if r != k and (r > k or r >= 4):
                m = M[:, r, k].copy()
                M[:, r, k + 1:] = M[:, r, k + 1:] - m[:, None] * M[:, k, k + 1:]
    return ok


def b_rows(M):
    """step 7: B as a list of three rows, each (bx (H, 4), by (H, 4), b1 (H, 5))"""
    rows = []
    for q in range(3):
        e, f = M[:, 4 + 2 * q], M[:, 5 + 2 * q]
        bx = np.stack([e[:, 12], e[:, 11] - f[:, 12], e[:, 10] - f[:, 11], -f[:, 10]], 1)
        by = np.stack([e[:, 15], e[:, 14] - f[:, 15], e[:, 13] - f[:, 14], -f[:, 13]], 1)
        b1 = np.stack([e[:, 19], e[:, 18] - f[:, 19], e[:, 17] - f[:, 18], e[:, 16] - f[:, 17], -f[:, 16]], 1)
        rows.append((bx, by, b1))
    return rows


def det_b(B):
    """step 8: c (H, 11) ascending"""
    p1 = conv(B[1][1], B[2][2]) - conv(B[1][2], B[2][1])
    p2 = conv(B[1][0], B[2][2]) - conv(B[1][2], B[2][0])
    p3 = conv(B[1][0], B[2][1]) - conv(B[1][1], B[2][0])
    return (conv(B[0][0], p1) - conv(B[0][1], p2)) + conv(B[0][2], p3)


def real_roots(c, ok):
    """step 9: (roots (H, 10) with NaN beyond the count, count (H,)); count 0 where not ok or where there is no model"""
    H = c.shape[0]
    hh = np.arange(H)
    ok = ok & (c[:, 10] != 0.0) & _finite(c).all(1)
    mx = np.zeros(H)
    for i in range(10):
        q = np.abs(c[:, i] / c[:, 10])
        mx = np.where(q > mx, q, mx)
    R = 1.0 + mx
    ok = ok & _finite(R)
    D = [c]
    for k in range(9):
        D.append(np.stack([F64(j) * D[k][:, j] for j in range(1, 11 - k)], 1))
    clamp = lambda t: np.where(t < -R, -R, np.where(t > R, R, t))
    lst = np.full((H, 10), np.nan)
    lst[:, 0] = clamp((-D[9][:, 0]) / D[9][:, 1])
    cnt = np.ones(H, np.int64)
    W = 12
    for k in range(8, -1, -1):
        d = 10 - k
        P = np.full((H, W), np.nan)
        P[:, 0] = -R
        for i in range(10):
            P[:, 1 + i] = np.where(i < cnt, lst[:, i], P[:, 1 + i])
        P[hh, cnt + 1] = R
        npts = cnt + 2
        v = horner(D[k], P)
        jj = np.arange(W)[None, :]
        zero = (v == 0.0) & (jj < npts[:, None])
        v0, v1 = v[:, :-1], v[:, 1:]
        change = (jj[:, 1:] < npts[:, None]) & (((v0 < 0.0) & (v1 > 0.0)) | ((v0 > 0.0) & (v1 < 0.0)))
        lo, hi, neg, active = P[:, :-1].copy(), P[:, 1:].copy(), v0 < 0.0, change.copy()
        for _ in range(128):
            if not active.any():
                break
            mid = 0.5 * (lo + hi)
            active &= ~((mid == lo) | (mid == hi))
            fm = horner(D[k], mid)
            hit = active & (fm == 0.0)
            lo = np.where(hit, mid, lo)
            active &= ~hit
            left = active & ((fm < 0.0) == neg)
            right = active & ~left
            lo = np.where(left, mid, lo)
            hi = np.where(right, mid, hi)
        new, cnt = np.full((H, 10), np.nan), np.zeros(H, np.int64)
        for j in range(W):
            take = zero[:, j] & (cnt < d)
            new[hh[take], cnt[take]] = P[take, j]
            cnt = cnt + take
            if j + 1 < W:
                take = change[:, j] & (cnt < d)
                new[hh[take], cnt[take]] = lo[take, j]
                cnt = cnt + take
        lst = new
    return lst, np.where(ok, cnt, 0)


POLISH_STEPS = 4


def _det3(m):
    return (m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6])) + m[2] * (m[3] * m[7] - m[4] * m[6])


def _abt(a, b, i, j):
    """(A B^T)[i][j] of row-major lists of nine arrays"""
    return (a[3 * i] * b[3 * j] + a[3 * i + 1] * b[3 * j + 1]) + a[3 * i + 2] * b[3 * j + 2]


def _ab(a, b, i, j):
    """(A B)[i][j]"""
    return (a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j]) + a[3 * i + 2] * b[6 + j]


def polished(x, y, z, e):
    """step 10's POLISH: POLISH_STEPS Gauss-Newton steps of (x, y, z) on the ten constraints, all hypotheses at once; (H,) arrays"""
    p = [x, y, z]
    e1, e2, e3, e4 = ([e[:, j, m] for m in range(9)] for j in range(4))
    for _ in range(POLISH_STEPS):
        G = [((p[0] * e1[m] + p[1] * e2[m]) + p[2] * e3[m]) + e4[m] for m in range(9)]
        S = [_abt(G, G, i, j) for i in range(3) for j in range(3)]
        h = 0.5 * ((S[0] + S[4]) + S[8])
        r = [_det3(G)] + [_ab(S, G, i, j) - h * G[3 * i + j] for i in range(3) for j in range(3)]
        C = [G[4] * G[8] - G[5] * G[7], G[5] * G[6] - G[3] * G[8], G[3] * G[7] - G[4] * G[6],
             G[2] * G[7] - G[1] * G[8], G[0] * G[8] - G[2] * G[6], G[1] * G[6] - G[0] * G[7],
             G[1] * G[5] - G[2] * G[4], G[2] * G[3] - G[0] * G[5], G[0] * G[4] - G[1] * G[3]]
        J = []
        for D in (e1, e2, e3):
            j0 = np.zeros_like(x)
            for m in range(9):
                j0 = j0 + C[m] * D[m]
            T = [_abt(D, G, i, j) for i in range(3) for j in range(3)]
            dS = [T[3 * i + j] + T[3 * j + i] for i in range(3) for j in range(3)]
            dh = 0.5 * ((dS[0] + dS[4]) + dS[8])
            J.append([j0] + [((_ab(dS, G, i, j) + _ab(S, D, i, j)) - dh * G[3 * i + j]) - h * D[3 * i + j] for i in range(3) for j in range(3)])
        N = [None] * 9
        g = []
        for a in range(3):
            for b in range(a, 3):
                acc = np.zeros_like(x)
                for k in range(10):
                    acc = acc + J[a][k] * J[b][k]
                N[3 * a + b] = N[3 * b + a] = acc
            acc = np.zeros_like(x)
            for k in range(10):
                acc = acc + J[a][k] * r[k]
            g.append(acc)
        dd = _det3(N)
        delta = []
        for a in range(3):
            Na = list(N)
            Na[a], Na[3 + a], Na[6 + a] = g[0], g[1], g[2]
            delta.append(_det3(Na) / dd)
        step = (dd != 0.0) & _finite(delta[0]) & _finite(delta[1]) & _finite(delta[2])
        p = [np.where(step, p[a] - delta[a], p[a]) for a in range(3)]
    return p


def slot_models(roots, count, B, e):
    """step 10: models (H, 10, 9), zero where invalid, and valid (H, 10) bool"""
    H = roots.shape[0]
    models, valid = np.zeros((H, 10, 9)), np.zeros((H, 10), bool)
    for s in range(10):
        z = np.where(s < count, roots[:, s], 0.0)
        kx, ky, k1 = horner(B[0][0], z), horner(B[0][1], z), horner(B[0][2], z)
        lx, ly, l1 = horner(B[1][0], z), horner(B[1][1], z), horner(B[1][2], z)
        v0, v1, v2 = ky * l1 - k1 * ly, k1 * lx - kx * l1, kx * ly - ky * lx
        x, y = v0 / v2, v1 / v2
        ok = (s < count) & (v2 != 0.0) & _finite(x) & _finite(y)
        x, y, zp = polished(x, y, z, e)
        G = ((x[:, None] * e[:, 0] + y[:, None] * e[:, 1]) + zp[:, None] * e[:, 2]) + e[:, 3]
        q = np.zeros(H)
        for j in range(9):
            q = q + G[:, j] * G[:, j]
        nrm = np.sqrt(q)
        ok = ok & (nrm > 0.0) & _finite(nrm)
        G = G / nrm[:, None]
        a = np.abs(G)
        at = np.argmax(np.where(a != a, -1.0, a), 1)                                      # strict >, the first of equals
        flip = G[np.arange(H), at] < 0.0
        G = np.where(flip[:, None], -G, G)
        models[:, s] = np.where(ok[:, None], G, 0.0)
        valid[:, s] = ok
    return models, valid


def solve(src, dst, subsets, camera=CAMERA) -> dict:
    """every hypothesis of one item: dict(models (H, 10, 9), valid (H, 10), nroots (H,), c (H, 11), ok (H,))"""
    src, dst = np.ascontiguousarray(src, F64), np.ascontiguousarray(dst, F64)
    subsets = np.asarray(subsets, np.int32).reshape(-1, 5)
    with np.errstate(all="ignore"):
        x, y = normalised(src, camera)
        X, Y = normalised(dst, camera)
        ok, e = null_vectors(x, y, X, Y, subsets)
        M = cubics(e)
        ok = reduced(M, ok)
        B = b_rows(M)
        c = det_b(B)
        roots, count = real_roots(c, ok)
        models, valid = slot_models(roots, count, B, e)
    return dict(models=models, valid=valid, nroots=count, c=c, ok=ok, roots=roots, e=e)


def errors(E, x, y, X, Y):
    """the Sampson error; E (..., 9) broadcast against the points"""
    with np.errstate(all="ignore"):
        a0 = (E[..., 0] * x + E[..., 1] * y) + E[..., 2]
        a1 = (E[..., 3] * x + E[..., 4] * y) + E[..., 5]
        a2 = (E[..., 6] * x + E[..., 7] * y) + E[..., 8]
        b0 = (E[..., 0] * X + E[..., 3] * Y) + E[..., 6]
        b1 = (E[..., 1] * X + E[..., 4] * Y) + E[..., 7]
        d = (X * a0 + Y * a1) + a2
        return (d * d) / (((a0 * a0 + a1 * a1) + b0 * b0) + b1 * b1)


def threshold2(threshold, camera):
    fx, fy = F64(camera[0]), F64(camera[1])
    t = F64(threshold) / ((fx + fy) / F64(2.0))
    return t * t


def pair_errors(E, src, dst, camera=CAMERA):
    x, y = normalised(np.asarray(src, F64), camera)
    X, Y = normalised(np.asarray(dst, F64), camera)
    return errors(np.asarray(E, F64).reshape(9), x, y, X, Y)


def counts(src, dst, models, valid, threshold, camera=CAMERA):
    """count[it][slot] (H, 10) int32, -1 for an invalid slot"""
    x, y = normalised(np.asarray(src, F64), camera)
    X, Y = normalised(np.asarray(dst, F64), camera)
    t2 = threshold2(threshold, camera)
    out = np.full(valid.shape, -1, np.int32)
    flat = models.reshape(-1, 9)[valid.ravel()]
    got = np.empty(len(flat), np.int32)
    for o in range(0, len(flat), 256):
        got[o:o + 256] = np.count_nonzero(errors(flat[o:o + 256, None, :], x, y, X, Y) <= t2, axis=1)
    out[valid] = got
    return out


def choose(count: np.ndarray, need: np.ndarray):
    """The sequential loop over (max_iters, 10) counts: (best_iter, best_slot, iters_run, valid, best_count)"""
    niters, best, best_count, it = len(count), (-1, -1), 4, 0
    while it < niters:
        for s in range(SLOTS):
            if count[it, s] > best_count:
                best, best_count = (it, s), int(count[it, s])
                niters = min(niters, int(need[best_count]))
        it += 1
    ran = it
    return best[0], best[1], ran, int(np.count_nonzero(count[:ran] >= 0)), best_count if best[0] >= 0 else 0


def pixel_F(E, camera):
    """F = K^-T E K^-1 as the header writes it out; (3, 3)"""
    fx, fy, cx, cy = (F64(v) for v in camera)
    E = np.asarray(E, F64).reshape(3, 3)
    G, Hm = np.empty((3, 3)), np.empty((3, 3))
    with np.errstate(all="ignore"):
        for i in range(3):
            G[i, 0] = E[i, 0] / fx
            G[i, 1] = E[i, 1] / fy
            G[i, 2] = (E[i, 2] - G[i, 0] * cx) - G[i, 1] * cy
        for j in range(3):
            Hm[0, j] = G[0, j] / fx
            Hm[1, j] = G[1, j] / fy
            Hm[2, j] = (G[2, j] - Hm[0, j] * cx) - Hm[1, j] * cy
        h = Hm.ravel()
        q = F64(0.0)
        for j in range(9):
            q = q + h[j] * h[j]
        nrm = np.sqrt(q)
        if not (nrm > 0.0 and _finite(nrm)):
            return np.zeros((3, 3))
        h = h / nrm
        a = np.abs(h)
        if h[int(np.argmax(np.where(a != a, -1.0, a)))] < 0.0:
            h = -h
    return h.reshape(3, 3)


def find_one(src, dst, subsets, threshold=1.0, confidence=0.999, camera=CAMERA) -> dict:
    """One item: dict(E (3, 3), F (3, 3), inliers (n,) uint8, record (RECORD_DTYPE scalar), count (max_iters, 10))"""
    src, dst = np.ascontiguousarray(src, F64), np.ascontiguousarray(dst, F64)
    subsets = np.asarray(subsets, np.int32).reshape(-1, 5)
    n, max_iters = src.shape[0], subsets.shape[0]
    sol = solve(src, dst, subsets, camera)
    count = counts(src, dst, sol["models"], sol["valid"], threshold, camera)
    bi, bs, ran, valid, g = choose(count, need_table(n, confidence, max_iters))
    rec = np.zeros((), RECORD_DTYPE)
    rec["best_iter"], rec["best_slot"], rec["iters_run"], rec["valid"] = bi, bs, ran, valid
    if bi < 0:
        return dict(E=np.zeros((3, 3)), F=np.zeros((3, 3)), inliers=np.zeros(n, np.uint8), record=rec, count=count)
    E = sol["models"][bi, bs]
    err = pair_errors(E, src, dst, camera)
    inl = err <= threshold2(threshold, camera)
    rec["ok"], rec["inliers"] = 1, g
    rec["sq_error"] = np.cumsum(np.where(inl, err, 0.0))[-1]           # left to right, one accumulator
    return dict(E=E.reshape(3, 3).copy(), F=pixel_F(E, camera), inliers=inl.astype(np.uint8), record=rec, count=count)


def find(src, dst, subsets, threshold=1.0, confidence=0.999, camera=CAMERA) -> dict:
    """A batch: src, dst (B, n, 2), subsets (B, max_iters, 5) -> dict(E, F (B, 3, 3), inliers (B, n) uint8, records (B,) RECORD_DTYPE)"""
    src, dst, subsets = np.asarray(src, F64), np.asarray(dst, F64), np.asarray(subsets, np.int32)
    items = [find_one(s, d, t, threshold, confidence, camera) for s, d, t in zip(src, dst, subsets)]
    return dict(E=np.stack([i["E"] for i in items]), F=np.stack([i["F"] for i in items]), inliers=np.stack([i["inliers"] for i in items]),
                records=np.array([i["record"] for i in items], RECORD_DTYPE))
