"""An independent float64 five-point solver, to hold tests/essential_ref.py to the definition (tests/test_essential_ref_cpu.py): the null
space from numpy.linalg.svd, the ten cubics from polynomial arithmetic on dictionaries of exponents, the reduction by numpy.linalg.solve,
det B(z) by numpy's polynomial products, its roots from numpy.roots, and (x, y) from the null vector of B(z) by another SVD.  It shares
no code and no table with the restatement, and no operation order."""
import numpy as np

NAMES = "x3 y3 x2y xy2 x2z x2 y2z y2 xyz xy xz2 xz x yz2 yz y z3 z2 z 1".split()


def _exponents(name):
    e = [0, 0, 0]
    k = 0
    while k < len(name) and name != "1":
        v = "xyz".index(name[k])
        k += 1
        p = 1
        if k < len(name) and name[k].isdigit():
            p = int(name[k])
            k += 1
        e[v] += p
    return tuple(e)


ORDER = [_exponents(n) for n in NAMES]


def _mul(a, b):
    out = {}
    for ea, ca in a.items():
        for eb, cb in b.items():
            e = (ea[0] + eb[0], ea[1] + eb[1], ea[2] + eb[2])
            out[e] = out.get(e, 0.0) + ca * cb
    return out


def _add(a, b, s=1.0):
    out = dict(a)
    for e, c in b.items():
        out[e] = out.get(e, 0.0) + s * c
    return out


def null_space(x, y, X, Y):
    """four null vectors (4, 9) of the 5 x 9 system of normalised pairs"""
    A = np.stack([X * x, X * y, X, Y * x, Y * y, Y, x, y, np.ones(5)], 1)
    return np.linalg.svd(A)[2][5:]


def cubic_matrix(nv):
    """the 10 x 20 matrix of det E = 0 and 2 E E^T E - tr(E E^T) E = 0 in Nister's monomial order"""
    E = [[{(1, 0, 0): nv[0][3 * r + c], (0, 1, 0): nv[1][3 * r + c], (0, 0, 1): nv[2][3 * r + c], (0, 0, 0): nv[3][3 * r + c]} for c in range(3)]
         for r in range(3)]
    det = _add(_add(_mul(E[0][0], _add(_mul(E[1][1], E[2][2]), _mul(E[1][2], E[2][1]), -1.0)),
                    _mul(E[0][1], _add(_mul(E[1][0], E[2][2]), _mul(E[1][2], E[2][0]), -1.0)), -1.0),
               _mul(E[0][2], _add(_mul(E[1][0], E[2][1]), _mul(E[1][1], E[2][0]), -1.0)))
    EEt = [[_add(_add(_mul(E[i][0], E[j][0]), _mul(E[i][1], E[j][1])), _mul(E[i][2], E[j][2])) for j in range(3)] for i in range(3)]
    tr = _add(_add(EEt[0][0], EEt[1][1]), EEt[2][2])
    rows = [det]
    for i in range(3):
        for j in range(3):
            eee = _add(_add(_mul(EEt[i][0], E[0][j]), _mul(EEt[i][1], E[1][j])), _mul(EEt[i][2], E[2][j]))
            rows.append(_add({e: 2.0 * c for e, c in eee.items()}, _mul(tr, E[i][j]), -1.0))
    return np.array([[r.get(e, 0.0) for e in ORDER] for r in rows])


def z_polynomial(M):
    """(det B(z) as numpy's descending coefficients (11), B as a 3 x 3 list of numpy polynomials)"""
    G = np.linalg.solve(M[:, :10], M[:, 10:])
    B = []
    for q in range(3):
        e, f = G[4 + 2 * q], G[5 + 2 * q]
        row = []
        for o, d in ((0, 3), (3, 3), (6, 4)):              # the coefficients of x, of y, and the constant: columns xz2 xz x | yz2 yz y | z3 z2 z 1
            pe = np.poly1d(e[o:o + d])
            pf = np.poly1d(np.append(f[o:o + d], 0.0))    # z * f
            row.append(pe - pf)
        B.append(row)
    det = (B[0][0] * (B[1][1] * B[2][2] - B[1][2] * B[2][1]) - B[0][1] * (B[1][0] * B[2][2] - B[1][2] * B[2][0])
           + B[0][2] * (B[1][0] * B[2][1] - B[1][1] * B[2][0]))
    return det.coeffs, B


def solve(x, y, X, Y):
    """the models of five normalised pairs: (list of (9,) arrays of unit Frobenius norm, all roots of det B as numpy.roots returns them)"""
    nv = null_space(x, y, X, Y)
    coeffs, B = z_polynomial(cubic_matrix(nv))
    roots = np.roots(coeffs)
    out = []
    for z in roots[np.imag(roots) == 0].real:
        Bz = np.array([[p(z) for p in row] for row in B])
        v = np.linalg.svd(Bz)[2][2]
        if v[2] == 0.0:
            continue
        xx, yy = v[0] / v[2], v[1] / v[2]
        E = xx * nv[0] + yy * nv[1] + z * nv[2] + nv[3]
        out.append(E / np.sqrt((E * E).sum()))
    return out, roots


def residuals(E, x, y, X, Y):
    """(|det E|, the largest |entry| of 2 E E^T E - tr(E E^T) E, the largest |X^T E x| over the pairs) of a unit-norm E"""
    E = np.asarray(E, np.float64).reshape(3, 3)
    T = 2.0 * E @ E.T @ E - np.trace(E @ E.T) * E
    fit = np.abs(np.einsum("ki,ij,kj->k", np.stack([X, Y, np.ones_like(X)], 1), E, np.stack([x, y, np.ones_like(x)], 1)))
    return abs(np.linalg.det(E)), np.abs(T).max(), fit.max()
