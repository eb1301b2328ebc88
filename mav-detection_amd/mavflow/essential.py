"""A robust essential-matrix fit on the device (include/mavflow_essential.h): the ctypes binding as methods of _lib.Context
(find_essential, flow_essential, their *_enqueue twins, find_essential_workspace_bytes), the draw of the sample subsets, and
`findEssentialMat` / `decomposeEssentialMat` with cv2's signatures and return shapes.  The library is _lib's (same loader, no CPU
fallback); the entry points here are not in _lib.EXPORTS, which lists include/mavflow.h alone.

The algorithm is the RANSAC frame of cv2.findEssentialMat with the CALLER's sample subsets and Nister's five-point solver in place of
OpenCV's (the header lists what to re-check against a cv2 build).  With subsets=None they are drawn here (sample_subsets) from the
caller's rng.  Everything after the draw is deterministic on the device.  decomposeEssentialMat runs on the host; it is unpinned against
cv2: the order of R1 and R2 and the sign of t may differ from a cv2 build's."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import Context, _dev_ptr, _ptr, check
from .affine import _generator
from .fundamental import _flow_shape

# every symbol include/mavflow_essential.h declares (tests check the library exports each of them)
EXPORTS = ("mav_essential_defaults", "mav_find_essential_workspace_bytes", "mav_find_essential", "mav_find_essential_dev",
           "mav_flow_essential", "mav_flow_essential_dev")

ESSENTIAL_MAX_PAIRS, ESSENTIAL_MAX_ITERS = 65536, 4096
# cv2's constants, for `findEssentialMat` below
LMEDS, RANSAC = 4, 8


class EssentialParams(C.Structure):
    """mav_essential_params"""
    _fields_ = [("threshold", C.c_double), ("confidence", C.c_double), ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double),
                ("cy", C.c_double), ("max_iters", C.c_int32), ("flags", C.c_int32)]


class EssentialRecord(C.Structure):
    """mav_essential_record"""
    _fields_ = [("ok", C.c_int32), ("inliers", C.c_int32), ("best_iter", C.c_int32), ("best_slot", C.c_int32), ("iters_run", C.c_int32),
                ("valid", C.c_int32), ("sq_error", C.c_double)]


RECORD_DTYPE = np.dtype([("ok", np.int32), ("inliers", np.int32), ("best_iter", np.int32), ("best_slot", np.int32), ("iters_run", np.int32),
                         ("valid", np.int32), ("sq_error", np.float64)])
RECORD_FIELDS = ("inliers_count", "best_iter", "best_slot", "iters_run", "valid", "sq_error")
assert C.sizeof(EssentialParams) == 56
assert RECORD_DTYPE.itemsize == C.sizeof(EssentialRecord) == 32

_ready = False


def load() -> C.CDLL:
    """_lib.load() with this header's prototypes attached."""
    global _ready
    lib = _lib.load()
    if not _ready:
        vp, i = C.c_void_p, C.c_int
        lib.mav_essential_defaults.restype, lib.mav_essential_defaults.argtypes = None, [vp]
        lib.mav_find_essential_workspace_bytes.restype, lib.mav_find_essential_workspace_bytes.argtypes = C.c_size_t, [i, i, vp]
        # ctx, src | flow, dst | coords, n, batch, params, subsets, E, F, inliers, records (, pairs_dst | workspace, workspace_bytes)
        lib.mav_find_essential.restype, lib.mav_find_essential.argtypes = i, [vp, vp, vp, i, i, vp, vp, vp, vp, vp, vp]
        lib.mav_flow_essential.restype, lib.mav_flow_essential.argtypes = i, [vp, vp, vp, i, i, vp, vp, vp, vp, vp, vp, vp]
        for name in ("mav_find_essential_dev", "mav_flow_essential_dev"):
            getattr(lib, name).restype, getattr(lib, name).argtypes = i, [vp, vp, vp, i, i, vp, vp, vp, vp, vp, vp, vp, C.c_size_t]
        _ready = True
    return lib


def camera_of(focal=1.0, pp=(0.0, 0.0)):
    """(fx, fy, cx, cy) of cv2's (focal, pp) arguments, or of a 3 x 3 camera matrix in `focal`'s place"""
    K = np.asarray(focal, np.float64)
    if K.shape == (3, 3):
        return float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
    if K.shape != ():
        raise ValueError(f"camera: expected a focal length or a 3 x 3 camera matrix, got an array of shape {K.shape}")
    return float(K), float(K), float(pp[0]), float(pp[1])


def essential_params(threshold=1.0, confidence=0.999, max_iters=1000, camera=(1.0, 1.0, 0.0, 0.0)) -> EssentialParams:
    """The library's defaults with these fields; camera = (fx, fy, cx, cy)."""
    p = EssentialParams()
    load().mav_essential_defaults(C.byref(p))
    p.threshold, p.confidence, p.max_iters = float(threshold), float(confidence), int(max_iters)
    p.fx, p.fy, p.cx, p.cy = (float(v) for v in camera)
    return p


def sample_subsets(rng, n: int, max_iters: int, batch: int = 1) -> np.ndarray:
    """(batch, max_iters, 5) int32 subsets of distinct indices in [0, n), n >= 5, from ONE call rng.random(batch * max_iters * 5),
    consumed item by item, hypothesis by hypothesis, index by index (u0 .. u4):  i_j = floor(u_j * (n - j)), moved past the earlier picks
    in ascending order (for each earlier pick p, smallest first: i_j += 1 when i_j >= p) -- fundamental.sample_subsets' scheme.  Always
    distinct, no rejection loop, a fixed consumption.  rng: np.random, a Generator, a RandomState or a seed."""
    n, max_iters, batch = int(n), int(max_iters), int(batch)
    if n < 5:
        raise ValueError(f"sample_subsets: n = {n} is less than 5")
    u = np.asarray(_generator(rng).random(batch * max_iters * 5), np.float64).reshape(batch, max_iters, 5)
    picks = np.empty((batch, max_iters, 5), np.int64)
    for j in range(5):
        i = np.minimum(np.floor(u[..., j] * (n - j)).astype(np.int64), n - j - 1)
        earlier = np.sort(picks[..., :j], axis=-1)
        for q in range(j):
            i = i + (i >= earlier[..., q])
        picks[..., j] = i
    return np.ascontiguousarray(picks.astype(np.int32))


def _subsets_for(subsets, rng, n, max_iters, B):
    if subsets is None:
        return sample_subsets(rng, n, max_iters, B)
    t = np.asarray(subsets)
    if t.ndim == 2:
        t = np.broadcast_to(t, (B,) + t.shape)
    if t.ndim != 3 or t.shape[0] != B or t.shape[2] != 5 or not np.issubdtype(t.dtype, np.integer):
        raise ValueError(f"subsets: expected (max_iters, 5) or ({B}, max_iters, 5) integers, got {t.dtype} {t.shape}")
    return np.ascontiguousarray(t, dtype=np.int32)


def _result(E, F, inl, rec, single) -> dict:
    out = dict(E=E, F=F, ok=rec["ok"].copy(), inliers=inl, inliers_count=rec["inliers"].copy(), best_iter=rec["best_iter"].copy(),
               best_slot=rec["best_slot"].copy(), iters_run=rec["iters_run"].copy(), valid=rec["valid"].copy(), sq_error=rec["sq_error"].copy(),
               records=rec)
    if single:
        out = {k: v[0] for k, v in out.items()}
        for k in ("ok",) + RECORD_FIELDS:
            out[k] = out[k].item()
    return out


def _find_essential(self, src, dst, threshold=1.0, confidence=0.999, max_iters=1000, subsets=None, rng=None, camera=(1.0, 1.0, 0.0, 0.0)) -> dict:
    """The RANSAC essential-matrix fit of include/mavflow_essential.h for pixel pairs src -> dst, (n, 2) or a batch (B, n, 2), float64
    (x, y), n >= 5, under camera = (fx, fy, cx, cy).  subsets: (max_iters, 5) or (B, max_iters, 5) integer sample subsets (max_iters is
    then their count); None: drawn by sample_subsets with rng.  Returns a dict: E (3, 3) float64 of unit Frobenius norm (the best minimal
    model, normalised coordinates), F (3, 3) = K^-T E K^-1 of unit norm (pixel coordinates, what epipolar_residual takes), ok, inliers
    (n,) uint8, inliers_count, best_iter, best_slot, iters_run, valid, sq_error, records (RECORD_DTYPE); with a leading B for a batch.
    ok == 0: no valid model had more than four inliers; E, F and the mask are zero."""
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    single = src.ndim == 2
    if single:
        src, dst = src[None], dst[None]
    if src.ndim != 3 or src.shape[2] != 2 or src.shape != dst.shape:
        raise ValueError(f"find_essential: expected two (n, 2) or (batch, n, 2) arrays, got {src.shape} and {dst.shape}")
    B, n = src.shape[:2]
    src, dst = np.ascontiguousarray(src), np.ascontiguousarray(dst)
    subsets = _subsets_for(subsets, rng, n, max_iters, B)
    p = essential_params(threshold, confidence, subsets.shape[1], camera)
    E, F, inl, rec = np.empty((B, 3, 3), np.float64), np.empty((B, 3, 3), np.float64), np.empty((B, n), np.uint8), np.zeros(B, RECORD_DTYPE)
    check(load().mav_find_essential(self.h, _ptr(src), _ptr(dst), n, B, C.byref(p), _ptr(subsets), _ptr(E), _ptr(F), _ptr(inl), _ptr(rec)))
    return _result(E, F, inl, rec, single)


def _flow_essential(self, flow, coords, threshold=1.0, confidence=0.999, max_iters=1000, subsets=None, rng=None, camera=(1.0, 1.0, 0.0, 0.0),
                    want_pairs=False) -> dict:
    """find_essential on the pairs coords -> coords + flow[y, x] (detector.py:126-128) of float32 fields (H, W, 2) or (B, H, W, 2), or
    of a device handle of this context (pipeline.DeviceArray or any object with .ptr and .shape): read where it is.  coords: (n, 2)
    integers (x, y) inside the frame.  With want_pairs the dict also has pairs_dst (B, n, 2) float64 (host fields only)."""
    lib = load()
    coords = self._coords(coords)
    n = coords.shape[0]
    dev, flow, shape = _flow_shape(self, flow)
    single = len(shape) == 3
    B = 1 if single else shape[0]
    subsets = _subsets_for(subsets, rng, n, max_iters, B)
    p = essential_params(threshold, confidence, subsets.shape[1], camera)
    E, F, inl, rec = np.empty((B, 3, 3), np.float64), np.empty((B, 3, 3), np.float64), np.empty((B, n), np.uint8), np.zeros(B, RECORD_DTYPE)
    pairs = None
    if not dev:
        flow = self._flows(flow[None] if single else flow, B, "flow")
        pairs = np.empty((B, n, 2), np.float64) if want_pairs else None
        check(lib.mav_flow_essential(self.h, _ptr(flow), _ptr(coords), n, B, C.byref(p), _ptr(subsets), _ptr(E), _ptr(F), _ptr(inl), _ptr(rec),
                                     _ptr(pairs)))
    else:
        if want_pairs:
            raise ValueError("flow_essential: want_pairs needs a host field")
        need = int(lib.mav_find_essential_workspace_bytes(n, B, C.byref(p)))
        bufs = []
        try:
            for nbytes in (subsets.nbytes, E.nbytes, F.nbytes, inl.nbytes, rec.nbytes, need):
                bufs.append(self.alloc(max(nbytes, 1)))
            dt, dE, dF, di, dr, dw = bufs
            dt.upload(subsets)
            check(lib.mav_flow_essential_dev(self.h, _dev_ptr(flow), _ptr(coords), n, B, C.byref(p), dt.ptr, dE.ptr, dF.ptr, di.ptr, dr.ptr, dw.ptr,
                                             need))
            E, F = dE.download(np.float64, (B, 3, 3)), dF.download(np.float64, (B, 3, 3))
            inl, rec = di.download(np.uint8, (B, n)), dr.download(RECORD_DTYPE, (B,))
        finally:
            for b in bufs:
                b.free()
    out = _result(E, F, inl, rec, single)
    if pairs is not None:
        out["pairs_dst"] = pairs[0] if single else pairs
    return out


def _find_essential_workspace_bytes(self, n: int, batch: int = 1, max_iters: int = 1000) -> int:
    """mav_find_essential_workspace_bytes: what find_essential_enqueue and flow_essential_enqueue need (a function of n, batch,
    max_iters)."""
    p = essential_params(max_iters=max_iters)
    need = load().mav_find_essential_workspace_bytes(int(n), int(batch), C.byref(p))
    if not need:
        raise _lib.MavflowError(load().mav_last_error().decode())
    return int(need)


def _find_essential_enqueue(self, src_ptr, dst_ptr, n: int, batch: int, subsets_ptr, E_ptr, F_ptr, inliers_ptr, records_ptr, workspace_ptr,
                            workspace_bytes: int, threshold=1.0, confidence=0.999, max_iters=1000, camera=(1.0, 1.0, 0.0, 0.0)) -> None:
    """mav_find_essential_dev: enqueue only, device pointers (ints, or objects with a .ptr): src, dst (batch, n, 2) float64, subsets
    (batch, max_iters, 5) int32, E and F (batch, 3, 3) float64, inliers (batch, n) uint8, records: `batch` RECORD_DTYPE blocks aligned to
    16, a workspace of find_essential_workspace_bytes(...) aligned to 16.  A subset that is out of range or repeats an index is an
    invalid hypothesis.  F is what epipolar_residual_enqueue reads."""
    p = essential_params(threshold, confidence, max_iters, camera)
    check(load().mav_find_essential_dev(self.h, _dev_ptr(src_ptr), _dev_ptr(dst_ptr), int(n), int(batch), C.byref(p), _dev_ptr(subsets_ptr),
                                        _dev_ptr(E_ptr), _dev_ptr(F_ptr), _dev_ptr(inliers_ptr), _dev_ptr(records_ptr), _dev_ptr(workspace_ptr),
                                        int(workspace_bytes)))


def _flow_essential_enqueue(self, flow_ptr, coords, batch: int, subsets_ptr, E_ptr, F_ptr, inliers_ptr, records_ptr, workspace_ptr,
                            workspace_bytes: int, threshold=1.0, confidence=0.999, max_iters=1000, camera=(1.0, 1.0, 0.0, 0.0)) -> None:
    """mav_flow_essential_dev: enqueue only; flow (batch, H, W, 2) float32 on the device, coords (n, 2) integers on the HOST
    (range-checked and copied with the call), the rest as find_essential_enqueue.  The gathered pairs stay in the workspace."""
    coords = self._coords(coords)
    p = essential_params(threshold, confidence, max_iters, camera)
    check(load().mav_flow_essential_dev(self.h, _dev_ptr(flow_ptr), _ptr(coords), coords.shape[0], int(batch), C.byref(p), _dev_ptr(subsets_ptr),
                                        _dev_ptr(E_ptr), _dev_ptr(F_ptr), _dev_ptr(inliers_ptr), _dev_ptr(records_ptr), _dev_ptr(workspace_ptr),
                                        int(workspace_bytes)))


Context.find_essential = _find_essential
Context.flow_essential = _flow_essential
Context.find_essential_workspace_bytes = _find_essential_workspace_bytes
Context.find_essential_enqueue = _find_essential_enqueue
Context.flow_essential_enqueue = _flow_essential_enqueue


def findEssentialMat(points1, points2, focal=1.0, pp=(0., 0.), method=RANSAC, prob=0.999, threshold=1.0, maxIters=1000, mask=None, rng=None):
    """cv2.findEssentialMat's second overload -- (points1, points2, focal, pp, method, prob, threshold, maxIters, mask) -- with its
    return shapes: (E (3, 3) float64 or None, mask (n, 1) uint8) for point sets (n, 2) or (n, 1, 2) of any real dtype.  A 3 x 3
    cameraMatrix is also accepted in the third position (cv2's first overload; pp is then ignored).  method: RANSAC only -- the sample
    subsets are drawn by sample_subsets from rng (np.random, a Generator or a seed; None: a fresh unseeded Generator), NOT from OpenCV's
    private generator, and the minimal solver is Nister's, not OpenCV's: a run equals no cv2 run sample for sample; LMEDS raises
    NotImplementedError.  E has unit Frobenius norm and its largest entry positive (cv2's scale and sign are its solver's).  n < 5 gives
    (None, zeros).  `mask` is accepted and ignored, as an output argument."""
    if int(method) != RANSAC:
        raise NotImplementedError(f"findEssentialMat: method {method} is not reproduced; method must be RANSAC")
    a, b = np.asarray(points1, np.float64).reshape(-1, 2), np.asarray(points2, np.float64).reshape(-1, 2)
    if a.shape != b.shape:
        raise ValueError(f"findEssentialMat: {a.shape[0]} and {b.shape[0]} points")
    n = a.shape[0]
    if n < 5:
        return None, np.zeros((n, 1), np.uint8)
    from . import im_helpers
    ctx = im_helpers._ctx(1024, 16)
    out = ctx.find_essential(a, b, threshold=threshold, confidence=prob, max_iters=maxIters, rng=rng, camera=camera_of(focal, pp))
    return (np.array(out["E"]) if out["ok"] else None), out["inliers"].reshape(-1, 1)


def decomposeEssentialMat(E):
    """cv2.decomposeEssentialMat's construction on the host: E = U diag(1, 1, 0) V^T by numpy.linalg.svd, U and V^T negated where their
    determinant is negative, W = [[0, 1, 0], [-1, 0, 0], [0, 0, 1]], R1 = U W V^T, R2 = U W^T V^T, t = U[:, 2] as (3, 1).  Both rotations
    have determinant +1, and [t]x R reproduces E up to sign and scale for either.  Unpinned against cv2: the order of R1 and R2 and the
    sign of t follow numpy's SVD, not OpenCV's, and may differ from a cv2 build's."""
    E = np.asarray(E, np.float64)
    if E.shape != (3, 3):
        raise ValueError(f"decomposeEssentialMat: expected a 3 x 3 matrix, got {E.shape}")
    U, _, Vt = np.linalg.svd(E)
    if np.linalg.det(U) < 0:
        U = -U
    if np.linalg.det(Vt) < 0:
        Vt = -Vt
    W = np.array([[0.0, 1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    return U @ W @ Vt, U @ W.T @ Vt, U[:, 2].reshape(3, 1).copy()
