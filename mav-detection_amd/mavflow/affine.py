"""A robust 2-D affine fit on the device (include/mavflow_affine.h): the ctypes binding as methods of _lib.Context (estimate_affine,
flow_affine, estimate_affine_enqueue, flow_affine_enqueue, estimate_affine_workspace_bytes), the draw of the sample triples, and
`estimateAffine2D` with cv2's literal signature and return shapes.  The library is _lib's (same loader, no CPU fallback); the entry points
here are not in _lib.EXPORTS, which lists include/mavflow.h alone.

The algorithm is cv2.estimateAffine2D's RANSAC with the CALLER's sample triples: cv2 draws them from a private generator, so no
implementation can equal its draw.  With triples=None they are drawn here (sample_triples) from the caller's rng; the draw and its order
are documented there and pinned to nothing.  Everything after the draw is deterministic on the device."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import Context, _dev_ptr, _ptr, check

# every symbol include/mavflow_affine.h declares (tests check the library exports each of them)
EXPORTS = ("mav_affine_defaults", "mav_estimate_affine_workspace_bytes", "mav_estimate_affine", "mav_estimate_affine_dev", "mav_flow_affine",
           "mav_flow_affine_dev")

AFFINE_MAX_PAIRS, AFFINE_MAX_ITERS, AFFINE_RANK_RATIO = 65536, 4096, 1e-12
# cv2's constants, for `estimateAffine2D` below
LMEDS, RANSAC = 4, 8


class AffineParams(C.Structure):
    """mav_affine_params"""
    _fields_ = [("threshold", C.c_double), ("confidence", C.c_double), ("max_iters", C.c_int32), ("refine", C.c_int32), ("flags", C.c_int32),
                ("pad", C.c_int32)]


class AffineRecord(C.Structure):
    """mav_affine_record"""
    _fields_ = [("ok", C.c_int32), ("inliers", C.c_int32), ("best_iter", C.c_int32), ("iters_run", C.c_int32), ("valid", C.c_int32),
                ("refined", C.c_int32), ("sq_error", C.c_double)]


RECORD_DTYPE = np.dtype([("ok", np.int32), ("inliers", np.int32), ("best_iter", np.int32), ("iters_run", np.int32), ("valid", np.int32),
                         ("refined", np.int32), ("sq_error", np.float64)])
RECORD_FIELDS = ("inliers_count", "best_iter", "iters_run", "valid", "refined", "sq_error")
assert C.sizeof(AffineParams) == 32
assert RECORD_DTYPE.itemsize == C.sizeof(AffineRecord) == 32

_ready = False


def load() -> C.CDLL:
    """_lib.load() with this header's prototypes attached."""
    global _ready
    lib = _lib.load()
    if not _ready:
        vp, i = C.c_void_p, C.c_int
        lib.mav_affine_defaults.restype, lib.mav_affine_defaults.argtypes = None, [vp]
        lib.mav_estimate_affine_workspace_bytes.restype, lib.mav_estimate_affine_workspace_bytes.argtypes = C.c_size_t, [i, i, vp]
        # ctx, src | flow, dst | coords, n, batch, params, triples, M, inliers, records (, pairs_dst | workspace, workspace_bytes)
        lib.mav_estimate_affine.restype, lib.mav_estimate_affine.argtypes = i, [vp, vp, vp, i, i, vp, vp, vp, vp, vp]
        lib.mav_flow_affine.restype, lib.mav_flow_affine.argtypes = i, [vp, vp, vp, i, i, vp, vp, vp, vp, vp, vp]
        for name in ("mav_estimate_affine_dev", "mav_flow_affine_dev"):
            getattr(lib, name).restype, getattr(lib, name).argtypes = i, [vp, vp, vp, i, i, vp, vp, vp, vp, vp, vp, C.c_size_t]
        _ready = True
    return lib


def affine_params(threshold=3.0, max_iters=2000, confidence=0.99, refine=True) -> AffineParams:
    """The library's defaults with these fields."""
    p = AffineParams()
    load().mav_affine_defaults(C.byref(p))
    p.threshold, p.max_iters, p.confidence, p.refine = float(threshold), int(max_iters), float(confidence), int(bool(refine))
    return p


def _generator(rng):
    """np.random (the module), a Generator, a RandomState, a seed, or None (a fresh unseeded Generator): an object with .random(n)"""
    if rng is None:
        return np.random.default_rng()
    if hasattr(rng, "random"):
        return rng
    return np.random.default_rng(rng)


def sample_triples(rng, n: int, max_iters: int, batch: int = 1) -> np.ndarray:
    """(batch, max_iters, 3) int32 triples of distinct indices in [0, n), n >= 3, from ONE call rng.random(batch * max_iters * 3),
    consumed item by item, hypothesis by hypothesis, index by index (u0, u1, u2):
        i0 = floor(u0 * n);   i1 = floor(u1 * (n - 1)), moved past i0 (i1 += 1 when i1 >= i0);
        i2 = floor(u2 * (n - 2)), moved past both in ascending order (i2 += 1 when i2 >= min(i0, i1); then i2 += 1 when i2 >= max(i0, i1)).
    Always distinct, no rejection loop, a fixed consumption.  rng: np.random, a Generator, a RandomState or a seed."""
    n, max_iters, batch = int(n), int(max_iters), int(batch)
    if n < 3:
        raise ValueError(f"sample_triples: n = {n} is less than 3")
    u = np.asarray(_generator(rng).random(batch * max_iters * 3), np.float64).reshape(batch, max_iters, 3)
    i0 = np.minimum(np.floor(u[..., 0] * n).astype(np.int64), n - 1)
    i1 = np.minimum(np.floor(u[..., 1] * (n - 1)).astype(np.int64), n - 2)
    i2 = np.minimum(np.floor(u[..., 2] * (n - 2)).astype(np.int64), n - 3)
    i1 = i1 + (i1 >= i0)
    lo, hi = np.minimum(i0, i1), np.maximum(i0, i1)
    i2 = i2 + (i2 >= lo)
    i2 = i2 + (i2 >= hi)
    return np.ascontiguousarray(np.stack([i0, i1, i2], axis=-1).astype(np.int32))


def _on_device(ctx, a) -> bool:
    return hasattr(a, "ptr") and getattr(a, "on_device", True) and getattr(a, "ctx", ctx) is ctx


def _triples_for(triples, rng, n, max_iters, B):
    if triples is None:
        return sample_triples(rng, n, max_iters, B)
    t = np.asarray(triples)
    if t.ndim == 2:
        t = np.broadcast_to(t, (B,) + t.shape)
    if t.ndim != 3 or t.shape[0] != B or t.shape[2] != 3 or not np.issubdtype(t.dtype, np.integer):
        raise ValueError(f"triples: expected (max_iters, 3) or ({B}, max_iters, 3) integers, got {t.dtype} {t.shape}")
    return np.ascontiguousarray(t, dtype=np.int32)


def _result(M, inl, rec, single) -> dict:
    out = dict(M=M, ok=rec["ok"].copy(), inliers=inl, inliers_count=rec["inliers"].copy(), best_iter=rec["best_iter"].copy(),
               iters_run=rec["iters_run"].copy(), valid=rec["valid"].copy(), refined=rec["refined"].copy(), sq_error=rec["sq_error"].copy(),
               records=rec)
    if single:
        out = {k: v[0] for k, v in out.items()}
        for k in ("ok",) + RECORD_FIELDS:
            out[k] = out[k].item()
    return out


def _estimate_affine(self, src, dst, threshold=3.0, max_iters=2000, confidence=0.99, refine=True, triples=None, rng=None) -> dict:
    """The RANSAC affine fit of include/mavflow_affine.h for pairs src -> dst, (n, 2) or a batch (B, n, 2), float64 (x, y).  triples:
    (max_iters, 3) or (B, max_iters, 3) integer sample triples (max_iters is then their count); None: drawn by sample_triples with rng
    (np.random, a Generator or a seed).  Returns a dict: M (2, 3) float64, ok, inliers (n,) uint8 (the best minimal model's),
    inliers_count, best_iter, iters_run, valid, refined, sq_error, records (RECORD_DTYPE); with a leading B for a batch.  ok == 0: no
    valid hypothesis had more than two inliers; M and the mask are zero."""
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    single = src.ndim == 2
    if single:
        src, dst = src[None], dst[None]
    if src.ndim != 3 or src.shape[2] != 2 or src.shape != dst.shape:
        raise ValueError(f"estimate_affine: expected two (n, 2) or (batch, n, 2) arrays, got {src.shape} and {dst.shape}")
    B, n = src.shape[:2]
    src, dst = np.ascontiguousarray(src), np.ascontiguousarray(dst)
    triples = _triples_for(triples, rng, n, max_iters, B)
    p = affine_params(threshold, triples.shape[1], confidence, refine)
    M, inl, rec = np.empty((B, 2, 3), np.float64), np.empty((B, n), np.uint8), np.zeros(B, RECORD_DTYPE)
    check(load().mav_estimate_affine(self.h, _ptr(src), _ptr(dst), n, B, C.byref(p), _ptr(triples), _ptr(M), _ptr(inl), _ptr(rec)))
    return _result(M, inl, rec, single)


def _flow_affine(self, flow, coords, threshold=3.0, max_iters=2000, confidence=0.99, refine=True, triples=None, rng=None, want_pairs=False) -> dict:
    """estimate_affine on the pairs coords -> coords + flow[y, x] (detector.py:126-128) of float32 fields (H, W, 2) or (B, H, W, 2), or
    of a device handle of this context (pipeline.DeviceArray or any object with .ptr and .shape): read where it is.  coords: (n, 2)
    integers (x, y) inside the frame.  With want_pairs the dict also has pairs_dst (B, n, 2) float64 (host fields only)."""
    lib = load()
    coords = self._coords(coords)
    n = coords.shape[0]
    dev = _on_device(self, flow)
    if dev:
        if getattr(flow, "_deferred", None) is not None:
            flow._deferred.flush()
        shape = tuple(flow.shape)
    else:
        flow = np.asarray(flow)
        shape = flow.shape
    single = len(shape) == 3
    B = 1 if single else shape[0]
    triples = _triples_for(triples, rng, n, max_iters, B)
    p = affine_params(threshold, triples.shape[1], confidence, refine)
    M, inl, rec = np.empty((B, 2, 3), np.float64), np.empty((B, n), np.uint8), np.zeros(B, RECORD_DTYPE)
    pairs = None
    if not dev:
        flow = self._flows(flow[None] if single else flow, B, "flow")
        pairs = np.empty((B, n, 2), np.float64) if want_pairs else None
        check(lib.mav_flow_affine(self.h, _ptr(flow), _ptr(coords), n, B, C.byref(p), _ptr(triples), _ptr(M), _ptr(inl), _ptr(rec), _ptr(pairs)))
    else:
        if want_pairs:
            raise ValueError("flow_affine: want_pairs needs a host field")
        need = int(lib.mav_estimate_affine_workspace_bytes(n, B, C.byref(p)))
        bufs = []
        try:
            for nbytes in (triples.nbytes, M.nbytes, inl.nbytes, rec.nbytes, need):
                bufs.append(self.alloc(max(nbytes, 1)))
            dt, dM, di, dr, dw = bufs
            dt.upload(triples)
            check(lib.mav_flow_affine_dev(self.h, _dev_ptr(flow), _ptr(coords), n, B, C.byref(p), dt.ptr, dM.ptr, di.ptr, dr.ptr, dw.ptr, need))
            M, inl, rec = dM.download(np.float64, (B, 2, 3)), di.download(np.uint8, (B, n)), dr.download(RECORD_DTYPE, (B,))
        finally:
            for b in bufs:
                b.free()
    out = _result(M, inl, rec, single)
    if pairs is not None:
        out["pairs_dst"] = pairs[0] if single else pairs
    return out


def _estimate_affine_workspace_bytes(self, n: int, batch: int = 1, max_iters: int = 2000) -> int:
    """mav_estimate_affine_workspace_bytes: what estimate_affine_enqueue and flow_affine_enqueue need (a function of n, batch, max_iters)."""
    p = affine_params(max_iters=max_iters)
    need = load().mav_estimate_affine_workspace_bytes(int(n), int(batch), C.byref(p))
    if not need:
        raise _lib.MavflowError(load().mav_last_error().decode())
    return int(need)


def _estimate_affine_enqueue(self, src_ptr, dst_ptr, n: int, batch: int, triples_ptr, M_ptr, inliers_ptr, records_ptr, workspace_ptr,
                             workspace_bytes: int, threshold=3.0, max_iters=2000, confidence=0.99, refine=True) -> None:
    """mav_estimate_affine_dev: enqueue only, device pointers (ints, or objects with a .ptr): src, dst (batch, n, 2) float64, triples
    (batch, max_iters, 3) int32, M (batch, 2, 3) float64, inliers (batch, n) uint8, records: `batch` RECORD_DTYPE blocks aligned to 16, a
    workspace of estimate_affine_workspace_bytes(...) aligned to 16.  A triple that is out of range or repeats an index is an invalid
    hypothesis."""
    p = affine_params(threshold, max_iters, confidence, refine)
    check(load().mav_estimate_affine_dev(self.h, _dev_ptr(src_ptr), _dev_ptr(dst_ptr), int(n), int(batch), C.byref(p), _dev_ptr(triples_ptr),
                                         _dev_ptr(M_ptr), _dev_ptr(inliers_ptr), _dev_ptr(records_ptr), _dev_ptr(workspace_ptr), int(workspace_bytes)))


def _flow_affine_enqueue(self, flow_ptr, coords, batch: int, triples_ptr, M_ptr, inliers_ptr, records_ptr, workspace_ptr, workspace_bytes: int,
                         threshold=3.0, max_iters=2000, confidence=0.99, refine=True) -> None:
    """mav_flow_affine_dev: enqueue only; flow (batch, H, W, 2) float32 on the device, coords (n, 2) integers on the HOST (range-checked and
    copied with the call), the rest as estimate_affine_enqueue.  The gathered pairs stay in the workspace."""
    coords = self._coords(coords)
    p = affine_params(threshold, max_iters, confidence, refine)
    check(load().mav_flow_affine_dev(self.h, _dev_ptr(flow_ptr), _ptr(coords), coords.shape[0], int(batch), C.byref(p), _dev_ptr(triples_ptr),
                                     _dev_ptr(M_ptr), _dev_ptr(inliers_ptr), _dev_ptr(records_ptr), _dev_ptr(workspace_ptr), int(workspace_bytes)))


Context.estimate_affine = _estimate_affine
Context.flow_affine = _flow_affine
Context.estimate_affine_workspace_bytes = _estimate_affine_workspace_bytes
Context.estimate_affine_enqueue = _estimate_affine_enqueue
Context.flow_affine_enqueue = _flow_affine_enqueue


def estimateAffine2D(from_, to, inliers=None, method=RANSAC, ransacReprojThreshold=3, maxIters=2000, confidence=0.99, refineIters=10, rng=None):
    """cv2.estimateAffine2D's signature and return shapes: (M (2, 3) float64 or None, inliers (n, 1) uint8) for point sets (n, 2) or
    (n, 1, 2) of any real dtype.  method: RANSAC only -- the sample triples are drawn by sample_triples from rng (np.random, a Generator or
    a seed; None: a fresh unseeded Generator), NOT from OpenCV's private generator, so a run equals no cv2 run sample for sample; LMEDS
    raises NotImplementedError.  refineIters == 0 turns the refinement off; any other value asks for the exact least-squares refinement
    (the minimiser cv2's Levenberg-Marquardt iterates towards).  `inliers` is accepted and ignored, as an output argument."""
    if int(method) == LMEDS:
        raise NotImplementedError("LMEDS is not reproduced; method must be RANSAC")
    if int(method) != RANSAC:
        raise ValueError(f"estimateAffine2D: method {method} is neither RANSAC nor LMEDS")
    a, b = np.asarray(from_, np.float64).reshape(-1, 2), np.asarray(to, np.float64).reshape(-1, 2)
    from . import im_helpers
    ctx = im_helpers._ctx(1024, 16)
    out = ctx.estimate_affine(a, b, threshold=ransacReprojThreshold, max_iters=maxIters, confidence=confidence, refine=int(refineIters) != 0, rng=rng)
    return (out["M"] if out["ok"] else None), out["inliers"].reshape(-1, 1)
