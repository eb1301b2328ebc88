"""A robust fundamental-matrix fit and the dense epipolar residual on the device (include/mavflow_fundamental.h): the ctypes binding as
methods of _lib.Context (find_fundamental, flow_fundamental, epipolar_residual, their *_enqueue twins, find_fundamental_workspace_bytes),
the draw of the sample subsets, and `findFundamentalMat` with cv2's literal signature and return shapes.  The library is _lib's (same
loader, no CPU fallback); the entry points here are not in _lib.EXPORTS, which lists include/mavflow.h alone.

The algorithm is cv2.findFundamentalMat's FM_RANSAC with the CALLER's sample subsets: cv2 draws them from a private generator, so no
implementation can equal its draw.  With subsets=None they are drawn here (sample_subsets) from the caller's rng; the draw and its order
are documented there and pinned to nothing.  Everything after the draw is deterministic on the device."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import Context, _dev_ptr, _ptr, check
from .affine import _generator, _on_device

# every symbol include/mavflow_fundamental.h declares (tests check the library exports each of them)
EXPORTS = ("mav_fundamental_defaults", "mav_find_fundamental_workspace_bytes", "mav_find_fundamental", "mav_find_fundamental_dev",
           "mav_flow_fundamental", "mav_flow_fundamental_dev", "mav_epipolar_residual", "mav_epipolar_residual_dev")

FUNDAMENTAL_MAX_PAIRS, FUNDAMENTAL_MAX_ITERS = 65536, 4096
# cv2's constants, for `findFundamentalMat` below
FM_7POINT, FM_8POINT, FM_LMEDS, FM_RANSAC = 1, 2, 4, 8
DBL_EPSILON = float(np.finfo(np.float64).eps)


class FundamentalParams(C.Structure):
    """mav_fundamental_params"""
    _fields_ = [("threshold", C.c_double), ("confidence", C.c_double), ("max_iters", C.c_int32), ("flags", C.c_int32), ("pad", C.c_int32 * 2)]


class FundamentalRecord(C.Structure):
    """mav_fundamental_record"""
    _fields_ = [("ok", C.c_int32), ("inliers", C.c_int32), ("best_iter", C.c_int32), ("best_slot", C.c_int32), ("iters_run", C.c_int32),
                ("valid", C.c_int32), ("sq_error", C.c_double)]


class EpipolarRecord(C.Structure):
    """mav_epipolar_record"""
    _fields_ = [("max_residual", C.c_float), ("max_row", C.c_int32), ("max_col", C.c_int32), ("movers", C.c_int32), ("not_finite", C.c_int32),
                ("pad", C.c_int32 * 3)]


RECORD_DTYPE = np.dtype([("ok", np.int32), ("inliers", np.int32), ("best_iter", np.int32), ("best_slot", np.int32), ("iters_run", np.int32),
                         ("valid", np.int32), ("sq_error", np.float64)])
EPI_DTYPE = np.dtype([("max_residual", np.float32), ("max_row", np.int32), ("max_col", np.int32), ("movers", np.int32),
                      ("not_finite", np.int32), ("pad", np.int32, (3,))])
RECORD_FIELDS = ("inliers_count", "best_iter", "best_slot", "iters_run", "valid", "sq_error")
EPI_OUTPUTS = ("residual", "mask")
assert C.sizeof(FundamentalParams) == 32
assert RECORD_DTYPE.itemsize == C.sizeof(FundamentalRecord) == 32
assert EPI_DTYPE.itemsize == C.sizeof(EpipolarRecord) == 32

_ready = False


def load() -> C.CDLL:
    """_lib.load() with this header's prototypes attached."""
    global _ready
    lib = _lib.load()
    if not _ready:
        vp, i = C.c_void_p, C.c_int
        lib.mav_fundamental_defaults.restype, lib.mav_fundamental_defaults.argtypes = None, [vp]
        lib.mav_find_fundamental_workspace_bytes.restype, lib.mav_find_fundamental_workspace_bytes.argtypes = C.c_size_t, [i, i, vp]
        # ctx, src | flow, dst | coords, n, batch, params, subsets, F, inliers, records (, pairs_dst | workspace, workspace_bytes)
        lib.mav_find_fundamental.restype, lib.mav_find_fundamental.argtypes = i, [vp, vp, vp, i, i, vp, vp, vp, vp, vp]
        lib.mav_flow_fundamental.restype, lib.mav_flow_fundamental.argtypes = i, [vp, vp, vp, i, i, vp, vp, vp, vp, vp, vp]
        for name in ("mav_find_fundamental_dev", "mav_flow_fundamental_dev"):
            getattr(lib, name).restype, getattr(lib, name).argtypes = i, [vp, vp, vp, i, i, vp, vp, vp, vp, vp, vp, C.c_size_t]
        # ctx, flow, F, threshold, batch, residual, mask, records
        for name in ("mav_epipolar_residual", "mav_epipolar_residual_dev"):
            getattr(lib, name).restype, getattr(lib, name).argtypes = i, [vp, vp, vp, C.c_double, i, vp, vp, vp]
        _ready = True
    return lib


def fundamental_params(threshold=3.0, confidence=0.99, max_iters=1000) -> FundamentalParams:
    """The library's defaults with these fields."""
    p = FundamentalParams()
    load().mav_fundamental_defaults(C.byref(p))
    p.threshold, p.confidence, p.max_iters = float(threshold), float(confidence), int(max_iters)
    return p


def sample_subsets(rng, n: int, max_iters: int, batch: int = 1) -> np.ndarray:
    """(batch, max_iters, 7) int32 subsets of distinct indices in [0, n), n >= 7, from ONE call rng.random(batch * max_iters * 7),
    consumed item by item, hypothesis by hypothesis, index by index (u0 .. u6):  i_j = floor(u_j * (n - j)), moved past the earlier picks
    in ascending order (for each earlier pick p, smallest first: i_j += 1 when i_j >= p).  Always distinct, no rejection loop, a fixed
    consumption.  rng: np.random, a Generator, a RandomState or a seed (affine.sample_triples' conventions)."""
    n, max_iters, batch = int(n), int(max_iters), int(batch)
    if n < 7:
        raise ValueError(f"sample_subsets: n = {n} is less than 7")
    u = np.asarray(_generator(rng).random(batch * max_iters * 7), np.float64).reshape(batch, max_iters, 7)
    picks = np.empty((batch, max_iters, 7), np.int64)
    for j in range(7):
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
    if t.ndim != 3 or t.shape[0] != B or t.shape[2] != 7 or not np.issubdtype(t.dtype, np.integer):
        raise ValueError(f"subsets: expected (max_iters, 7) or ({B}, max_iters, 7) integers, got {t.dtype} {t.shape}")
    return np.ascontiguousarray(t, dtype=np.int32)


def _result(F, inl, rec, single) -> dict:
    out = dict(F=F, ok=rec["ok"].copy(), inliers=inl, inliers_count=rec["inliers"].copy(), best_iter=rec["best_iter"].copy(),
               best_slot=rec["best_slot"].copy(), iters_run=rec["iters_run"].copy(), valid=rec["valid"].copy(), sq_error=rec["sq_error"].copy(),
               records=rec)
    if single:
        out = {k: v[0] for k, v in out.items()}
        for k in ("ok",) + RECORD_FIELDS:
            out[k] = out[k].item()
    return out


def _find_fundamental(self, src, dst, threshold=3.0, confidence=0.99, max_iters=1000, subsets=None, rng=None) -> dict:
    """The RANSAC fundamental-matrix fit of include/mavflow_fundamental.h for pairs src -> dst, (n, 2) or a batch (B, n, 2), float64
    (x, y), n >= 7.  subsets: (max_iters, 7) or (B, max_iters, 7) integer sample subsets (max_iters is then their count); None: drawn by
    sample_subsets with rng (np.random, a Generator or a seed).  Returns a dict: F (3, 3) float64 of unit Frobenius norm (the best
    minimal model), ok, inliers (n,) uint8, inliers_count, best_iter, best_slot, iters_run, valid, sq_error, records (RECORD_DTYPE); with
    a leading B for a batch.  ok == 0: no valid model had more than six inliers; F and the mask are zero."""
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    single = src.ndim == 2
    if single:
        src, dst = src[None], dst[None]
    if src.ndim != 3 or src.shape[2] != 2 or src.shape != dst.shape:
        raise ValueError(f"find_fundamental: expected two (n, 2) or (batch, n, 2) arrays, got {src.shape} and {dst.shape}")
    B, n = src.shape[:2]
    src, dst = np.ascontiguousarray(src), np.ascontiguousarray(dst)
    subsets = _subsets_for(subsets, rng, n, max_iters, B)
    p = fundamental_params(threshold, confidence, subsets.shape[1])
    F, inl, rec = np.empty((B, 3, 3), np.float64), np.empty((B, n), np.uint8), np.zeros(B, RECORD_DTYPE)
    check(load().mav_find_fundamental(self.h, _ptr(src), _ptr(dst), n, B, C.byref(p), _ptr(subsets), _ptr(F), _ptr(inl), _ptr(rec)))
    return _result(F, inl, rec, single)


def _flow_shape(self, flow):
    """(is a device handle of this context, shape); a handle's deferred flow is enqueued first"""
    dev = _on_device(self, flow)
    if dev:
        if getattr(flow, "_deferred", None) is not None:
            flow._deferred.flush()
        return True, flow, tuple(flow.shape)
    flow = np.asarray(flow)
    return False, flow, flow.shape


def _flow_fundamental(self, flow, coords, threshold=3.0, confidence=0.99, max_iters=1000, subsets=None, rng=None, want_pairs=False) -> dict:
    """find_fundamental on the pairs coords -> coords + flow[y, x] (detector.py:126-128) of float32 fields (H, W, 2) or (B, H, W, 2), or
    of a device handle of this context (pipeline.DeviceArray or any object with .ptr and .shape): read where it is.  coords: (n, 2)
    integers (x, y) inside the frame.  With want_pairs the dict also has pairs_dst (B, n, 2) float64 (host fields only)."""
    lib = load()
    coords = self._coords(coords)
    n = coords.shape[0]
    dev, flow, shape = _flow_shape(self, flow)
    single = len(shape) == 3
    B = 1 if single else shape[0]
    subsets = _subsets_for(subsets, rng, n, max_iters, B)
    p = fundamental_params(threshold, confidence, subsets.shape[1])
    F, inl, rec = np.empty((B, 3, 3), np.float64), np.empty((B, n), np.uint8), np.zeros(B, RECORD_DTYPE)
    pairs = None
    if not dev:
        flow = self._flows(flow[None] if single else flow, B, "flow")
        pairs = np.empty((B, n, 2), np.float64) if want_pairs else None
        check(lib.mav_flow_fundamental(self.h, _ptr(flow), _ptr(coords), n, B, C.byref(p), _ptr(subsets), _ptr(F), _ptr(inl), _ptr(rec), _ptr(pairs)))
    else:
        if want_pairs:
            raise ValueError("flow_fundamental: want_pairs needs a host field")
        need = int(lib.mav_find_fundamental_workspace_bytes(n, B, C.byref(p)))
        bufs = []
        try:
            for nbytes in (subsets.nbytes, F.nbytes, inl.nbytes, rec.nbytes, need):
                bufs.append(self.alloc(max(nbytes, 1)))
            dt, dF, di, dr, dw = bufs
            dt.upload(subsets)
            check(lib.mav_flow_fundamental_dev(self.h, _dev_ptr(flow), _ptr(coords), n, B, C.byref(p), dt.ptr, dF.ptr, di.ptr, dr.ptr, dw.ptr, need))
            F, inl, rec = dF.download(np.float64, (B, 3, 3)), di.download(np.uint8, (B, n)), dr.download(RECORD_DTYPE, (B,))
        finally:
            for b in bufs:
                b.free()
    out = _result(F, inl, rec, single)
    if pairs is not None:
        out["pairs_dst"] = pairs[0] if single else pairs
    return out


def _find_fundamental_workspace_bytes(self, n: int, batch: int = 1, max_iters: int = 1000) -> int:
    """mav_find_fundamental_workspace_bytes: what find_fundamental_enqueue and flow_fundamental_enqueue need (a function of n, batch,
    max_iters)."""
    p = fundamental_params(max_iters=max_iters)
    need = load().mav_find_fundamental_workspace_bytes(int(n), int(batch), C.byref(p))
    if not need:
        raise _lib.MavflowError(load().mav_last_error().decode())
    return int(need)


def _find_fundamental_enqueue(self, src_ptr, dst_ptr, n: int, batch: int, subsets_ptr, F_ptr, inliers_ptr, records_ptr, workspace_ptr,
                              workspace_bytes: int, threshold=3.0, confidence=0.99, max_iters=1000) -> None:
    """mav_find_fundamental_dev: enqueue only, device pointers (ints, or objects with a .ptr): src, dst (batch, n, 2) float64, subsets
    (batch, max_iters, 7) int32, F (batch, 3, 3) float64, inliers (batch, n) uint8, records: `batch` RECORD_DTYPE blocks aligned to 16,
    a workspace of find_fundamental_workspace_bytes(...) aligned to 16.  A subset that is out of range or repeats an index is an invalid
    hypothesis."""
    p = fundamental_params(threshold, confidence, max_iters)
    check(load().mav_find_fundamental_dev(self.h, _dev_ptr(src_ptr), _dev_ptr(dst_ptr), int(n), int(batch), C.byref(p), _dev_ptr(subsets_ptr),
                                          _dev_ptr(F_ptr), _dev_ptr(inliers_ptr), _dev_ptr(records_ptr), _dev_ptr(workspace_ptr), int(workspace_bytes)))


def _flow_fundamental_enqueue(self, flow_ptr, coords, batch: int, subsets_ptr, F_ptr, inliers_ptr, records_ptr, workspace_ptr,
                              workspace_bytes: int, threshold=3.0, confidence=0.99, max_iters=1000) -> None:
    """mav_flow_fundamental_dev: enqueue only; flow (batch, H, W, 2) float32 on the device, coords (n, 2) integers on the HOST
    (range-checked and copied with the call), the rest as find_fundamental_enqueue.  The gathered pairs stay in the workspace."""
    coords = self._coords(coords)
    p = fundamental_params(threshold, confidence, max_iters)
    check(load().mav_flow_fundamental_dev(self.h, _dev_ptr(flow_ptr), _ptr(coords), coords.shape[0], int(batch), C.byref(p), _dev_ptr(subsets_ptr),
                                          _dev_ptr(F_ptr), _dev_ptr(inliers_ptr), _dev_ptr(records_ptr), _dev_ptr(workspace_ptr),
                                          int(workspace_bytes)))


def _epipolar_residual(self, flow, F, threshold=1.0, outputs=EPI_OUTPUTS) -> dict:
    """The dense epipolar residual of include/mavflow_fundamental.h: for every pixel p of float32 fields (H, W, 2) or (B, H, W, 2) -- or
    of a device handle of this context, read where it is -- the distance in pixels of p + flow(p) from the epipolar line of p under F
    ((3, 3) or (B, 3, 3) float64; one matrix serves every field of a batch), symmetric as in the fit.  Returns a dict with, of `outputs`,
    "residual" float32 and "mask" uint8 (255 where the residual exceeds threshold; the layout components() takes), and records
    (EPI_DTYPE), max_residual, flow_max (row, col: the first pixel of max_residual), movers, not_finite; a leading B for a batch.  An
    all-zero F (a failed fit's) gives a zero map, a zero mask and not_finite == H * W."""
    lib = load()
    for o in outputs:
        if o not in EPI_OUTPUTS:
            raise ValueError(f"epipolar_residual: outputs are among {EPI_OUTPUTS}, got {o!r}")
    dev, flow, shape = _flow_shape(self, flow)
    single = len(shape) == 3
    B = 1 if single else shape[0]
    F = np.asarray(F, np.float64)
    if F.shape == (3, 3):
        F = np.broadcast_to(F, (B, 3, 3))
    if F.shape != (B, 3, 3):
        raise ValueError(f"epipolar_residual: expected F (3, 3) or ({B}, 3, 3), got {F.shape}")
    F = np.ascontiguousarray(F)
    res = np.empty((B, self.H, self.W), np.float32) if "residual" in outputs else None
    mask = np.empty((B, self.H, self.W), np.uint8) if "mask" in outputs else None
    rec = np.zeros(B, EPI_DTYPE)
    if not dev:
        flow = self._flows(flow[None] if single else flow, B, "flow")
        check(lib.mav_epipolar_residual(self.h, _ptr(flow), _ptr(F), float(threshold), B, _ptr(res), _ptr(mask), _ptr(rec)))
    else:
        if shape[-3:] != (self.H, self.W, 2):
            raise ValueError(f"epipolar_residual: expected a ({self.H}, {self.W}, 2) field, got {shape}")
        bufs = {}
        try:
            bufs["F"] = self.alloc(F.nbytes).upload(F)
            bufs["rec"] = self.alloc(rec.nbytes)
            if res is not None:
                bufs["res"] = self.alloc(res.nbytes)
            if mask is not None:
                bufs["mask"] = self.alloc(mask.nbytes)
            check(lib.mav_epipolar_residual_dev(self.h, _dev_ptr(flow), bufs["F"].ptr, float(threshold), B, bufs["res"].ptr if res is not None else None,
                                                bufs["mask"].ptr if mask is not None else None, bufs["rec"].ptr))
            rec = bufs["rec"].download(EPI_DTYPE, (B,))
            res = bufs["res"].download(np.float32, res.shape) if res is not None else None
            mask = bufs["mask"].download(np.uint8, mask.shape) if mask is not None else None
        finally:
            for b in bufs.values():
                b.free()
    out = dict(records=rec, max_residual=rec["max_residual"].copy(), flow_max=np.stack([rec["max_row"], rec["max_col"]], -1),
               movers=rec["movers"].copy(), not_finite=rec["not_finite"].copy())
    if res is not None:
        out["residual"] = res
    if mask is not None:
        out["mask"] = mask
    if single:
        out = {k: v[0] for k, v in out.items()}
        out["flow_max"] = tuple(int(v) for v in out["flow_max"])
        for k in ("max_residual", "movers", "not_finite"):
            out[k] = out[k].item()
    return out


def _epipolar_residual_enqueue(self, flow_ptr, F_ptr, batch: int, residual_ptr, mask_ptr, records_ptr, threshold=1.0) -> None:
    """mav_epipolar_residual_dev: enqueue only, device pointers (ints, or objects with a .ptr; residual and mask may be None): flow
    (batch, H, W, 2) float32, F (batch, 3, 3) float64 -- the layout find_fundamental_enqueue writes, so a fit feeds the pass without the
    host -- residual (batch, H, W) float32, mask (batch, H, W) uint8, records: `batch` EPI_DTYPE blocks aligned to 16."""
    opt = lambda q: None if q is None else _dev_ptr(q)
    check(load().mav_epipolar_residual_dev(self.h, _dev_ptr(flow_ptr), _dev_ptr(F_ptr), float(threshold), int(batch), opt(residual_ptr), opt(mask_ptr),
                                           _dev_ptr(records_ptr)))


Context.find_fundamental = _find_fundamental
Context.flow_fundamental = _flow_fundamental
Context.find_fundamental_workspace_bytes = _find_fundamental_workspace_bytes
Context.find_fundamental_enqueue = _find_fundamental_enqueue
Context.flow_fundamental_enqueue = _flow_fundamental_enqueue
Context.epipolar_residual = _epipolar_residual
Context.epipolar_residual_enqueue = _epipolar_residual_enqueue


def repaired(ransacReprojThreshold, confidence):
    """cv2.findFundamentalMat's argument repair as remembered: a threshold <= 0 becomes 3; a confidence below DBL_EPSILON or above
    1 - DBL_EPSILON becomes 0.99"""
    threshold, confidence = float(ransacReprojThreshold), float(confidence)
    if threshold <= 0:
        threshold = 3.0
    if confidence < DBL_EPSILON or confidence > 1 - DBL_EPSILON:
        confidence = 0.99
    return threshold, confidence


def scaled(F):
    """cv2's scaling: F / F[2, 2] when |F[2, 2]| > DBL_EPSILON"""
    F = np.array(F, np.float64)
    return F / F[2, 2] if abs(F[2, 2]) > DBL_EPSILON else F


def findFundamentalMat(points1, points2, method=FM_RANSAC, ransacReprojThreshold=3., confidence=0.99, maxIters=1000, mask=None, rng=None):
    """cv2.findFundamentalMat's signature, constants and return shapes: (F (3, 3) float64 or None, mask (n, 1) uint8) for point sets (n, 2)
    or (n, 1, 2) of any real dtype.  method: FM_RANSAC only -- the sample subsets are drawn by sample_subsets from rng (np.random, a
    Generator or a seed; None: a fresh unseeded Generator), NOT from OpenCV's private generator, so a run equals no cv2 run sample for
    sample; FM_7POINT, FM_8POINT and FM_LMEDS raise NotImplementedError.  cv2's argument repair as remembered (`repaired`) and its scaling
    to F[2, 2] = 1 (`scaled`) are applied; n < 7 gives (None, zeros).  `mask` is accepted and ignored, as an output argument."""
    if int(method) != FM_RANSAC:
        raise NotImplementedError(f"findFundamentalMat: method {method} is not reproduced; method must be FM_RANSAC")
    a, b = np.asarray(points1, np.float64).reshape(-1, 2), np.asarray(points2, np.float64).reshape(-1, 2)
    if a.shape != b.shape:
        raise ValueError(f"findFundamentalMat: {a.shape[0]} and {b.shape[0]} points")
    n = a.shape[0]
    if n < 7:
        return None, np.zeros((n, 1), np.uint8)
    threshold, confidence = repaired(ransacReprojThreshold, confidence)
    from . import im_helpers
    ctx = im_helpers._ctx(1024, 16)
    out = ctx.find_fundamental(a, b, threshold=threshold, confidence=confidence, max_iters=maxIters, rng=rng)
    return (scaled(out["F"]) if out["ok"] else None), out["inliers"].reshape(-1, 1)
