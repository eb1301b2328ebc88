"""k-means clustering on the device (include/mavflow_cluster.h): the ctypes binding as methods of _lib.Context (kmeans, kmeans_enqueue,
kmeans_workspace_bytes, kmeans_paint, kmeans_paint_enqueue), the draw of random initial centres, and `kmeans` with cv2.kmeans' literal
signature and return shapes.  The library is _lib's (same loader, no CPU fallback); the entry points here are not in _lib.EXPORTS, which
lists include/mavflow.h alone.

The algorithm has cv2.kmeans' loop structure with the CALLER's initial centres: cv2 draws them from a private generator, so no
implementation can equal its draw.  With init=None the centres are drawn here (random_centers), from the caller's rng, by cv2's box rule;
the draw and its order are documented there and pinned to nothing."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import Context, _dev_ptr, _ptr, check

# every symbol include/mavflow_cluster.h declares (tests check the library exports each of them)
EXPORTS = ("mav_kmeans_defaults", "mav_kmeans_workspace_bytes", "mav_kmeans", "mav_kmeans_dev", "mav_kmeans_paint", "mav_kmeans_paint_dev")

KMEANS_F32, KMEANS_U8 = 0, 1                             # MAV_KMEANS_F32 / MAV_KMEANS_U8 (params.depth)
KMEANS_MAX_K, KMEANS_MAX_ATTEMPTS, KMEANS_MAX_DIMS, KMEANS_CHUNK = 16, 16, 4, 4096
# cv2's constants, for `kmeans` below
KMEANS_RANDOM_CENTERS, KMEANS_PP_CENTERS, KMEANS_USE_INITIAL_LABELS = 0, 2, 1
TERM_CRITERIA_COUNT = TERM_CRITERIA_MAX_ITER = 1
TERM_CRITERIA_EPS = 2


class KmeansParams(C.Structure):
    """mav_kmeans_params"""
    _fields_ = [("K", C.c_int), ("attempts", C.c_int), ("max_iter", C.c_int), ("dims", C.c_int), ("depth", C.c_int), ("flags", C.c_int),
                ("eps", C.c_double)]


class KmeansRecord(C.Structure):
    """mav_kmeans_record"""
    _fields_ = [("compactness", C.c_double), ("shift", C.c_double), ("best_attempt", C.c_int32), ("iterations", C.c_int32), ("repairs", C.c_int32),
                ("skipped", C.c_int32), ("counts", C.c_int32 * 16)]


RECORD_DTYPE = np.dtype([("compactness", np.float64), ("shift", np.float64), ("best_attempt", np.int32), ("iterations", np.int32),
                         ("repairs", np.int32), ("skipped", np.int32), ("counts", np.int32, (16,))])
assert C.sizeof(KmeansParams) == 32
assert RECORD_DTYPE.itemsize == C.sizeof(KmeansRecord) == 96

_ready = False


def load() -> C.CDLL:
    """_lib.load() with this header's prototypes attached."""
    global _ready
    lib = _lib.load()
    if not _ready:
        vp, i = C.c_void_p, C.c_int
        lib.mav_kmeans_defaults.restype, lib.mav_kmeans_defaults.argtypes = None, [vp]
        lib.mav_kmeans_workspace_bytes.restype, lib.mav_kmeans_workspace_bytes.argtypes = C.c_size_t, [i, i, vp]
        # ctx, samples, n, batch, params, init, labels, centers, records (, workspace, workspace_bytes)
        lib.mav_kmeans.restype, lib.mav_kmeans.argtypes = i, [vp, vp, i, i, vp, vp, vp, vp, vp]
        lib.mav_kmeans_dev.restype, lib.mav_kmeans_dev.argtypes = i, [vp, vp, i, i, vp, vp, vp, vp, vp, vp, C.c_size_t]
        # ctx, labels, centers, n, batch, K, dims, res, mask
        for name in ("mav_kmeans_paint", "mav_kmeans_paint_dev"):
            getattr(lib, name).restype, getattr(lib, name).argtypes = i, [vp, vp, vp, i, i, i, i, vp, vp]
        _ready = True
    return lib


def kmeans_params(K=8, attempts=10, max_iter=10, dims=3, dtype=np.float32, eps=1.0) -> KmeansParams:
    """The library's defaults with these fields."""
    p = KmeansParams()
    load().mav_kmeans_defaults(C.byref(p))
    dt = np.dtype(dtype)
    if dt not in (np.dtype(np.float32), np.dtype(np.uint8)):
        raise TypeError(f"kmeans takes float32 or uint8 samples, got {dt}")
    p.K, p.attempts, p.max_iter, p.dims, p.eps = int(K), int(attempts), int(max_iter), int(dims), float(eps)
    p.depth = KMEANS_U8 if dt == np.uint8 else KMEANS_F32
    return p


def _generator(rng):
    """np.random (the module), a Generator, a RandomState, a seed, or None (a fresh unseeded Generator): an object with .random(n)"""
    if rng is None:
        return np.random.default_rng()
    if hasattr(rng, "random"):
        return rng                      # np.random itself, a Generator or a RandomState
    return np.random.default_rng(rng)


def random_centers(samples, K: int, attempts: int, rng=None) -> np.ndarray:
    """(attempts, K, D) float32 centres by cv2's box rule (generateCentres of OpenCV 4.x kmeans.cpp as remembered; pinned to nothing):
    per dimension d, with lo / hi the data's minimum / maximum in float32 and margin = 1 / D,
        centre_d = ((float32)u * (1 + 2 * margin) - margin) * (hi_d - lo_d) + lo_d,     every operation in float32,
    u uniform in [0, 1).  The draws are ONE call rng.random(attempts * K * D), consumed attempt by attempt, centre by centre, dimension
    by dimension.  samples (N, D) or (B, N, D): the box is taken per image, the same draws serve every image."""
    x = np.asarray(samples)
    D = x.shape[-1]
    u = np.asarray(_generator(rng).random(int(attempts) * int(K) * D), np.float64).astype(np.float32).reshape(int(attempts), int(K), D)
    lo = x.min(axis=-2).astype(np.float32)[..., None, None, :]
    hi = x.max(axis=-2).astype(np.float32)[..., None, None, :]
    margin = np.float32(1.0) / np.float32(D)
    return ((u * (np.float32(1.0) + margin * np.float32(2.0)) - margin) * (hi - lo) + lo).astype(np.float32)


class DeviceSamples:
    """A plain device handle: what Context.kmeans and Detector.clustering need of one (.ctx, .ptr, .shape, .dtype); owns nothing."""

    def __init__(self, ctx, ptr, shape, dtype):
        self.ctx, self.ptr, self.shape, self.dtype = ctx, int(_dev_ptr(ptr)), tuple(shape), np.dtype(dtype)


def _on_device(ctx, a) -> bool:
    return hasattr(a, "ptr") and getattr(a, "on_device", True) and getattr(a, "ctx", ctx) is ctx


def _unwrap(out: dict, single: bool) -> dict:
    return {k: v[0] for k, v in out.items()} if single else out


def _result(rec, labels, centers, single):
    out = dict(labels=labels, centers=centers, compactness=rec["compactness"].copy(), best_attempt=rec["best_attempt"].copy(),
               iterations=rec["iterations"].copy(), repairs=rec["repairs"].copy(), counts=rec["counts"][:, :centers.shape[1]].copy(), records=rec)
    if single:
        out = _unwrap(out, True)
        for k in ("compactness", "best_attempt", "iterations", "repairs"):
            out[k] = out[k].item()
    return out


def _kmeans(self, samples, K=8, init=None, attempts=10, max_iter=10, eps=1.0, rng=None) -> dict:
    """k-means of (N, D) samples, or of a batch (B, N, D), float32 or uint8, D = 1..4, K and attempts = 1..16, on the device
    (include/mavflow_cluster.h has the algorithm).  init: (attempts, K, D) centres, or (B, attempts, K, D); None: drawn by random_centers
    with rng (np.random, a Generator or a seed).  samples may be a device handle of this context (pipeline.DeviceArray, or any object with
    .ptr, .shape and .dtype): read where it is; with init=None it is copied to the host once for the box of the draw.
    Returns a dict: labels (N,) int32, centers (K, D) float32, compactness, best_attempt, iterations (assignments the best attempt ran),
    repairs (samples moved into empty clusters, all attempts), counts (K,), records (RECORD_DTYPE); with a leading B for a batch."""
    lib = load()
    dev = _on_device(self, samples)
    if dev:
        if getattr(samples, "_deferred", None) is not None:
            samples._deferred.flush()
        shape, dtype = tuple(samples.shape), np.dtype(samples.dtype)
    else:
        samples = np.ascontiguousarray(samples)
        shape, dtype = samples.shape, samples.dtype
    if len(shape) not in (2, 3):
        raise ValueError(f"kmeans: samples have shape {shape}; expected (N, D) or (B, N, D)")
    single = len(shape) == 2
    B, N, D = (1,) + tuple(shape) if single else shape
    p = kmeans_params(K, attempts, max_iter, D, dtype, eps)
    if init is None:
        if dev:
            host = np.empty((B, N, D), dtype)
            check(lib.mav_memcpy_d2h(self.h, _ptr(host), _dev_ptr(samples), host.nbytes))
        else:
            host = samples.reshape(B, N, D)
        init = random_centers(host, K, attempts, rng)
    init = np.asarray(init, np.float32)
    if init.shape == (p.attempts, p.K, D):
        init = np.broadcast_to(init, (B,) + init.shape)
    if init.shape != (B, p.attempts, p.K, D):
        raise ValueError(f"kmeans: init has shape {init.shape}; expected ({p.attempts}, {p.K}, {D}) or ({B}, {p.attempts}, {p.K}, {D})")
    init = np.ascontiguousarray(init)
    labels, centers, rec = np.empty((B, N), np.int32), np.empty((B, p.K, D), np.float32), np.zeros(B, RECORD_DTYPE)
    if not dev:
        check(lib.mav_kmeans(self.h, _ptr(samples), N, B, C.byref(p), _ptr(init), _ptr(labels), _ptr(centers), _ptr(rec)))
    else:
        need = self.kmeans_workspace_bytes(N, B, K, attempts, D, dtype)
        bufs = []
        try:
            for nbytes in (init.nbytes, labels.nbytes, centers.nbytes, rec.nbytes, need):
                bufs.append(self.alloc(max(nbytes, 1)))
            di, dl, dc, dr, dw = bufs
            di.upload(init)
            check(lib.mav_kmeans_dev(self.h, _dev_ptr(samples), N, B, C.byref(p), di.ptr, dl.ptr, dc.ptr, dr.ptr, dw.ptr, need))
            labels, centers, rec = dl.download(np.int32, (B, N)), dc.download(np.float32, (B, p.K, D)), dr.download(RECORD_DTYPE, (B,))
        finally:
            for b in bufs:
                b.free()
    return _result(rec, labels, centers, single)


def _kmeans_workspace_bytes(self, n: int, batch: int = 1, K=8, attempts=10, dims=3, dtype=np.float32) -> int:
    """mav_kmeans_workspace_bytes: what kmeans_enqueue needs for these shapes (a function of n, batch, K, attempts and dims)."""
    p = kmeans_params(K, attempts, 10, dims, dtype, 1.0)
    need = load().mav_kmeans_workspace_bytes(int(n), int(batch), C.byref(p))
    if not need:
        raise _lib.MavflowError(load().mav_last_error().decode())
    return int(need)


def _kmeans_enqueue(self, samples_ptr, n: int, batch: int, init_ptr, labels_ptr, centers_ptr, records_ptr, workspace_ptr, workspace_bytes: int, K=8,
                    attempts=10, max_iter=10, eps=1.0, dims=3, dtype=np.float32) -> None:
    """mav_kmeans_dev: enqueue only, device pointers (ints, or objects with a .ptr): samples (batch, n, dims) of dtype, init (batch,
    attempts, K, dims) float32, labels (batch, n) int32, centers (batch, K, dims) float32, records: `batch` RECORD_DTYPE blocks aligned to
    16, a workspace of kmeans_workspace_bytes(...) aligned to 16."""
    p = kmeans_params(K, attempts, max_iter, dims, dtype, eps)
    check(load().mav_kmeans_dev(self.h, _dev_ptr(samples_ptr), int(n), int(batch), C.byref(p), _dev_ptr(init_ptr), _dev_ptr(labels_ptr),
                                _dev_ptr(centers_ptr), _dev_ptr(records_ptr), _dev_ptr(workspace_ptr), int(workspace_bytes)))


def _kmeans_paint(self, labels, centers):
    """What Detector.clustering does after the cv2 call (mav_kmeans_paint): labels (N,) / (N, 1) / (B, N) int32 and centers (K, D) /
    (B, K, D) float32 -> (res (.., N, D) uint8 = uint8(center * 255 / max(center))[label], mask (.., N) uint8 = res[..., 0] >= 225)."""
    centers = np.ascontiguousarray(centers, np.float32)
    single = centers.ndim == 2
    centers = centers[None] if single else centers
    B, K, D = centers.shape
    labels = np.ascontiguousarray(labels, np.int32).reshape(B, -1)
    N = labels.shape[1]
    if labels.size and (labels.min() < 0 or labels.max() >= K):
        raise ValueError(f"kmeans_paint: labels outside [0, {K})")
    res, mask = np.empty((B, N, D), np.uint8), np.empty((B, N), np.uint8)
    check(load().mav_kmeans_paint(self.h, _ptr(labels), _ptr(centers), N, B, K, D, _ptr(res), _ptr(mask)))
    return (res[0], mask[0]) if single else (res, mask)


def _kmeans_paint_enqueue(self, labels_ptr, centers_ptr, n: int, batch: int, K: int, dims: int, res_ptr, mask_ptr=None) -> None:
    """mav_kmeans_paint_dev: enqueue only, device pointers."""
    check(load().mav_kmeans_paint_dev(self.h, _dev_ptr(labels_ptr), _dev_ptr(centers_ptr), int(n), int(batch), int(K), int(dims), _dev_ptr(res_ptr),
                                      None if mask_ptr is None else _dev_ptr(mask_ptr)))


Context.kmeans = _kmeans
Context.kmeans_workspace_bytes = _kmeans_workspace_bytes
Context.kmeans_enqueue = _kmeans_enqueue
Context.kmeans_paint = _kmeans_paint
Context.kmeans_paint_enqueue = _kmeans_paint_enqueue


def context_for(n_values: int) -> "Context":
    """A cached context (im_helpers._ctx) whose staging bound, max_batch * W * H * 4 values, covers n_values: the sample count is not a
    frame size, so the frame is a strip of 1024 x h."""
    from . import im_helpers
    return im_helpers._ctx(1024, max(1, -(-int(n_values) // 4096)))


def kmeans(data, K, bestLabels, criteria, attempts, flags, centers=None, rng=None):
    """cv2.kmeans' signature and return shapes: (compactness, labels (N, 1) int32, centers (K, D) float32) for data (N, D) float32 (a
    1-D array is N samples of one dimension).  criteria = (type, max_iter, eps): without TERM_CRITERIA_EPS eps is 0, without
    TERM_CRITERIA_MAX_ITER max_iter is 100.  flags: KMEANS_RANDOM_CENTERS only -- the centres are drawn by random_centers from rng
    (np.random, a Generator or a seed; None: a fresh unseeded Generator), NOT from OpenCV's private generator, so a run equals no cv2
    run sample for sample.  KMEANS_PP_CENTERS and KMEANS_USE_INITIAL_LABELS raise NotImplementedError.  bestLabels and centers are
    accepted and ignored, as cv2's Python binding ignores them without KMEANS_USE_INITIAL_LABELS."""
    if int(flags) & KMEANS_PP_CENTERS:
        raise NotImplementedError("KMEANS_PP_CENTERS: k-means++ seeding is not reproduced; draw the centres and pass them to Context.kmeans")
    if int(flags) & KMEANS_USE_INITIAL_LABELS:
        raise NotImplementedError("KMEANS_USE_INITIAL_LABELS is not reproduced")
    data = np.asarray(data)
    if data.dtype != np.float32:
        raise TypeError(f"kmeans: data must be float32 as cv2.kmeans demands, got {data.dtype}")
    data = data.reshape(data.shape[0], -1) if data.ndim != 2 else data
    ctype, count, eps = criteria
    max_iter = int(count) if int(ctype) & TERM_CRITERIA_MAX_ITER else 100
    eps = float(eps) if int(ctype) & TERM_CRITERIA_EPS else 0.0
    out = context_for(data.size).kmeans(data, K=K, attempts=attempts, max_iter=max_iter, eps=eps, rng=rng)
    return out["compactness"], out["labels"].reshape(-1, 1), out["centers"]
