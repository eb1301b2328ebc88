"""ctypes binding of include/mavflow_validation.h: the validation tail of the reference's loop (drone pixel count and list, the
segmentation's bounding box, validate_sky_segment's counts, the sum of the derotated ground-truth flow over the drone) in one call,
as methods of _lib.Context.  The library is _lib's (same loader, no CPU fallback); the entry points here are not in _lib.EXPORTS, which
lists include/mavflow.h alone."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import Context, _arr, _dev_ptr, _ptr, check

# every symbol include/mavflow_validation.h declares (tests check the library exports each of them)
EXPORTS = ("mav_gt_stats_defaults", "mav_gt_stats", "mav_gt_stats_dev")

GT_STATS_FRAME0, GT_STATS_THR_F64 = 1, 2                 # MAV_GT_STATS_FRAME0 / MAV_GT_STATS_THR_F64 (params.flags)
GT_STATS_TRUNCATED, GT_STATS_DEPTH_NAN = 1, 2            # MAV_GT_STATS_TRUNCATED / MAV_GT_STATS_DEPTH_NAN (record.flags)
GT_STATS_MAX_PIXELS = 1 << 20                            # MAV_GT_STATS_MAX_PIXELS
DEFAULT_MAX_PIXELS = 16384


class GtStatsParams(C.Structure):
    """mav_gt_stats_params: one pair's rates and time step, the two fractions, the MAV threshold, flags."""
    _fields_ = [("omega", C.c_double * 3), ("dt", C.c_double), ("box_fraction", C.c_double), ("depth_fraction", C.c_float),
                ("seg_threshold", C.c_int), ("flags", C.c_int), ("pad", C.c_int)]


class GtStatsRecord(C.Structure):
    """mav_gt_stats_record"""
    _fields_ = [("drone_pixels", C.c_int64), ("sky", C.c_int64 * 4), ("flow_sum", C.c_double * 2), ("box", C.c_int32 * 4), ("seg_max", C.c_int32),
                ("listed", C.c_int32), ("depth_max", C.c_float), ("flags", C.c_uint32), ("pad", C.c_uint32 * 2)]


PARAMS_DTYPE = np.dtype([("omega", np.float64, (3,)), ("dt", np.float64), ("box_fraction", np.float64), ("depth_fraction", np.float32),
                         ("seg_threshold", np.int32), ("flags", np.int32), ("pad", np.int32)])
RECORD_DTYPE = np.dtype([("drone_pixels", np.int64), ("sky", np.int64, (4,)), ("flow_sum", np.float64, (2,)), ("box", np.int32, (4,)),
                         ("seg_max", np.int32), ("listed", np.int32), ("depth_max", np.float32), ("flags", np.uint32), ("pad", np.uint32, (2,))])
assert PARAMS_DTYPE.itemsize == C.sizeof(GtStatsParams) == 56
assert RECORD_DTYPE.itemsize == C.sizeof(GtStatsRecord) == 96

_ready = False


def load() -> C.CDLL:
    """_lib.load() with this header's prototypes attached."""
    global _ready
    lib = _lib.load()
    if not _ready:
        vp = C.c_void_p
        lib.mav_gt_stats_defaults.restype, lib.mav_gt_stats_defaults.argtypes = None, [vp]
        # ctx, seg, gt_flow, sky, depth, params, batch, max_pixels, records, indices
        for name in ("mav_gt_stats", "mav_gt_stats_dev"):
            getattr(lib, name).restype = C.c_int
            getattr(lib, name).argtypes = [vp, vp, vp, vp, vp, vp, C.c_int, C.c_int, vp, vp]
        _ready = True
    return lib


def gt_stats_params(omega=(0.0, 0.0, 0.0), dt=1.0, frame0=False, legacy_threshold=False, batch=None) -> np.ndarray:
    """(B,) PARAMS_DTYPE blocks, the library's defaults (box_fraction 0.1, depth_fraction 0.8f, seg_threshold 127) with (B, 3) / (3,)
    rates, one time step or B, one frame0 / legacy_threshold or B."""
    om = np.asarray(omega, np.float64)
    B = int(batch) if batch is not None else (om.shape[0] if om.ndim == 2 else 1)
    d = GtStatsParams()
    load().mav_gt_stats_defaults(C.byref(d))
    p = np.zeros(B, PARAMS_DTYPE)
    p["box_fraction"], p["depth_fraction"], p["seg_threshold"] = d.box_fraction, d.depth_fraction, d.seg_threshold
    p["omega"] = np.broadcast_to(om.reshape(-1, 3), (B, 3))
    p["dt"] = np.broadcast_to(np.asarray(dt, np.float64).reshape(-1), (B,))
    f0 = np.broadcast_to(np.asarray(frame0, bool).reshape(-1), (B,))
    lg = np.broadcast_to(np.asarray(legacy_threshold, bool).reshape(-1), (B,))
    p["flags"] = f0 * GT_STATS_FRAME0 + lg * GT_STATS_THR_F64
    return p


def _on_device(ctx, a) -> bool:
    return hasattr(a, "ptr") and getattr(a, "on_device", True) and getattr(a, "ctx", ctx) is ctx


def _gt_stats(self, seg, gt_flow=None, sky=None, depth=None, omega=(0.0, 0.0, 0.0), dt=1.0, frame0=False, max_pixels=DEFAULT_MAX_PIXELS,
              indices=True, legacy_threshold=False) -> dict:
    """The validation tail of the reference's loop (src/processor.py:315-317, 343-347, 360) for one frame or a batch, in one call on the
    device.  seg (H, W) or (B, H, W) uint8 (the drone is seg > 127), gt_flow (.., H, W, 2) float32, sky (.., H, W) (non-zero or True = sky),
    depth (.., H, W) float32; gt_flow, sky and depth may each be None.  A float64 depth or ground-truth flow is a TypeError (it would
    round).  seg and gt_flow may be device handles of this context (pipeline.DeviceArray): read where they are, the other inputs are
    then staged beside them.  omega (3,) / (B, 3) and dt as detect() takes them, frame0: no derotation (one flag or B).
    legacy_threshold: the depth threshold by numpy 1.x's casting rule (include/mavflow_validation.h).
    Returns records (a RECORD_DTYPE array, (B,)), indices (a list of B int32 arrays y * W + x in raster order, cut to `listed`; None
    with indices=False), and per frame: drone_size_pixels (numpy int64), box (a Rectangle as get_simple_bounding_box returns it),
    sky_tpr_fpr (calculate_tpr_fpr's pair, None without depth), drone_flow_avg (flow_sum / drone_pixels as np.average gives it: float64,
    float32 at frame 0, NaN for an empty drone; None without gt_flow or for a truncated list), truncated.  A single frame gives the
    per-frame fields unwrapped."""
    from . import im_helpers
    from .utils import Rectangle
    H, W = self.H, self.W
    dev = {}
    single = None
    B = None
    host = {}
    for name, a, tail, dtype in (("seg", seg, (H, W), np.uint8), ("gt_flow", gt_flow, (H, W, 2), np.float32), ("sky", sky, (H, W), np.uint8),
                                 ("depth", depth, (H, W), np.float32)):
        if a is None:
            if name == "seg":
                raise ValueError("gt_stats: seg is None")
            continue
        if _on_device(self, a):
            if name not in ("seg", "gt_flow"):
                raise TypeError(f"gt_stats: {name} must be a host array")
            if getattr(a, "_deferred", None) is not None:
                a._deferred.flush()
            if np.dtype(a.dtype) != dtype:
                raise TypeError(f"gt_stats: {name} must be {np.dtype(dtype)}, got {a.dtype}")
            shape = tuple(a.shape)
            dev[name] = a
        else:
            a = np.asarray(a)
            if name in ("gt_flow", "depth") and a.dtype != np.float32:
                raise TypeError(f"gt_stats() takes a float32 {name} (a float64 array would be rounded), got {a.dtype}")
            if name == "sky":
                a = (a != 0).astype(np.uint8)
            shape = a.shape
            host[name] = a
        if tuple(shape[-len(tail):]) != tail or len(shape) not in (len(tail), len(tail) + 1):
            raise ValueError(f"gt_stats: {name} has shape {tuple(shape)}; expected {tail} or (B,) + {tail}")
        n = 1 if len(shape) == len(tail) else shape[0]
        if B is not None and n != B:
            raise ValueError(f"gt_stats: {name} holds {n} frames, the others {B}")
        B = n
        if name == "seg":
            single = len(shape) == len(tail)
    mp = int(max_pixels)
    p = gt_stats_params(omega, dt, frame0, legacy_threshold, B)
    rec = np.zeros(B, RECORD_DTYPE)
    idx = np.empty((B, mp), np.int32) if indices and 1 <= mp <= GT_STATS_MAX_PIXELS else None
    lib = load()
    if not dev:
        arrs = {k: _arr(v.reshape((B,) + v.shape[-(2 if k != "gt_flow" else 3):]), v.dtype) for k, v in host.items()}
        check(lib.mav_gt_stats(self.h, _ptr(arrs["seg"]), _ptr(arrs.get("gt_flow")), _ptr(arrs.get("sky")), _ptr(arrs.get("depth")), _ptr(p), B, mp,
                               _ptr(rec), _ptr(idx)))
    else:
        staged = []
        try:
            def up(a):
                a = np.ascontiguousarray(a)
                staged.append(self.alloc(max(a.nbytes, 1)).upload(a))
                return staged[-1].ptr
            ptrs = {k: (dev[k].ptr if k in dev else up(host[k]) if k in host else None) for k in ("seg", "gt_flow", "sky", "depth")}
            dp = up(p)
            dr = self.alloc(rec.nbytes)
            staged.append(dr)
            di = None
            if idx is not None:
                di = self.alloc(idx.nbytes)
                staged.append(di)
            self.gt_stats_enqueue(ptrs["seg"], ptrs["gt_flow"], ptrs["sky"], ptrs["depth"], dp, B, mp, dr.ptr, None if di is None else di.ptr)
            rec = dr.download(RECORD_DTYPE, (B,))
            if di is not None:
                idx = di.download(np.int32, (B, mp))
        finally:
            for b in staged:
                b.free()
    out = dict(records=rec, indices=None if idx is None else [idx[b, :rec["listed"][b]].copy() for b in range(B)])
    trunc = (rec["flags"] & GT_STATS_TRUNCATED) != 0
    f0 = np.broadcast_to(np.asarray(frame0, bool).reshape(-1), (B,))
    sizes, boxes, rates, avgs = [], [], [], []
    for b in range(B):
        r = rec[b]
        sizes.append(np.int64(r["drone_pixels"]))
        boxes.append(Rectangle.from_points((int(r["box"][0]), int(r["box"][1])), (int(r["box"][2]), int(r["box"][3]))))
        rates.append(im_helpers._rates(r["sky"]) if "depth" in host else None)
        if gt_flow is None or trunc[b]:
            avgs.append(None)
        else:
            with np.errstate(all="ignore"):
                avgs.append(r["flow_sum"].astype(np.float32) / np.float32(r["drone_pixels"]) if f0[b] else r["flow_sum"] / np.float64(r["drone_pixels"]))
    pick = (lambda v: v[0]) if single else (lambda v: v)
    out.update(drone_size_pixels=pick(sizes), box=pick(boxes), sky_tpr_fpr=pick(rates), drone_flow_avg=pick(avgs), truncated=pick([bool(t) for t in trunc]))
    return out


def _gt_stats_enqueue(self, seg_ptr, gt_flow_ptr, sky_ptr, depth_ptr, params_ptr, batch: int, max_pixels: int, records_ptr, indices_ptr=None) -> None:
    """mav_gt_stats_dev: enqueue only, device pointers (ints, or objects with a .ptr); params: `batch` PARAMS_DTYPE blocks on the device
    (gt_stats_params builds them), records: `batch` RECORD_DTYPE blocks, indices: (batch, max_pixels) int32 or None; gt_flow_ptr, sky_ptr
    and depth_ptr may be None."""
    opt = lambda p: None if p is None else _dev_ptr(p)
    check(load().mav_gt_stats_dev(self.h, _dev_ptr(seg_ptr), opt(gt_flow_ptr), opt(sky_ptr), opt(depth_ptr), _dev_ptr(params_ptr), int(batch),
                                  int(max_pixels), _dev_ptr(records_ptr), opt(indices_ptr)))


Context.gt_stats = _gt_stats
Context.gt_stats_enqueue = _gt_stats_enqueue
