"""ctypes binding of include/mavflow_truth.h: the ground-truth flow from depth and pose (mav_gt_flow) and the radial-error histogram of a
flow against it (mav_radial_error_hist), as methods of _lib.Context.  The library is _lib's (same loader, no CPU fallback); the entry
points here are not in _lib.EXPORTS, which lists include/mavflow.h alone."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import DEPTH_32F, DEPTH_64F, Context, _arr, _dev_ptr, _ptr, check

# every symbol include/mavflow_truth.h declares (tests check the library exports each of them)
EXPORTS = ("mav_gt_flow", "mav_gt_flow_dev", "mav_radial_error_hist", "mav_radial_error_hist_dev")

RADIAL_MAX_EDGES, RADIAL_MAX_CELLS = 257, 65536         # MAV_RADIAL_MAX_EDGES / MAV_RADIAL_MAX_CELLS
DEFAULT_MAG_EDGES = np.linspace(0, 10, 160)             # the reference's bins (src/plot_radial_error.py:38)
DEFAULT_ERR_EDGES = np.linspace(-20, 20, 160)
GT_FLOW_DEPTHS = {np.dtype(np.float32): DEPTH_32F, np.dtype(np.float64): DEPTH_64F}


class GtFlowParams(C.Structure):
    """mav_gt_flow_params: one pair's two matrices (row-major), the MAV's displacement, the float32 depth factor, flags (0)."""
    _fields_ = [("view_proj_prev", C.c_double * 16), ("view_proj_inv", C.c_double * 16), ("displacement", C.c_double * 3),
                ("depth_scale", C.c_float), ("flags", C.c_int)]


GT_FLOW_PARAMS_DTYPE = np.dtype([("view_proj_prev", np.float64, (16,)), ("view_proj_inv", np.float64, (16,)), ("displacement", np.float64, (3,)),
                                 ("depth_scale", np.float32), ("flags", np.int32)])
assert GT_FLOW_PARAMS_DTYPE.itemsize == C.sizeof(GtFlowParams) == 288

_ready = False


def load() -> C.CDLL:
    """_lib.load() with this header's prototypes attached."""
    global _ready
    lib = _lib.load()
    if not _ready:
        vp = C.c_void_p
        for name in EXPORTS:
            getattr(lib, name).restype = C.c_int
        # ctx, depth, seg, params, batch, out_depth, flow
        lib.mav_gt_flow.argtypes = lib.mav_gt_flow_dev.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, vp]
        # ctx, flow, gt_flow, sky, batch, mag_edges, n_mag_edges, err_edges, n_err_edges, table
        lib.mav_radial_error_hist.argtypes = lib.mav_radial_error_hist_dev.argtypes = [vp, vp, vp, vp, C.c_int, vp, C.c_int, vp, C.c_int, vp]
        _ready = True
    return lib


def table_words(bins_mag: int, bins_err: int) -> int:
    """MAV_RADIAL_TABLE_WORDS: non_sky, in_range, then counts[i][j]"""
    return 2 + int(bins_mag) * int(bins_err)


def gt_flow_params(view_proj_prev, view_proj_inv, displacement, depth_scale=1.0, batch=None) -> np.ndarray:
    """(B,) GT_FLOW_PARAMS_DTYPE blocks from (B, 4, 4) / (4, 4) matrices, (B, 3) / (3,) displacements and one factor or B."""
    vp1, inv = np.asarray(view_proj_prev, np.float64), np.asarray(view_proj_inv, np.float64)
    B = int(batch) if batch is not None else (vp1.shape[0] if vp1.ndim == 3 else 1)
    if vp1.shape[-2:] != (4, 4) or inv.shape[-2:] != (4, 4):
        raise ValueError(f"gt_flow: view-projection matrices must be 4x4, got {vp1.shape} and {inv.shape}")
    p = np.zeros(B, GT_FLOW_PARAMS_DTYPE)
    p["view_proj_prev"] = np.broadcast_to(vp1.reshape(-1, 16), (B, 16))
    p["view_proj_inv"] = np.broadcast_to(inv.reshape(-1, 16), (B, 16))
    p["displacement"] = np.broadcast_to(np.asarray(displacement, np.float64).reshape(-1, 3), (B, 3))
    p["depth_scale"] = np.broadcast_to(np.asarray(depth_scale, np.float32).reshape(-1), (B,))
    return p


def _edges(e) -> np.ndarray:
    """an edge list as a contiguous float64 array (the library checks it: strictly increasing, finite, 2 .. 257 entries)"""
    return np.ascontiguousarray(np.asarray(e, np.float64).reshape(-1))


def _result(table: np.ndarray, nm: int, ne: int) -> dict:
    return dict(counts=table[2:].reshape(nm - 1, ne - 1).copy(), non_sky=int(table[0]), in_range=int(table[1]))


def _fields(ctx, flow, gt_flow_, sky):
    """(flow, gt_flow, sky or None, B) as the contiguous arrays a host call takes; a float64 field is refused (it would round)"""
    out = []
    for a, name in ((flow, "flow"), (gt_flow_, "gt_flow")):
        a = np.asarray(a)
        if a.dtype != np.float32:
            raise TypeError(f"radial_error_hist() takes float32 fields, got {a.dtype} for {name}")
        out.append(a[None] if a.ndim == 3 else a)
    B = out[0].shape[0]
    flow, gt_flow_ = (_arr(a, np.float32, (B, ctx.H, ctx.W, 2), n) for a, n in zip(out, ("flow", "gt_flow")))
    sky = None if sky is None else _arr((np.asarray(sky).reshape(B, ctx.H, ctx.W) != 0).astype(np.uint8), np.uint8)
    return flow, gt_flow_, sky, B


def _gt_flow(self, depth, seg, view_proj_prev, view_proj_next, displacement, depth_scale=1.0, dtype=np.float32, view_proj_inv=None) -> np.ndarray:
    """The ground-truth flow of the reference's write_flow (src/airsim_optical_flow.py:109-149) for one pair or a batch: depth (H, W) or
    (B, H, W) float32 (float64 is a TypeError: it would round), seg likewise uint8 (the MAV is seg > 0; None: no MAV), the two states'
    view-projection matrices (get_view_proj_mat: (4, 4) or (B, 4, 4)), the MAV's displacement (3,) or (B, 3), the float32 factor on the
    depth.  view_proj_next is inverted here with numpy.linalg.inv, as calculate_flow does (view_proj_inv: the inverse, if the caller
    has it already).  Returns (H, W, 2) / (B, H, W, 2) of dtype: float64 = the array write_flow hands to utils.write_flow, float32 = it
    rounded (what the .flo holds and get_gt_of returns)."""
    depth = np.asarray(depth)
    if depth.dtype != np.float32:
        raise TypeError(f"gt_flow() takes a float32 depth buffer, got {depth.dtype}")
    if np.dtype(dtype) not in GT_FLOW_DEPTHS:
        raise ValueError(f"gt_flow: dtype must be float32 or float64, got {np.dtype(dtype)}")
    single = depth.ndim == 2
    depth = depth[None] if single else depth
    B = depth.shape[0]
    depth = _arr(depth, np.float32, (B, self.H, self.W), "depth")
    seg = None if seg is None else _arr(np.asarray(seg).reshape(B, self.H, self.W), np.uint8)
    inv = np.linalg.inv(np.asarray(view_proj_next, np.float64)) if view_proj_inv is None else view_proj_inv
    p = gt_flow_params(view_proj_prev, inv, displacement, depth_scale, B)
    out = np.empty((B, self.H, self.W, 2), dtype)
    check(load().mav_gt_flow(self.h, _ptr(depth), _ptr(seg), _ptr(p), B, GT_FLOW_DEPTHS[np.dtype(dtype)], _ptr(out)))
    return out[0] if single else out


def _gt_flow_enqueue(self, depth_ptr, seg_ptr, params_ptr, batch: int, flow_ptr, dtype=np.float32) -> None:
    """mav_gt_flow_dev: enqueue only, device pointers (ints, or objects with a .ptr); params: `batch` GT_FLOW_PARAMS_DTYPE blocks on the
    device (gt_flow_params builds them); seg_ptr may be None."""
    if np.dtype(dtype) not in GT_FLOW_DEPTHS:
        raise ValueError(f"gt_flow_enqueue: dtype must be float32 or float64, got {np.dtype(dtype)}")
    check(load().mav_gt_flow_dev(self.h, _dev_ptr(depth_ptr), None if seg_ptr is None else _dev_ptr(seg_ptr), _dev_ptr(params_ptr), int(batch),
                                 GT_FLOW_DEPTHS[np.dtype(dtype)], _dev_ptr(flow_ptr)))


def _radial_error_hist(self, flow, gt_flow, sky=None, mag_edges=DEFAULT_MAG_EDGES, err_edges=DEFAULT_ERR_EDGES) -> dict:
    """Flow magnitude against angular error of flow vs gt_flow over the non-sky pixels, binned as numpy.histogram2d bins the arrays the
    reference's analyze_radial_error saves: counts (Nm, Ne) int64, non_sky, in_range.  Fields (H, W, 2) or (B, H, W, 2) float32."""
    flow, gt_flow, sky, B = _fields(self, flow, gt_flow, sky)
    em, ee = _edges(mag_edges), _edges(err_edges)
    table = np.zeros(table_words(max(em.size - 1, 0), max(ee.size - 1, 0)), np.int64)
    check(load().mav_radial_error_hist(self.h, _ptr(flow), _ptr(gt_flow), _ptr(sky), B, _ptr(em), em.size, _ptr(ee), ee.size, _ptr(table)))
    return _result(table, em.size, ee.size)


class RadialErrorAccumulator:
    """A radial-error histogram that builds up on the device (Context.radial_error_accumulator): the table is a device block between
    calls; add() stages host fields or reads the loop's device handles where they are; only counts() brings anything back."""

    def __init__(self, ctx: Context, mag_edges=DEFAULT_MAG_EDGES, err_edges=DEFAULT_ERR_EDGES):
        self.ctx, self.mag_edges, self.err_edges = ctx, _edges(mag_edges), _edges(err_edges)
        nm, ne = self.mag_edges.size, self.err_edges.size
        if not (2 <= nm <= RADIAL_MAX_EDGES and 2 <= ne <= RADIAL_MAX_EDGES) or (nm - 1) * (ne - 1) > RADIAL_MAX_CELLS:
            raise ValueError(f"radial_error_accumulator: {nm} x {ne} edges (2 .. {RADIAL_MAX_EDGES} each, at most {RADIAL_MAX_CELLS} cells)")
        self.words = table_words(nm - 1, ne - 1)
        self.table = ctx.alloc(self.words * 8)
        self.frames = 0
        self.reset()

    def reset(self) -> None:
        """zero counts (waits for what was enqueued)"""
        self.table.upload(np.zeros(self.words, np.int64))
        self.frames = 0

    def add_enqueue(self, flow_ptr, gt_flow_ptr, sky_ptr=None, batch: int = 1) -> None:
        """mav_radial_error_hist_dev into the table: enqueue only, device pointers (ints, or objects with a .ptr)."""
        check(load().mav_radial_error_hist_dev(self.ctx.h, _dev_ptr(flow_ptr), _dev_ptr(gt_flow_ptr), None if sky_ptr is None else _dev_ptr(sky_ptr),
                                               int(batch), _ptr(self.mag_edges), self.mag_edges.size, _ptr(self.err_edges), self.err_edges.size,
                                               self.table.ptr))
        self.frames += int(batch)

    @staticmethod
    def _on_device(ctx, a) -> bool:
        return hasattr(a, "ptr") and getattr(a, "on_device", True) and getattr(a, "ctx", ctx) is ctx

    def add(self, flow, gt_flow, sky=None) -> None:
        """One frame or a batch.  Each of flow / gt_flow (float32 (H, W, 2) or (B, H, W, 2)) and sky ((H, W) / (B, H, W), non-zero or
        True = sky, or None) is a host array, staged for the call, or a device handle of this context with .ptr / .shape (a
        pipeline.DeviceArray of the loop), read where it is."""
        ctx = self.ctx
        staged, ptrs, B = [], [], None
        try:
            for a, name, tail in ((flow, "flow", (ctx.H, ctx.W, 2)), (gt_flow, "gt_flow", (ctx.H, ctx.W, 2)), (sky, "sky", (ctx.H, ctx.W))):
                if a is None:
                    if name != "sky":
                        raise ValueError(f"add: {name} is None")
                    ptrs.append(None)
                    continue
                if self._on_device(ctx, a):
                    if getattr(a, "_deferred", None) is not None:             # a flow the flow stage has not enqueued yet
                        a._deferred.flush()
                    if name != "sky" and np.dtype(a.dtype) != np.float32:
                        raise TypeError(f"add: {name} must be float32, got {a.dtype}")
                    shape, ptr = tuple(a.shape), a.ptr
                else:
                    a = np.asarray(a)
                    if name == "sky":
                        a = (a != 0).astype(np.uint8)
                    elif a.dtype != np.float32:
                        raise TypeError(f"add: {name} must be float32 (a float64 field would be rounded), got {a.dtype}")
                    a = np.ascontiguousarray(a)
                    shape = a.shape
                    staged.append(ctx.alloc(a.nbytes).upload(a))
                    ptr = staged[-1].ptr
                n = 1 if len(shape) == len(tail) else shape[0]
                if tuple(shape[-len(tail):]) != tail or len(shape) not in (len(tail), len(tail) + 1) or (B is not None and n != B):
                    raise ValueError(f"add: {name} has shape {shape}; expected {tail} or (B,) + {tail} with the same B for all")
                B = n
                ptrs.append(ptr)
            self.add_enqueue(ptrs[0], ptrs[1], ptrs[2], B)
            if staged:
                ctx.sync()
        finally:
            for b in staged:
                b.free()

    def counts(self) -> dict:
        """the histogram so far (waits for what was enqueued)"""
        t = self.table.download(np.int64, (self.words,))
        return _result(t, self.mag_edges.size, self.err_edges.size)

    def close(self) -> None:
        if getattr(self, "table", None) is not None and self.ctx.alive:
            self.table.free()
        self.table = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _radial_error_accumulator(self, mag_edges=DEFAULT_MAG_EDGES, err_edges=DEFAULT_ERR_EDGES) -> RadialErrorAccumulator:
    """A histogram that accumulates over calls on the device (RadialErrorAccumulator)."""
    return RadialErrorAccumulator(self, mag_edges, err_edges)


Context.gt_flow = _gt_flow
Context.gt_flow_enqueue = _gt_flow_enqueue
Context.radial_error_hist = _radial_error_hist
Context.radial_error_accumulator = _radial_error_accumulator
