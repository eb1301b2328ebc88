"""Farneback -- the reference's stateful wrapper (/root/reference/src/farneback.py:12-107) with
cv2.calcOpticalFlowFarneback replaced by libmavflow's HIP path; the parameters are the reference's literals (:78-80).

`capture` is anything with .read() -> (ok, BGR u8 frame) (cv2.VideoCapture has that shape).  process() keeps the
reference's behaviour -- it returns a BGR visualisation and falls back to the previous one when the frame produces no
flow -- and additionally exposes the dense field as .flow, which the reference computes and throws away."""
from __future__ import annotations

import builtins

import numpy as np

from . import _lib


def flow_to_hsv(flow: np.ndarray):
    """The HSV image the reference composes from a flow field (farneback.py:83-94), including its quirks: hue = angle / 2
    in degrees truncated to u8, saturation 255, value = 2 x min-max-normalised magnitude stored into a u8 array (numpy
    wraps it modulo 256, so the upper half of the magnitude range folds over), and pixels with value < 1 repainted as
    (127, 255, 255).  cv2.cartToPolar's angle is a ~0.3 degree approximation, so hues can differ by one step from cv2's:
    visualisation only, not a parity surface.  Returns (hsv u8, invalid_frame)."""
    fx, fy = flow[..., 0].astype(np.float32), flow[..., 1].astype(np.float32)
    mag = np.sqrt(fx * fx + fy * fy)
    ang = np.arctan2(fy, fx).astype(np.float32)
    ang = np.where(ang < 0, ang + np.float32(2 * np.pi), ang)
    lo, hi = float(mag.min()), float(mag.max())
    norm = np.zeros_like(mag) if hi - lo <= np.finfo(np.float64).eps else (mag - lo) * np.float32(255.0 / (hi - lo))
    hsv = np.zeros(flow.shape[:2] + (3,), np.uint8)
    hsv[..., 0] = (ang * 180 / np.pi / 2).astype(np.int64) & 255
    hsv[..., 1] = 255
    hsv[..., 2] = (norm * 2.0).astype(np.int64) & 255
    mask = hsv[..., 2] < 1
    hsv[mask, 0] = 127
    hsv[mask, 2] = 255
    return hsv, bool(np.sum((norm * 2.0).astype(np.int64) & 255) < 1)


def hsv_to_bgr(hsv: np.ndarray) -> np.ndarray:
    """cv2.cvtColor(COLOR_HSV2BGR) on u8 (H in [0, 180)): the float sector formula, rounded to nearest."""
    h = hsv[..., 0].astype(np.float32) * np.float32(6.0 / 180.0)
    s = hsv[..., 1].astype(np.float32) / np.float32(255)
    v = hsv[..., 2].astype(np.float32) / np.float32(255)
    sector = np.floor(h)
    f = h - sector
    sector = sector.astype(np.int64) % 6
    tab = np.stack([v, v * (1 - s), v * (1 - s * f), v * (1 - s * (1 - f))], axis=-1)
    idx = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]])   # (b, g, r) picks per sector
    pick = idx[sector]
    bgr = np.take_along_axis(tab, pick, axis=-1)
    return np.clip(np.rint(bgr * 255.0), 0, 255).astype(np.uint8)


def flow_to_bgr(flow: np.ndarray) -> np.ndarray:
    return hsv_to_bgr(flow_to_hsv(flow)[0])


_CTX_CACHE_SIZES = 8                 # contexts kept by calcOpticalFlowFarneback, least recently used first
_ctx_cache = {}                      # (W, H, parameters, window) -> Context


def calcOpticalFlowFarneback(prev, next, flow, pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, flags) -> np.ndarray:
    """cv2.calcOpticalFlowFarneback's literal signature on libmavflow: a cv2 argument list passes as it is.  flags: 0,
    OPTFLOW_USE_INITIAL_FLOW (4: `flow` is the starting field), OPTFLOW_FARNEBACK_GAUSSIAN (256: the Gaussian window) or both.
    Returns the float32 (H, W, 2) field (a new array; `flow` is not written).  Contexts are kept per (W, H, parameters, window),
    as im_helpers keeps them per frame size, and only dropped, never closed, when the cache lets go of them."""
    known = _lib.OPTFLOW_USE_INITIAL_FLOW | _lib.OPTFLOW_FARNEBACK_GAUSSIAN
    if int(flags) & ~known:
        raise ValueError(f"flags must be a combination of OPTFLOW_USE_INITIAL_FLOW (4) and OPTFLOW_FARNEBACK_GAUSSIAN (256), got {flags}")
    prev, nxt = np.asarray(prev), np.asarray(next)
    if prev.ndim != 2 or prev.shape != nxt.shape:
        raise ValueError("prev and next must be single-channel images of one size")
    H, W = prev.shape
    window = "gaussian" if int(flags) & _lib.OPTFLOW_FARNEBACK_GAUSSIAN else "box"
    key = (W, H, float(pyr_scale), int(levels), int(winsize), int(iterations), int(poly_n), float(poly_sigma), window)
    ctx = _ctx_cache.pop(key, None)
    if ctx is None or not ctx.alive:
        fb = _lib.fb_defaults()
        fb.pyr_scale, fb.levels, fb.winsize, fb.iterations = float(pyr_scale), int(levels), int(winsize), int(iterations)
        fb.poly_n, fb.poly_sigma, fb.flags = int(poly_n), float(poly_sigma), 0
        ctx = _lib.Context(W, H, 1, fb, window=window)
    _ctx_cache[key] = ctx
    while len(_ctx_cache) > _CTX_CACHE_SIZES:
        _ctx_cache.pop(builtins.next(iter(_ctx_cache)))      # (`next` is cv2's argument name here)
    init = None
    if int(flags) & _lib.OPTFLOW_USE_INITIAL_FLOW:
        if flow is None:
            raise ValueError("OPTFLOW_USE_INITIAL_FLOW needs the starting field in `flow`")
        init = flow
    return np.array(ctx.farneback(prev, nxt, initial_flow=init)[0])


class Farneback:
    PARAMS = dict(pyr_scale=0.4, levels=1, winsize=12, iterations=10, poly_n=8, poly_sigma=1.2, flags=0)

    def __init__(self, capture, output=None, vis: str = "host") -> None:
        """vis="host": the picture is composed in numpy (flow_to_hsv, hsv_to_bgr), the field comes to the host every frame.
        vis="device": process() hands the frame to a pipeline.FlowStage of the context (gray conversion, prevgray and the flow stay on the
        device) and mav_flow_hsv_dev builds the picture where the flow is: one frame goes up, the picture and its 16-byte record come down."""
        if vis not in ("host", "device"):
            raise ValueError(f"vis must be 'host' or 'device', got {vis!r}")
        if vis == "device" and self.PARAMS["flags"] & _lib.OPTFLOW_USE_INITIAL_FLOW:
            raise NotImplementedError("vis='device' with OPTFLOW_USE_INITIAL_FLOW in PARAMS['flags'] is not built: the device path's "
                                      "pipeline.FlowStage has no warm start; use vis='host'")
        self.vis = vis
        self.capture = capture
        self.output = output
        _, prev = self.capture.read()
        H, W = prev.shape[:2]
        fb = _lib.fb_defaults()
        for k, v in self.PARAMS.items():
            setattr(fb, k, v)
        # cv2.OPTFLOW_FARNEBACK_GAUSSIAN in PARAMS["flags"] selects the context's window; mav_create itself takes the bit for an error
        gaussian = bool(fb.flags & _lib.OPTFLOW_FARNEBACK_GAUSSIAN)
        fb.flags &= ~_lib.OPTFLOW_FARNEBACK_GAUSSIAN
        self.ctx = _lib.Context(W, H, 1, fb, window="gaussian" if gaussian else "box")
        self.prevgray = self._gray(prev)
        self.flow = np.zeros((H, W, 2), np.float32)
        self.history_length = 1
        self.prev_result = np.zeros((H, W, 3), np.uint8)
        if vis == "device":
            self._device_init(prev)

    @classmethod
    def from_png_sequence(cls, img_path: str, img_format: str = "image_%05d.png", output=None, vis: str = "host", decoder: str = "host",
                          ahead: int = 64) -> "Farneback":
        """Farneback(cv2.VideoCapture(f'{img_path}/image_%05d.png'), output) with the capture this build provides for PNG sequences
        (frame_source.PngSequenceCapture; src/datasets/dataset.py:38,57).  decoder / ahead: the capture's (decoder="device": the
        files are decoded on the device, `ahead` per call; the frames are the same)."""
        from .frame_source import PngSequenceCapture
        cap = PngSequenceCapture(f"{img_path}/{img_format}", decoder=decoder, ahead=ahead)
        if not cap.isOpened():
            raise OSError(f"no PNG sequence at {img_path}/{img_format}")
        return cls(cap, output, vis)

    def _gray(self, img: np.ndarray) -> np.ndarray:
        return self.ctx.bgr2gray(img)[0] if img.ndim == 3 else np.ascontiguousarray(img, np.uint8)

    def warp_flow(self, img: np.ndarray, flow: np.ndarray) -> np.ndarray:
        """farneback.py:63-69: img (a BGR frame, or any image Context.remap takes) sampled at grid - flow by cv2.remap(INTER_LINEAR) --
        the motion-compensated frame --, the map generated on the device (mav_warp_flow).  flow (H, W, 2) float32, or anything numpy
        converts to it; the caller's array is not negated in place.  Runs on this object's context when the frame is its size, else on a
        cached context of the frame's size."""
        from . import im_helpers, warp  # noqa: F401
        h, w = np.shape(flow)[:2]
        ctx = self.ctx if (w, h) == (self.ctx.W, self.ctx.H) else im_helpers._ctx(w, h)
        return ctx.warp_flow(img, np.asarray(flow, np.float32))

    # ---- vis="device" ----------------------------------------------------------------------------------------------------------------
    def _device_init(self, prev: np.ndarray) -> None:
        from . import vis as _vis                         # (attaches Context.flow_hsv_enqueue)
        from .pipeline import FlowStage
        n = self.ctx.W * self.ctx.H
        self._stage = FlowStage(self.ctx, defer=False)    # the flow is enqueued at once: the picture is enqueued right behind it
        self._stage.flow_next(prev)                       # frame 0: its gray image is the device's prevgray
        self._pic = self.ctx.alloc(16 + (3 * n + 15) // 16 * 16 + 3 * n)     # the record, the BGR picture, the HSV picture (on demand)
        self._hsv_of = None                               # the flow handle whose HSV picture self._hsv holds
        self._hsv = None
        self._record_dtype = _vis.RECORD_DTYPE

    @property
    def hsv(self) -> np.ndarray:
        """The HSV picture of the last frame; in device mode it is rendered when somebody asks for it."""
        if self.vis == "device" and self._hsv_of is not self.flow:
            n = self.ctx.W * self.ctx.H
            off = 16 + (3 * n + 15) // 16 * 16
            if not getattr(self.flow, "on_device", False):
                self._hsv = flow_to_hsv(np.asarray(self.flow))[0]      # the handle has been brought over (or no frame yet): the host's form
            else:
                self.ctx.flow_hsv_enqueue(self.flow, self._pic.ptr + 16, self._pic.ptr, "process", hsv_ptr=self._pic.ptr + off)
                raw = self._pic.download(np.uint8, (self._pic.nbytes,))
                self._hsv = raw[off:off + 3 * n].reshape(self.ctx.H, self.ctx.W, 3)
            self._hsv_of = self.flow
        return self._hsv

    @hsv.setter
    def hsv(self, value) -> None:
        self._hsv = value

    def _process_device(self) -> np.ndarray:
        _, img = self.capture.read()
        n = self.ctx.W * self.ctx.H
        self.flow = self._stage.flow_next(np.asarray(img))            # the frame has been read when this returns
        self.ctx.flow_hsv_enqueue(self.flow, self._pic.ptr + 16, self._pic.ptr, "process")
        raw = self._pic.download(np.uint8, (16 + 3 * n,))              # the record and the BGR picture: all that comes back
        record = raw[:16].view(self._record_dtype)[0]
        result = raw[16:].reshape(self.ctx.H, self.ctx.W, 3)
        if record["invalid"]:
            result = self.prev_result
        self.prev_result = result
        return result

    def close(self) -> None:
        """Device mode: gives the stage's and the picture's device memory back (the context itself goes with the object)."""
        if getattr(self, "_stage", None) is not None:
            self._stage.close()
            self._pic.free()
            self._stage = None

    def draw_hsv(self, flow: np.ndarray) -> np.ndarray:
        """farneback.py:50-60: hue from atan2(fy, fx) + pi, value min(4 |flow|, 255), saturation 255, COLOR_HSV2BGR -- on the device
        (MAV_HSV_DRAW).  flow (H, W, 2) float32; a float64 field is a TypeError (it would round).  Runs on this object's context when
        the field is its size, else on a cached context of the field's size."""
        from . import im_helpers, vis as _vis  # noqa: F401
        h, w = np.shape(flow)[:2]
        ctx = self.ctx if (w, h) == (self.ctx.W, self.ctx.H) else im_helpers._ctx(w, h)
        return ctx.flow_hsv(flow, mode="draw")["bgr"]

    def draw_flow(self, img: np.ndarray, flow: np.ndarray, step: int = 8) -> np.ndarray:
        """farneback.py:28-48: green lines from every step-th pixel whose flow is longer than 1 to where it points, and a dot at the
        pixel; img is drawn into and returned, as cv2.polylines does.  On the device (mav_draw_flow)."""
        from . import im_helpers, vis as _vis  # noqa: F401
        h, w = np.shape(img)[:2]
        ctx = self.ctx if (w, h) == (self.ctx.W, self.ctx.H) else im_helpers._ctx(w, h)
        return ctx.draw_flow(img, flow, step=step, threshold=1.0, color=(0, 255, 0))

    def process(self) -> np.ndarray:
        if self.vis == "device":
            return self._process_device()
        _, img = self.capture.read()
        gray = self._gray(img)
        # with cv2.OPTFLOW_USE_INITIAL_FLOW in PARAMS["flags"] the call (:76-80) hands cv2 the previous result as its starting flow
        # (zeros before the first frame); the default flags = 0 starts from zero
        init = self.flow if self.PARAMS["flags"] & _lib.OPTFLOW_USE_INITIAL_FLOW else None
        self.flow = self.ctx.farneback(self.prevgray, gray, initial_flow=init)[0]
        self.prevgray = gray
        self.hsv, invalid_frame = flow_to_hsv(self.flow)
        result = hsv_to_bgr(self.hsv)
        if invalid_frame:                              # the normalised magnitude sums to 0 (:89): keep the previous result (:97-98)
            result = self.prev_result
        self.prev_result = result
        return result
