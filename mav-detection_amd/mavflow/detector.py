"""Detector -- the Algorithm switch, IMU derotation, the window search (analyze_pyramid, optimize_window) and the global-motion
branch (get_transformation_matrix for HOMOGRAPHY, flow_vec_subtract) of the reference's Detector (src/detector.py:14-202,280-358,
430-433) on libmavflow.  The affine, fundamental and essential-matrix estimators are cv2 RANSAC with a private RNG (unreachable
from run_detection) and are refused by default: get_transformation_matrix says so.  The affine estimator runs with the caller's generator in
.affine_rng (an extra; None: refused as before); flow_vec_subtract takes .aff, user-set as in the reference or set by that fit.  The
fundamental-matrix estimator likewise runs with .fundamental_rng (an extra; None: refused as before) and gives epipolar_residual its
matrix; the essential-matrix estimator -- the reference's default -- runs with .essential_rng (an extra; None: refused as before) on
Nister's five-point solver (include/mavflow_essential.h), sets .essential for get_rotation and gives epipolar_residual its matrix too."""
from __future__ import annotations

from enum import Enum
from typing import Any, Tuple

import numpy as np

from . import im_helpers, utils
from ._lib import MOTION_DTYPE as _MOTION_DTYPE, check as _lib_check
from .frame_result import FrameResult

_MOTION_BYTES = _MOTION_DTYPE.itemsize


class LucasKanade:
    """The reference's sparse tracker (lucas_kanade.py:9-63): Shi-Tomasi corners, re-detected when fewer than a third of the budget
    remain, tracked from frame to frame by pyramidal Lucas-Kanade -- both on libmavflow (Context.good_features / lk_track).
    The constructor keeps the reference's fields and its one draw from the global RNG and touches no GPU; the device context (one of
    its own: it holds the previous frame and its pyramid between calls) comes with the first get_features."""

    def __init__(self, old_frame: np.ndarray) -> None:
        self.old_frame = old_frame
        self.num_corners = 2000
        self.minimum_num_corners = self.num_corners // 3
        self.total_num_corners = self.num_corners + self.minimum_num_corners
        self.corners = np.zeros((self.total_num_corners, 2), dtype=np.uint)
        self.num_features = 0
        self.features: list = []
        self.feature_params = dict(maxCorners=self.num_corners, qualityLevel=0.2, minDistance=7, blockSize=7)
        # criteria: cv2.TERM_CRITERIA_EPS | cv2.TERM_CRITERIA_COUNT = 3
        self.lk_params = dict(winSize=(21, 21), criteria=(3, 30, 0.01))
        self.color = np.random.randint(0, 255, (self.total_num_corners, 3))
        self._ctx = None
        self._resident = None           # the gray frame the context holds (the `frame` of the previous call)

    def _context(self, H: int, W: int):
        from . import _lib
        if self._ctx is None or not self._ctx.alive or (self._ctx.W, self._ctx.H) != (W, H):
            self._ctx, self._resident = _lib.Context(W, H, 1), None
        return self._ctx

    def get_features(self, frame: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """LK optical flow from the previous frame to `frame` (BGR): (old_features (n, 2) float32, good_new (n, 2) float32,
        status (n, 1) uint8), cv2's shapes.  Every feature is tracked whatever its last status and .features becomes the tracked
        points; new corners are appended when fewer than minimum_num_corners features remain.  An all-black previous frame returns
        three empty arrays.  Each frame crosses to the device once as a gray image: the previous call's `frame` is still there
        (recognised by identity -- a frame changed in place after it was handed in is not noticed: assign a new array to
        .old_frame instead)."""
        H, W = np.shape(self.old_frame)[:2]
        self.mask = np.zeros_like(self.old_frame)
        ctx = self._context(H, W)
        frame_gray = ctx.bgr2gray(np.asarray(frame))[0]
        held = self._resident is not None and self._resident[0] is self.old_frame         # the context holds old_gray already
        self.old_gray = self._resident[1] if held else ctx.bgr2gray(np.asarray(self.old_frame).astype(np.uint8))[0]
        self.old_frame = frame
        self._resident = None

        if np.sum(self.old_gray) < 1:
            return np.zeros(0), np.zeros(0), np.zeros(0)

        if len(self.features) < self.minimum_num_corners:
            new_features = ctx.good_features(None if held else self.old_gray, mask=None, **self.feature_params)
            held = True
            for feature in new_features:
                self.features.append(feature)

        old_features = np.array(self.features).astype(np.float32).reshape(-1, 2)
        good_new, status = ctx.lk_track(None if held else self.old_gray, frame_gray, old_features, **self.lk_params)
        self.features = good_new.tolist()
        self._resident = (frame, frame_gray)
        return old_features, good_new, status.reshape(-1, 1)


class Detector:
    class Algorithm(Enum):
        NONE = 0,
        FOE = 1,
        AFFINE = 2,
        HOMOGRAPHY = 3,
        FUNDAMENTAL = 4,
        ESSENTIAL = 5,

    def __init__(self, dataset, algorithm: "Detector.Algorithm" = None, use_sparse_of: bool = False) -> None:
        self.dataset = dataset
        self.algorithm = Detector.Algorithm.ESSENTIAL if algorithm is None else algorithm
        self.use_sparse_of = use_sparse_of
        W, H = self.dataset.capture_size[0], self.dataset.capture_size[1]
        self.sample_size = 1000
        self.border_offset = 20
        # same draws, same order as the reference's constructor (keeps a seeded global RNG stream aligned)
        self.sample_y = np.random.randint(self.border_offset, H - self.border_offset, self.sample_size)
        self.sample_x = np.random.randint(self.border_offset, W - self.border_offset, self.sample_size)
        self.coords = np.column_stack((self.sample_x, self.sample_y))
        self.confidence = 0
        self.prev_frame = np.zeros((H, W, 3), dtype=np.uint8)
        self.lucas_kanade = LucasKanade(self.prev_frame)
        self.fov = 90
        self.focal_length = 1 / np.tan(np.deg2rad(self.fov) / 2)
        self.frame_result = FrameResult()
        self.use_optimization = False
        self._gm_dev = None              # (context, device buffers) of the calls that take a device-resident flow field
        # get_history (detector.py:30-36): the reference allocates two (20, H, W, 2) host arrays here; the ring lives on the device and
        # is made by the first get_history call
        self.history_length = 20
        self._history = None
        # clustering (detector.py:396-428): off in flow_vec_subtract, as the reference's commented-out line leaves it
        self.use_clustering = False
        self.cluster_rng = None          # the generator of clustering's initial centres (None: np.random)
        # an extra: the generator of the AFFINE fit's sample triples (a seed, a Generator or np.random).  None: get_transformation_matrix
        # refuses AFFINE as before
        self.affine_rng = None
        # an extra: the generator of the FUNDAMENTAL fit's sample subsets, likewise.  None: FUNDAMENTAL is refused as before
        self.fundamental_rng = None
        # an extra: the generator of the ESSENTIAL fit's sample subsets, likewise.  None: ESSENTIAL is refused as before
        self.essential_rng = None
        self.mag_handle = self.gray_handle = None    # flow_uv_warped_mag / one channel of to_rgb(magnitude) on the device, after a flow_vec_subtract of a device flow

    def get_gradient_and_magnitude(self, frame: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        """Polar form of a cartesian flow field (detector.py:53-63): (magnitude, angle)."""
        return np.sqrt(frame[..., 0] ** 2.0 + frame[..., 1] ** 2.0), np.arctan2(frame[..., 1], frame[..., 0])

    def derotate(self, previous_frame_index: int, current_frame_index: int, flow_uv: np.ndarray) -> np.ndarray:
        """Subtract the rotational flow predicted from the IMU rates; float64 out.  Frame 0 is returned untouched."""
        if current_frame_index < 1:
            return flow_uv
        dt = self.dataset.get_delta_time(current_frame_index)
        omega = np.asarray(self.dataset.get_angular_difference(previous_frame_index, current_frame_index), np.float64) / dt
        W, H = self.dataset.capture_size[0], self.dataset.capture_size[1]
        flow_uv = np.asarray(flow_uv)
        if flow_uv.dtype != np.float32:
            # a float64 field (no dataset of the reference produces one: .flo files and Farneback are float32) keeps its precision:
            # the reference's own numpy arithmetic on the host, not the float32-input kernel
            rows, cols = np.mgrid[0:flow_uv.shape[0], 0:flow_uv.shape[1]]
            return self.derotate_at(previous_frame_index, current_frame_index, flow_uv.astype(np.float64, copy=False), rows, cols)
        return im_helpers._ctx(W, H).derotate(flow_uv, omega, dt)[0]

    def derotate_at(self, previous_frame_index: int, current_frame_index: int, flow_values: np.ndarray, rows: np.ndarray,
                    cols: np.ndarray) -> np.ndarray:
        """derotate() restricted to the pixels (rows[k], cols[k]) whose flow vectors are flow_values[k]: the correction is
        pointwise, so selecting first and derotating after gives the values the reference gets by derotating the whole field
        and selecting (processor.py:310,343-345 need the ground-truth flow at the few hundred drone pixels only).  Host numpy in
        the reference's operation order (detector.py:83-117); float64 out, frame 0 untouched."""
        if current_frame_index < 1:
            return flow_values
        dt = self.dataset.get_delta_time(current_frame_index)
        w, h = self.dataset.capture_size[0], self.dataset.capture_size[1]
        omega = np.asarray(self.dataset.get_angular_difference(previous_frame_index, current_frame_index), np.float64) / dt
        x = -(np.asarray(cols) / w - 0.5) * 2.0
        y = -(np.asarray(rows) / h - 0.5) * 2.0
        du = +omega[0] * x * y - omega[1] * x ** 2 - omega[1] + omega[2] * y
        dv = -omega[2] * x + omega[0] + omega[0] * y ** 2 - omega[1] * x * y
        du = du * (w * dt / 2)
        dv = dv * (h * dt / 2)
        return flow_values - np.stack([du, dv], axis=-1)

    @staticmethod
    def _gray_of(img: np.ndarray, who: str):
        a = np.asarray(img)
        if a.dtype != np.uint8:
            raise TypeError(f"{who} expects the u8 image im_helpers.to_rgb produces")
        if a.ndim == 3:
            if not (np.array_equal(a[..., 0], a[..., 1]) and np.array_equal(a[..., 0], a[..., 2])):
                raise ValueError(f"{who}: 3-channel input must be a gray replica (im_helpers.to_rgb)")
            return a, np.ascontiguousarray(a[..., 0]), 1
        return a, a, 3

    @staticmethod
    def _window_tuple(ctx, record, gray: np.ndarray, three: bool) -> Tuple[float, utils.Rectangle, np.ndarray, Any]:
        """analyze_pyramid's 4-tuple from the device's record (score, x, y, level, argmax row, argmax col) of the u8 image `gray`;
        three: the image handed in had three (equal) channels."""
        score, x, y, level, ay, ax = (int(v) for v in record)
        if score == 0:
            return (0, utils.Rectangle((0, 0), (0, 0)), np.zeros(0), 0)
        lv = gray if level == 0 else ctx.pyramid_level(gray, level)
        window = lv[y:y + 64, x:x + 64]
        if three:
            window = np.repeat(window[..., None], 3, axis=2)
        return (score // (1 if three else 3), utils.Rectangle((x, y), (64, 64)), window, (ay, ax, 0) if three else (ay, ax))

    def analyze_pyramid(self, img: np.ndarray) -> Tuple[float, utils.Rectangle, np.ndarray, Any]:
        """Highest-sum 64x64 window (stride 16, first maximum wins) over every pyramid level (scale 1.5, INTER_AREA).
        Returns (score, Rectangle, window, argmax inside the window) like the reference (detector.py:280-312): the
        rectangle is in the winning level's own coordinates and `window` is that level's sub-image."""
        a, gray, mult = self._gray_of(img, "analyze_pyramid")
        H, W = gray.shape
        ctx = im_helpers._ctx(W, H)
        return self._window_tuple(ctx, ctx.analyze_pyramid(gray)[0], gray, a.ndim == 3)

    def optimize_window(self, mag_img: np.ndarray, window: utils.Rectangle) -> Tuple[float, utils.Rectangle]:
        """Greedy corner walk of detector.py:314-358 (the window grows / shrinks while the enclosed sum rises)."""
        a, gray, mult = self._gray_of(mag_img, "optimize_window")
        H, W = gray.shape
        win = [int(window.get_left()), int(window.get_top()), int(window.get_right()) - int(window.get_left()),
               int(window.get_bottom()) - int(window.get_top())]
        score, out = im_helpers._ctx(W, H).optimize_window(gray, [win])
        if int(score[0]) == 0:
            return (0.0, window)
        x, y, w, h = (int(v) for v in out[0])
        return (float(int(score[0]) // mult), utils.Rectangle.from_points((x, y), (x + w, y + h)))

    # -- global-motion subtraction (detector.py:119-202) ----------------------------------------------------------------------------
    def _device_flow(self, flow_uv):
        """(context, device pointer) of a float32 flow handle from the flow seam that is still on the device, else None."""
        from . import pipeline
        if not (isinstance(flow_uv, pipeline.DeviceArray) and flow_uv.on_device and flow_uv.dtype == np.float32 and flow_uv.ctx.alive):
            return None
        if flow_uv._deferred is not None:              # the flow stage has not enqueued it yet
            flow_uv._deferred.flush()
        return flow_uv.ctx, flow_uv.ptr

    def _dev_buffers(self, ctx) -> dict:
        """Device buffers (on the flow's context) of the calls that take a device-resident field: allocated once per context."""
        if self._gm_dev is None or self._gm_dev[0] is not ctx:
            self._free_dev_buffers()
            n0 = ctx.W * ctx.H
            sizes = dict(H=72, ok=4, M=48, res=_MOTION_BYTES, gray=n0, warped=8 * n0, mag=4 * n0)
            self._gm_dev = (ctx, {k: ctx.alloc(v) for k, v in sizes.items()})
        return self._gm_dev[1]

    def _free_dev_buffers(self) -> None:
        if self._gm_dev is not None:
            ctx, bufs = self._gm_dev
            self._gm_dev = None
            if ctx.alive:
                for b in bufs.values():
                    b.free()

    def get_transformation_matrix(self, orig_frame: np.ndarray, flow_uv: np.ndarray) -> None:
        """The homography of detector.py:119-139: 1000 sampled pairs coords -> coords + flow[y, x] (or, with use_sparse_of, the
        Lucas-Kanade tracks of orig_frame when there are any), fitted on the device in the structure of cv2.findHomography's method 0
        (Context.find_homography: not pinned against cv2).  Sets .homography (3x3 float64) and .confidence (the all-ones inlier mask,
        (n, 1) uint8); RuntimeError when the pairs determine no homography.  flow_uv: a host array or the flow seam's device handle.
        AFFINE with .affine_rng set: _affine_matrix (sets .aff and .aff_inliers); FUNDAMENTAL with .fundamental_rng set:
        _fundamental_matrix (sets .fundamental and .fundamental_inliers); ESSENTIAL with .essential_rng set: _essential_matrix (sets
        .essential, .essential_inliers and .essential_F); with its generator None each of the three raises."""
        A = Detector.Algorithm
        affine = self.algorithm == A.AFFINE and self.affine_rng is not None
        if self.algorithm == A.FUNDAMENTAL and self.fundamental_rng is not None:
            return self._fundamental_matrix(orig_frame, flow_uv)
        if self.algorithm == A.ESSENTIAL and self.essential_rng is not None:
            return self._essential_matrix(orig_frame, flow_uv)
        if self.algorithm in (A.AFFINE, A.FUNDAMENTAL, A.ESSENTIAL) and not affine:
            raise NotImplementedError(
                f"{self.algorithm.name}: cv2.estimateAffine2D / findFundamentalMat / findEssentialMat are RANSAC estimators driven by "
                "OpenCV's private RNG; they are not reproduced (run_detection reaches HOMOGRAPHY only)")
        if affine:
            return self._affine_matrix(orig_frame, flow_uv)
        if self.algorithm != A.HOMOGRAPHY:
            return
        W, H = self.dataset.capture_size[0], self.dataset.capture_size[1]
        pairs = None
        if self.use_sparse_of:
            old, new, _ = self.lucas_kanade.get_features(orig_frame)
            if len(old) > 0 and len(new) > 0:
                pairs = (np.asarray(old, np.float64), np.asarray(new, np.float64))
                logger = getattr(self.dataset, "logger", None)
                if logger is not None:
                    logger.info(f"features: {len(new)}")
        dev = None if pairs is not None else self._device_flow(flow_uv)
        if pairs is not None:
            Hm, ok = im_helpers._ctx(W, H).find_homography(*pairs)
            n = len(pairs[0])
        elif dev is not None:
            ctx, ptr = dev
            b = self._dev_buffers(ctx)
            coords = ctx._coords(self.coords)
            _lib_check(ctx.lib.mav_flow_homography_dev(ctx.h, ptr, coords.ctypes.data, coords.shape[0], 1, b["H"].ptr, b["ok"].ptr))
            Hm, ok = b["H"].download(np.float64, (1, 3, 3)), b["ok"].download(np.int32, (1,))
            n = coords.shape[0]
        else:
            flow = np.asarray(flow_uv)
            n = self.coords.shape[0]
            if flow.dtype == np.float32:
                Hm, ok = im_helpers._ctx(W, H).flow_homography(flow, self.coords)
            else:                                       # a float64 field keeps its precision: the reference's own pair arithmetic
                new = self.coords.astype(np.float64) + flow[self.sample_y, self.sample_x]
                Hm, ok = im_helpers._ctx(W, H).find_homography(self.coords.astype(np.float64), new)
        if not int(ok[0]):
            raise RuntimeError("get_transformation_matrix: the point pairs do not determine a homography")
        self.homography = np.array(Hm[0])
        self.confidence = np.ones((n, 1), np.uint8)

    def _affine_matrix(self, orig_frame: np.ndarray, flow_uv: np.ndarray) -> None:
        """detector.py:141-143 with .affine_rng set (an extra): cv2.estimateAffine2D(coords_old, coords_new)'s RANSAC fit on the device
        (include/mavflow_affine.h: not pinned against cv2), the sample triples drawn from .affine_rng by affine.sample_triples, on the
        same three pair sources as HOMOGRAPHY.  Sets .aff (2x3 float64) and .aff_inliers ((n, 1) uint8); RuntimeError when no valid
        hypothesis had more than two inliers."""
        W, H = self.dataset.capture_size[0], self.dataset.capture_size[1]
        pairs = None
        if self.use_sparse_of:
            old, new, _ = self.lucas_kanade.get_features(orig_frame)
            if len(old) > 0 and len(new) > 0:
                pairs = (np.asarray(old, np.float64), np.asarray(new, np.float64))
        dev = None if pairs is not None else self._device_flow(flow_uv)
        if pairs is not None:
            out = im_helpers._ctx(W, H).estimate_affine(*pairs, rng=self.affine_rng)
        elif dev is not None:
            out = dev[0].flow_affine(flow_uv, self.coords, rng=self.affine_rng)           # the field is read where it is
        else:
            flow = np.asarray(flow_uv)
            if flow.dtype == np.float32:
                out = im_helpers._ctx(W, H).flow_affine(flow, self.coords, rng=self.affine_rng)
            else:                                       # a float64 field keeps its precision: the reference's own pair arithmetic
                new = self.coords.astype(np.float64) + flow[self.sample_y, self.sample_x]
                out = im_helpers._ctx(W, H).estimate_affine(self.coords.astype(np.float64), new, rng=self.affine_rng)
        if not out["ok"]:
            raise RuntimeError("get_transformation_matrix: the point pairs do not determine an affine map")
        self.aff = np.array(out["M"])
        self.aff_inliers = np.array(out["inliers"]).reshape(-1, 1)

    def _fundamental_matrix(self, orig_frame: np.ndarray, flow_uv: np.ndarray) -> None:
        """detector.py:144-146 with .fundamental_rng set (an extra): cv2.findFundamentalMat(coords_old, coords_new, cv2.FM_RANSAC, 0.999,
        1.0)'s RANSAC fit on the device (include/mavflow_fundamental.h: not pinned against cv2), the sample subsets drawn from
        .fundamental_rng by fundamental.sample_subsets, on the same three pair sources as HOMOGRAPHY and AFFINE.  The reference's literal
        arguments are swapped -- cv2's order is (threshold, confidence) -- so the threshold is 0.999 pixels and the confidence 1.0, which
        cv2's argument repair turns into 0.99; both are taken as cv2 would take them.  Sets .fundamental (3x3 float64, scaled to
        F[2, 2] = 1 as cv2 returns it) and .fundamental_inliers ((n, 1) uint8); RuntimeError when no valid model had more than six
        inliers."""
        from . import fundamental as fm
        W, H = self.dataset.capture_size[0], self.dataset.capture_size[1]
        threshold, confidence = fm.repaired(0.999, 1.0)
        kw = dict(threshold=threshold, confidence=confidence, rng=self.fundamental_rng)
        pairs = None
        if self.use_sparse_of:
            old, new, _ = self.lucas_kanade.get_features(orig_frame)
            if len(old) > 0 and len(new) > 0:
                pairs = (np.asarray(old, np.float64), np.asarray(new, np.float64))
        dev = None if pairs is not None else self._device_flow(flow_uv)
        if pairs is not None:
            out = im_helpers._ctx(W, H).find_fundamental(*pairs, **kw)
        elif dev is not None:
            out = dev[0].flow_fundamental(flow_uv, self.coords, **kw)                   # the field is read where it is
        else:
            flow = np.asarray(flow_uv)
            if flow.dtype == np.float32:
                out = im_helpers._ctx(W, H).flow_fundamental(flow, self.coords, **kw)
            else:                                       # a float64 field keeps its precision: the reference's own pair arithmetic
                new = self.coords.astype(np.float64) + flow[self.sample_y, self.sample_x]
                out = im_helpers._ctx(W, H).find_fundamental(self.coords.astype(np.float64), new, **kw)
        if not out["ok"]:
            raise RuntimeError("get_transformation_matrix: the point pairs do not determine a fundamental matrix")
        self.fundamental = fm.scaled(out["F"])
        self.fundamental_inliers = np.array(out["inliers"]).reshape(-1, 1)

    def _essential_matrix(self, orig_frame: np.ndarray, flow_uv: np.ndarray) -> None:
        """detector.py:147-151 with .essential_rng set (an extra): cv2.findEssentialMat(coords_old, coords_new, self.focal_length,
        (0, 0), cv2.FM_RANSAC, 0.999, 1.0)'s RANSAC fit on the device (include/mavflow_essential.h: Nister's five-point solver, not pinned
        against cv2), the sample subsets drawn from .essential_rng by essential.sample_subsets, on the same pair sources as FUNDAMENTAL.
        The reference's literal arguments are kept: the focal length 1 / tan(fov / 2) and the principal point (0, 0) on pixel
        coordinates, prob 0.999, threshold 1.0.  Sets .essential (3x3 float64 of unit Frobenius norm), .essential_inliers ((n, 1) uint8)
        and .essential_F (K^-T E K^-1, what epipolar_residual reads); RuntimeError when no valid model had more than four inliers."""
        W, H = self.dataset.capture_size[0], self.dataset.capture_size[1]
        f = float(self.focal_length)
        kw = dict(threshold=1.0, confidence=0.999, rng=self.essential_rng, camera=(f, f, 0.0, 0.0))
        pairs = None
        if self.use_sparse_of:
            old, new, _ = self.lucas_kanade.get_features(orig_frame)
            if len(old) > 0 and len(new) > 0:
                pairs = (np.asarray(old, np.float64), np.asarray(new, np.float64))
        dev = None if pairs is not None else self._device_flow(flow_uv)
        if pairs is not None:
            out = im_helpers._ctx(W, H).find_essential(*pairs, **kw)
        elif dev is not None:
            out = dev[0].flow_essential(flow_uv, self.coords, **kw)                     # the field is read where it is
        else:
            flow = np.asarray(flow_uv)
            if flow.dtype == np.float32:
                out = im_helpers._ctx(W, H).flow_essential(flow, self.coords, **kw)
            else:                                       # a float64 field keeps its precision: the reference's own pair arithmetic
                new = self.coords.astype(np.float64) + flow[self.sample_y, self.sample_x]
                out = im_helpers._ctx(W, H).find_essential(self.coords.astype(np.float64), new, **kw)
        if not out["ok"]:
            raise RuntimeError("get_transformation_matrix: the point pairs do not determine an essential matrix")
        self.essential = np.array(out["E"])
        self.essential_inliers = np.array(out["inliers"]).reshape(-1, 1)
        self.essential_F = np.array(out["F"])

    def get_rotation(self, flow_uv: np.ndarray, use_fundamental: bool = True) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """detector.py:65-68: (euler(R1), euler(R2), t) of .essential's decomposition (essential.decomposeEssentialMat on the host: R1's
        and R2's order and t's sign are not pinned against cv2), the Euler angles in degrees by utils.rotation_matrix_to_euler; t is
        (3, 1).  Both arguments are ignored, as in the reference."""
        from . import essential as em
        R1, R2, t = em.decomposeEssentialMat(self.essential)
        return utils.rotation_matrix_to_euler(R1), utils.rotation_matrix_to_euler(R2), t

    def epipolar_residual(self, flow_uv, threshold: float = 1.0) -> Tuple[np.ndarray, np.ndarray]:
        """An extra: (residual (H, W) float32, mask (H, W) uint8 0/255) of the dense epipolar residual of flow_uv under .fundamental
        (for ESSENTIAL: under .essential_F, the fitted essential matrix in pixel coordinates) (Context.epipolar_residual): per pixel the distance of p + flow(p) from the epipolar line of p; the mask marks what moves off its
        line by more than `threshold` pixels -- an independent mover, whatever the scene's depth.  flow_uv: a float32 host array or the
        flow seam's device handle, on whose context the pass runs."""
        Fm = np.asarray(self.essential_F if self.algorithm == Detector.Algorithm.ESSENTIAL else self.fundamental, np.float64)
        dev = self._device_flow(flow_uv)
        if dev is not None:
            out = dev[0].epipolar_residual(flow_uv, Fm, threshold)
        else:
            W, H = self.dataset.capture_size[0], self.dataset.capture_size[1]
            out = im_helpers._ctx(W, H).epipolar_residual(np.asarray(flow_uv, np.float32), Fm, threshold)
        return out["residual"], out["mask"]

    def flow_vec_subtract(self, orig_frame: np.ndarray, flow_uv: np.ndarray) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
        """detector.py:153-202: the motion the matrix predicts (.homography for HOMOGRAPHY, else a user-set .aff) is subtracted from
        the field, the residual's magnitude becomes cluster_vis and the window search runs on it (optimize_window too with
        .use_optimization).  A float32 field -- host array or the flow seam's device handle -- goes through mav_global_motion; any other
        dtype takes the reference's numpy arithmetic on the host, as derotate does.  Returns (get_flow_vis(flow_uv_warped),
        cluster_vis, to_rgb(magnitude), get_flow_vis(global_motion)) and sets flow_uv_warped, flow_uv_warped_mag, flow_max, cluster_vis,
        opt_window, iou, flow_uv_warped_vis, prev_frame, frame_result.  With .use_clustering (an extra, off by default) cluster_vis and
        the second return are clustering(flow_uv_warped_mag)'s image instead."""
        self.frame_result = FrameResult()
        M = np.asarray(self.homography if self.algorithm == Detector.Algorithm.HOMOGRAPHY else self.aff, np.float64)
        W, H = self.dataset.capture_size[0], self.dataset.capture_size[1]
        dev = self._device_flow(flow_uv)
        host = None if dev is not None else np.asarray(flow_uv)
        if dev is None and host.dtype != np.float32:
            x_coords = np.tile(np.arange(W), (H, 1))
            y_coords = np.tile(np.arange(H), (W, 1)).T
            global_motion = np.zeros_like(host)
            global_motion[..., 0] = M[0, 0] * x_coords + M[0, 1] * y_coords + M[0, 2] - x_coords
            global_motion[..., 1] = M[1, 0] * x_coords + M[1, 1] * y_coords + M[1, 2] - y_coords
            self.flow_uv_warped = global_motion - host
            flow_uv_warped_vis = im_helpers.get_flow_vis(self.flow_uv_warped)
            self.flow_uv_warped_mag = np.sqrt(self.flow_uv_warped[..., 0] ** 2.0 + self.flow_uv_warped[..., 1] ** 2.0)
            self.flow_max = np.unravel_index(self.flow_uv_warped_mag.argmax(), self.flow_uv_warped_mag.shape)
            with np.errstate(invalid="ignore", divide="ignore"):
                self.cluster_vis = im_helpers.to_rgb(self.flow_uv_warped_mag)
            self.opt_window = self.analyze_pyramid(self.cluster_vis)
            window_optimized = self.opt_window[1]
            if self.use_optimization:
                window_optimized = self.optimize_window(self.cluster_vis, self.opt_window[1])[1]
            global_motion_vis = im_helpers.get_flow_vis(global_motion)
        else:
            if dev is not None:
                ctx, ptr = dev
                b = self._dev_buffers(ctx)
                b["M"].upload(np.ascontiguousarray(M[:2, :]))
                _lib_check(ctx.lib.mav_global_motion_dev(ctx.h, ptr, b["M"].ptr, 1, 1.5, int(bool(self.use_optimization)), b["warped"].ptr,
                                                         b["mag"].ptr, b["gray"].ptr, b["res"].ptr))
                imgs = ctx.render_last_global_motion(1)
                rec = b["res"].download(_MOTION_DTYPE, (1,))[0]
                gray = b["gray"].download(np.uint8, (H, W))
                self.flow_uv_warped = b["warped"].download(np.float32, (H, W, 2))
                self.flow_uv_warped_mag = b["mag"].download(np.float32, (H, W))
                from .clustering import DeviceSamples
                self.mag_handle, self.gray_handle = DeviceSamples(ctx, b["mag"].ptr, (H, W), np.float32), DeviceSamples(ctx, b["gray"].ptr, (H, W), np.uint8)
            else:
                ctx = im_helpers._ctx(W, H)
                out = ctx.global_motion(host, M, optimize=self.use_optimization, outputs=("warped", "mag", "gray"))
                imgs = ctx.render_last_global_motion(1)
                rec, gray = out["results"][0], out["gray"][0]
                self.flow_uv_warped, self.flow_uv_warped_mag = out["warped"][0], out["mag"][0]
            flow_uv_warped_vis, global_motion_vis = imgs["warped"][0], imgs["global"][0]
            self.flow_max = (int(rec["max_row"]), int(rec["max_col"]))
            self.cluster_vis = np.repeat(gray[..., None], 3, axis=2)
            self.opt_window = self._window_tuple(ctx, rec["window"], gray, True)
            x, y, w, h = (int(v) for v in rec["opt_window"])
            window_optimized = utils.Rectangle.from_points((x, y), (x + w, y + h)) if self.use_optimization else self.opt_window[1]
        if self.use_optimization:
            opt_window_list = list(self.opt_window)
            opt_window_list[1] = window_optimized
            self.opt_window = tuple(opt_window_list)
        for gt in getattr(self.dataset, "ground_truth", []):
            self.iou = utils.Rectangle.calculate_iou(window_optimized, gt)
        self.flow_uv_warped_vis = flow_uv_warped_vis
        self.prev_frame = orig_frame
        if dev is None:
            self.mag_handle = self.gray_handle = None
        if self.use_clustering:
            # the reference's commented-out line (detector.py:182): cluster_vis is clustering's image of the residual magnitude.  The
            # window search above stays on the magnitude's grey image (clustering's rgb is no grey replica: channel 1 is cleared under its mask)
            magnitude_vis = self.cluster_vis
            self.cluster_vis, _ = self.clustering(self.mag_handle if dev is not None else self.flow_uv_warped_mag)
            return flow_uv_warped_vis, self.cluster_vis, magnitude_vis.copy(), global_motion_vis
        return flow_uv_warped_vis, self.cluster_vis, self.cluster_vis.copy(), global_motion_vis

    # -- drawing (detector.py:242-256, 390-394) ---------------------------------------------------------------------------------------
    def ground_truth_shapes(self, image: int = 0) -> list:
        """draw's rectangles as records of a shapes table: every ground-truth box in red, thickness 2"""
        from . import shapes
        return [shapes.shape(shapes.RECT, *gt.get_topleft_int(), *gt.get_bottomright_int(), 2, (0, 0, 255), image)
                for gt in getattr(self.dataset, "ground_truth", [])]

    def draw(self, orig_frame: np.ndarray) -> None:
        """Render the ground truths (:242-256): cv2.rectangle(orig_frame, topleft, bottomright, (0, 0, 255), 2) for every ground-truth
        box, into orig_frame in place -- one table, one call (Context.draw_shapes)."""
        table = self.ground_truth_shapes()
        if table:
            im_helpers._ctx(orig_frame.shape[1], orig_frame.shape[0]).draw_shapes(orig_frame, table)

    def predict(self, segment: np.ndarray, flow_uv: np.ndarray, orig_frame: np.ndarray) -> None:
        """:390-394: the mean flow over `segment` (numpy, as the reference has it) moves the first ground-truth box's centre to
        self.prediction; the line between the two, red, thickness 5, is drawn into orig_frame in place."""
        from . import shapes
        avg = np.average(flow_uv[segment], 0)
        center = self.dataset.ground_truth[0].get_center_int()
        self.prediction = (int(center[0] + avg[0]), int(center[1] + avg[1]))
        shapes.line(orig_frame, center, self.prediction, (0, 0, 255), 5)

    # -- flow history (detector.py:365-388) -----------------------------------------------------------------------------------------
    @property
    def history_index(self) -> int:
        """The ring slot the next field goes to (0 before the first call)."""
        return self._history.index if self._history is not None else 0

    def get_history(self, flow_uv: np.ndarray) -> np.ndarray:
        """detector.py:365-388: the field is stored in the ring of the last history_length fields and every pixel's trajectory is
        followed through them by chained bilinear lookups (Context.flow_history: cv2.remap restated, not pinned against cv2).
        Returns the accumulated displacement, float64 (H, W, 2) in the reference's channel order.  flow_uv: a host array or the flow
        seam's device handle.  The ring is made by the first call, on the handle's context or the shared one of this frame size, with
        the element type of that first field (float32, or float64 for a float64 array) and kept until history_length changes or its
        context is closed (then a new, zero ring starts); a float64 field into a float32 ring would round and is a ValueError."""
        W, H = self.dataset.capture_size[0], self.dataset.capture_size[1]
        hist = self._history
        if hist is not None and (hist.length != int(self.history_length) or not hist.ctx.alive):
            hist.close()
            hist = self._history = None
        dev = self._device_flow(flow_uv)
        if dev is None or (hist is not None and dev[0] is not hist.ctx):      # a handle of another context is read through the host
            flow_uv = np.asarray(flow_uv)
            if flow_uv.dtype not in (np.float32, np.float64):
                flow_uv = flow_uv.astype(np.float64)
            dev = None
        if hist is None:
            ctx = dev[0] if dev is not None else im_helpers._ctx(W, H)
            hist = self._history = ctx.flow_history(int(self.history_length), flow_uv.dtype, "reference")
        return hist.push(flow_uv, out="reference")

    # -- clustering (detector.py:396-428) -------------------------------------------------------------------------------------------
    def clustering(self, img: np.ndarray, enable_raw: bool = False) -> Tuple[np.ndarray, np.ndarray]:
        """detector.py:396-428: k-means (K = 8, 10 attempts, criteria (EPS | MAX_ITER, 10, 1.0), random centres) of the image's values
        taken three at a time -- the reference's reshape((-1, 3)); a size not divisible by 3 is numpy's ValueError --, every value
        replaced by its centre scaled to 0..255.  Returns (res, zeros(0)) with enable_raw, else (rgb, mask): res repeated to three channels
        with channel 1 cleared where res >= 225.  img: a host array (float32 and uint8 as they are, anything else as float32, the
        reference's astype) or a device handle with .ptr, .shape, .dtype and .ctx (the mag / gray of a global-motion call on the flow's
        context: .mag_handle, .gray_handle), clustered where it is.  The centres are drawn from .cluster_rng (None: np.random, the global
        generator the reference's other draws use) by clustering.random_centers, not by OpenCV's private generator: the result equals no
        cv2 run sample for sample (include/mavflow_cluster.h)."""
        from . import clustering as _cl
        if hasattr(img, "ptr") and getattr(img, "on_device", True) and getattr(getattr(img, "ctx", None), "alive", False):
            shape = tuple(img.shape)
            np.empty(shape, np.uint8).reshape((-1, 3))                    # numpy's ValueError for a size not divisible by 3
            n = int(np.prod(shape)) // 3
            ctx = img.ctx
            samples = _cl.DeviceSamples(ctx, img.ptr, (n, 3), img.dtype)
        else:
            a = np.asarray(img)
            shape = a.shape
            z = a.reshape((-1, 3))
            samples = np.ascontiguousarray(z if z.dtype in (np.float32, np.uint8) else z.astype(np.float32))
            ctx = _cl.context_for(z.size)
        out = ctx.kmeans(samples, K=8, attempts=10, max_iter=10, eps=1.0, rng=np.random if self.cluster_rng is None else self.cluster_rng)
        res = ctx.kmeans_paint(out["labels"], out["centers"])[0].reshape(shape)
        if enable_raw:
            return res, np.zeros(0)
        rgb = np.repeat(res[..., None], 3, axis=-1)
        mask = rgb[..., 0] >= 225
        rgb[mask, 1] = 0
        return rgb, mask

    # -- warp method (detector.py:204-240) --------------------------------------------------------------------------------------------
    def warp_method(self, flow_uv: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        """detector.py:204-240, the reference's second way of removing global motion: the field warped by the matrix (.homography for
        HOMOGRAPHY through warpPerspective, else a user-set .aff through warpAffine), subtracted from the field -- elements whose warped
        value is 0 count as equal --, the difference's magnitude.  Returns (get_flow_vis(flow_diff), to_rgb(flow_diff_mag)) and sets
        .flow_diff_mag (and .flow_diff, .flow_diff_max = (row, col) of the largest magnitude, which the reference computes and drops).
        flow_uv: a host array or the flow seam's device handle, on whose context the call then runs.  A float32 field goes through
        mav_warp_method; any other dtype takes the reference's arithmetic on the host with mavflow.warp.warpPerspective / warpAffine
        on a float32 COPY of the field -- which rounds it: the warp is built for float32 alone.  The reference hard-codes
        dsize = (752, 480), its dataset's frame, and fails at any other size; this warps at the field's own size.  The `blocks`
        arithmetic of :229-237 is dead code there and is not reproduced."""
        from . import warp as _warp
        homography = self.algorithm == Detector.Algorithm.HOMOGRAPHY
        M = np.asarray(self.homography if homography else self.aff, np.float64)
        M = M if homography else M[:2, :]
        dev = self._device_flow(flow_uv)
        host = None if dev is not None else np.asarray(flow_uv)
        if dev is None and host.dtype != np.float32:
            H, W = host.shape[:2]
            stable = (_warp.warpPerspective if homography else _warp.warpAffine)(host.astype(np.float32), M, (W, H))
            flow = np.where(stable == 0, stable.astype(host.dtype), host)      # elements whose warped value is 0 count as equal
            self.flow_diff = flow - stable
            self.flow_diff_mag = np.sqrt(self.flow_diff[..., 0] ** 2.0 + self.flow_diff[..., 1] ** 2.0)
            self.flow_diff_max = tuple(int(v) for v in np.unravel_index(self.flow_diff_mag.argmax(), self.flow_diff_mag.shape))
        else:
            if dev is not None:
                ctx = dev[0]
                out = ctx.warp_method(flow_uv, M)
            else:
                ctx = im_helpers._ctx(host.shape[1], host.shape[0])
                out = ctx.warp_method(host, M)
            self.flow_diff, self.flow_diff_mag, self.flow_diff_max = out["diff"], out["mag"], out["flow_max"]
        with np.errstate(invalid="ignore", divide="ignore"):
            return im_helpers.get_flow_vis(self.flow_diff), im_helpers.to_rgb(self.flow_diff_mag)

    def is_homography_based(self) -> bool:
        return self.algorithm in [Detector.Algorithm.HOMOGRAPHY]
