"""Processor -- the detection loop of /root/reference/src/processor.py:277-396 on libmavflow: the FoE branch (:304-394) and, with
Processor(algorithm=Detector.Algorithm.HOMOGRAPHY), the global-motion branch (:286-303, see run_detection).

run_detection() keeps the reference's shape: one frame index at a time, the same order of operations
(:305-341), the same FrameResult fields (:353-362); run_detection_staged() is that loop through the reference-named
calls one at a time.  run_detection_batched() is the MI355X form of the same loop:
frame pairs are independent once the flow no longer comes from files, so they go through the fused
mav_process_batch_dev entry point `batch` pairs at a time, two batches in flight.

What the fast loops move (mavflow/pipeline.py): frames (or a host flow field) in; one 32-byte record and eight counts per frame
out.  Flow, derotated flow and both masks stay on the device as DeviceArray handles (Processor.flow_uv, .estimate_fixed,
.total_mask) that turn into host arrays the moment somebody reads them; the calculate_tpr_fpr counts of both masks (:350-351) are
taken on the device against a ground truth that is uploaded once when the dataset declares it constant.

Each loop writes `{results_path}/image_{i:05d}.json` per frame as the reference's write() does (:83-84) when the dataset (or the
constructor) names a results_path.  With an explicit images_path each loop also writes the three result images of :364-374 per frame,
`{images_path}/result-images|derotated|phi/image_{i:05d}.png`, rendered on the device (mav_last_render: one launch behind the
frame's step, the flow is not moved again) and PNG-encoded by a pool of at most 16 threads off the loop's thread; every file is
complete when the loop returns.  Processor(..., png_encoder="device") moves the encoder of the fast loops to where the pixels are
(mav_last_render_png / mav_last_overlay_png: only the compressed streams cross PCIe, the pool adds the chunk framing and writes); the files decode to
the same pixels, their bytes differ.  The staged loop always encodes on the host.  With a processed_path each loop also writes the frame the reference appends to processed.mp4 (:376-392:
FoE discs on the frame, the fixed mask painted purple, blended 0.2 / 0.8) as `{processed_path}/image_{i:05d}.png` for every frame the
reference would write (np.sum(result_img) > 0); the fast loops render it on the device from the resident mask and FoE
(mav_last_overlay), the staged loop composes it from draw_FoE, the painted mask and add_weighted.  No video container is encoded: the
reference's etc/bash/pngs_to_mp4.sh turns the sequence into the mp4.  The global-motion branch writes cluster_vis there instead
(:303) and neither JSON nor result images, as the reference's does outside debug mode; its one-frame loop encodes on the host, its
batched loop (run_detection_batched with algorithm HOMOGRAPHY: _run_global_motion_batched) where png_encoder says."""
from __future__ import annotations

import json
import os
from collections import deque
from concurrent.futures import ThreadPoolExecutor
from typing import Dict, Optional, Tuple

import numpy as np

from . import _lib, frame_source, im_helpers, pipeline, synth, utils
from .detector import Detector
from .focus_of_expansion import FocusOfExpansion
from .frame_result import FrameResult
from .run_config import RunConfig


class SyntheticDataset:
    """A dataset object with the getters run_detection uses (datasets/dataset.py:152-344), fed by mavflow.synth: a textured
    scene under radial (FoE) motion plus one 24x24 patch moving against it.  Flow comes from libmavflow's Farneback
    (use_farneback=True, the seam this build adds) or from the analytic field (the reference's .flo seam)."""

    def __init__(self, W: int = 640, H: int = 480, N: int = 6, use_farneback: bool = True, dt: float = 1 / 30.0,
                 dangle=(0.0, 0.0, 0.0), seed: int = 0, distinct: Optional[int] = None, results_path: Optional[str] = None,
                 video: bool = False, lanes: Optional[int] = None):
        self.capture_size = (W, H)
        self.resolution = np.array([W, H])
        self.constant_segmentation = True                # one segmentation image for all frames (Processor derives it once)
        self.constant_sky_segmentation = True            # ... and one sky mask
        self.N = N
        self.distinct = distinct                         # pair i shows the content of pair i % distinct (long runs from few pictures)
        # video = True: ONE sequence of frames (synth.make_sequence: a texture under a growing zoom), pair i = (frame i, frame i + 1) as
        # the SAME array objects -- how a video runs through the reference's loop; the batched loop then uploads and expands every frame once
        self.video = video
        self._frames = None
        self.lanes = lanes                               # contexts the Farneback seam takes in turn (None: pipeline.auto_lanes for one pair)
        self.results_path = results_path                 # where Processor writes image_%05d.json (dataset.py: results_path)
        self.sequence = f"synthetic-{seed}"
        self.use_farneback = use_farneback
        self.dt = dt
        self.dangle = np.asarray(dangle, np.float64)
        self.seed = seed
        self._pairs = {}
        self._gt32 = {}
        self._bgr = {}
        self._seg = self._sky = self._depth = None       # the constant images are built once, like files read once
        self._ctxs = []
        self._stage: Optional[pipeline.LanedFlowStage] = None
        self._frame_cursor = 0

    VIDEO_K = 0.004                                      # zoom per frame of the video form (synth.make_sequence)

    def _pair(self, i: int):
        if self.distinct:
            i %= self.distinct
        if i not in self._pairs:
            W, H = self.capture_size
            if self.video:
                if self._frames is None:
                    n = (self.distinct or (self.N - 1)) + 1
                    self._frames = list(synth.make_sequence(W, H, n, seed=self.seed, k=self.VIDEO_K))
                # frame j is the texture zoomed by j k about c = (0.55 W, 0.45 H): a point seen at x in frame i sits at
                # x + k (x - c) / (1 - (i + 1) k) in frame i + 1
                g = self.VIDEO_K / (1.0 - (i + 1) * self.VIDEO_K)
                truth = np.empty((H, W, 2))
                truth[..., 0] = (g * (np.arange(W) - 0.55 * W))[None, :]
                truth[..., 1] = (g * (np.arange(H) - 0.45 * H))[:, None]
                self._pairs[i] = (self._frames[i], self._frames[i + 1], truth)
            else:
                self._pairs[i] = synth.make_pair(W, H, self.seed * 1000 + i)
        return self._pairs[i]

    def frame_pair(self, i: int) -> Tuple[np.ndarray, np.ndarray]:
        f0, f1, _ = self._pair(i)
        return f0, f1

    def get_frame(self) -> np.ndarray:
        i = self._frame_cursor % self.N
        self._frame_cursor += 1
        if i not in self._bgr:
            self._bgr[i] = np.repeat(self._pair(i)[1][..., None], 3, axis=2)
        return self._bgr[i]

    def get_flow_uv(self, i: int):
        """float32 (H, W, 2): the analytic field (a host array, what a .flo file would hold) or libmavflow's Farneback -- then as a
        pipeline.DeviceArray: array-like, on the device until read, so the loop's next stage takes it from where it is."""
        f0, f1, truth = self._pair(i)
        if not self.use_farneback:
            return self.get_gt_of(i)
        if self._stage is None:
            W, H = self.capture_size
            n = self.lanes or pipeline.auto_lanes(W, H, 1)
            self._ctxs = [_lib.Context(W, H, 1) for _ in range(n)]
            self._stage = pipeline.LanedFlowStage(self._ctxs)
        return self._stage.flow_of(f0, f1)

    def get_gt_of(self, i: int) -> np.ndarray:
        if self.distinct:
            i %= self.distinct
        if i not in self._gt32:
            self._gt32[i] = self._pair(i)[2].astype(np.float32)
        return self._gt32[i]

    def get_segmentation(self, i: int) -> np.ndarray:
        if self._seg is None:
            W, H = self.capture_size
            self._seg = np.zeros((H, W, 3), np.uint8)
            self._seg[H // 4:H // 4 + 24, W // 4:W // 4 + 24] = 255
        return self._seg

    def get_sky_segmentation(self, i: int) -> np.ndarray:
        if self._sky is None:
            self._sky = np.zeros((self.capture_size[1], self.capture_size[0]), dtype=bool)
        return self._sky

    def get_depth(self, i: int) -> np.ndarray:
        if self._depth is None:
            self._depth = np.ones((self.capture_size[1], self.capture_size[0]), np.float32)
        return self._depth

    def validate_sky_segment(self, sky_mask, depth_buffer) -> Tuple[float, float]:
        return (0.0, 0.0)

    def get_gt_foe(self, i: int) -> Tuple[float, float]:
        return (0.55 * self.capture_size[0], 0.45 * self.capture_size[1])

    def get_time(self, i: int) -> float:
        return i * self.dt

    def get_delta_time(self, i: int) -> float:
        return self.dt

    def get_angular_difference(self, a: int, b: int) -> np.ndarray:
        return self.dangle

    @property
    def ground_truth(self):
        """The moving patch's rectangle (dataset.py: ground_truth, what get_annotation fills in): one box for every frame."""
        W, H = self.capture_size
        return [utils.Rectangle((W // 4, H // 4), (24, 24))]

    def get_annotation(self, i: int) -> None:
        """Nothing to read: ground_truth is constant."""

    def release(self) -> None:
        if self._stage is not None:
            self._stage.close()
            for c in self._ctxs:
                c.close()
            self._ctxs, self._stage = [], None


# the result images of processor.py:364-374: Context.render's names -> the reference's directories
IMAGE_DIRS = {"result": "result-images", "flow": "derotated", "phi": "phi"}
PNG_WORKERS = 16                     # encoder threads at most
PNG_BACKLOG = 4 * PNG_WORKERS        # files queued before the loop waits for the oldest


def _write_stream(path: str, stream) -> None:
    """The PNG file around a zlib stream the device produced (stream: frame_source.png_wrap's argument tuple)."""
    with open(path, "wb") as f:
        f.write(frame_source.png_wrap(*stream))


class Processor:
    def __init__(self, config: RunConfig, results_path: Optional[str] = None, images_path: Optional[str] = None,
                 processed_path: Optional[str] = None, png_encoder: str = "host", algorithm: Optional["Detector.Algorithm"] = None,
                 blobs: Optional[dict] = None, roc: Optional[dict] = None, debug_path: Optional[str] = None, validation: str = "host") -> None:
        if validation not in ("host", "device"):
            raise ValueError(f"validation must be 'host' or 'device', got {validation!r}")
        if png_encoder not in ("host", "device"):
            raise ValueError(f"png_encoder must be 'host' or 'device', got {png_encoder!r}")
        # extra: validation="device" takes the validation tail of the FoE loops (processor.py:315-317, 343-347, 360) -- drone_size_pixels,
        # the box centre behind center_phi, sky_tpr / sky_fpr and drone_flow_pixels -- from ONE Context.gt_stats call per batch on the
        # loop's own context (include/mavflow_validation.h) instead of full-frame numpy on the host: no np.nonzero, no
        # get_simple_bounding_box upload, no dataset.validate_sky_segment.  The sky scores then follow the reference's
        # Dataset.validate_sky_segment rule (depth > 0.80 * max(depth), calculate_tpr_fpr) WHATEVER the dataset overrides, and the depth
        # buffer has to be float32 (as the reference's .pfm reader returns it).  A ground-truth flow the dataset hands out as a device
        # handle of the loop's context is summed where it is; a host array is not uploaded: it is gathered at the listed pixels and
        # averaged as today.  A frame whose drone has more than validation_max_pixels pixels takes today's host path for its pixel list.
        # FrameResult, its JSON and every file are the same either way; the global-motion branch has no validation tail and ignores it.
        self.validation = validation
        # extra: debug_path=DIR makes run_detection() in the global-motion branch write the reference's debug frame (processor.py:295-301),
        # image_{i:05d}.png at 3W x 2H: Detector.draw on the frame, then the six tiles, composed on the device from the pictures where
        # they are and brought back in one download; detection_results[i] = detector.frame_result.  config.debug alone keeps raising.
        self.debug_path = debug_path
        self.validation_max_pixels = _lib._validation.DEFAULT_MAX_PIXELS
        self._tails: Dict[int, dict] = dict()
        # extra: blobs=dict(connectivity=, min_area=, max_blobs=) (any subset; {} = the defaults 8, 1, 256) labels every frame's fixed mask
        # on the device, inside the frame's own step, and fills detection_blobs[i] = [(Rectangle, area, (cx, cy)), ...] in label order --
        # one entry per connected component where detection_boxes[i] is the hull of them all.  None (default): not one launch more.
        # FrameResult, its JSON and every file the loops write are the same either way.
        self.blobs = None if blobs is None else _lib.cc_defaults(**blobs)
        self.detection_blobs: Dict[int, list] = dict()
        # extra: roc=dict(angles=[...], mags=[...]) sweeps the fixed mask's two thresholds (processor.py:340-341: 15 degrees, 1.0 px) over
        # both lists in the frame's own step and fills roc_counts[i], a (Ka, Km, 4) int64 array of calculate_tpr_fpr's sums (pos, neg, tp,
        # fp) per threshold pair; roc_rates() divides them.  None (default): not one launch more; results and files are the same either way.
        self.roc = None
        if roc is not None:
            if set(roc) != {"angles", "mags"}:
                raise ValueError("roc: dict(angles=[...], mags=[...]) expected")
            _, a, m = _lib.roc_params(roc["angles"], roc["mags"])
            self.roc = dict(angles=a, mags=m)
        self.roc_counts: Dict[int, np.ndarray] = dict()
        self.png_encoder = png_encoder
        self.config = config
        self.logger = config.logger
        self.sequence = config.sequence
        self.debug_mode = config.debug
        self.headless = config.headless
        self.dataset = config.get_dataset()
        self.detector = Detector(self.dataset, algorithm)           # None: the reference's default, which takes the FoE branch
        self.detection_results: Dict[int, FrameResult] = dict()
        # extras of the global-motion branch: every frame's (optimised) window and its IoU with the last ground-truth box
        self.detection_windows: Dict[int, utils.Rectangle] = dict()
        self.detection_iou: Dict[int, float] = dict()
        self._gm_bufs = None                             # (context, device buffers) of the global-motion step
        self._gm_slots = None                            # (key, the two buffer sets) of the batched global-motion loop
        # extra: get_simple_bounding_box of every frame's fixed mask, which the device records with the FoE (the reference derives no
        # box in this loop; FrameResult and its JSON stay exactly the reference's)
        self.detection_boxes: Dict[int, utils.Rectangle] = dict()
        self.frame_step_size = 1
        self.frame_index, self.start_frame = 0, 100
        self.is_exiting = False
        self.focus_of_expansion = FocusOfExpansion(self.detector.lucas_kanade)
        self.flow_uv = None
        self._derot, self._derot_frame = None, 0
        # {results_path}/image_{i:05d}.json per frame (processor.py:83-84); the reference takes the directory from its dataset
        self.results_path = results_path if results_path is not None else getattr(self.dataset, "results_path", None)
        self._ctxs = []                                 # this loop's own contexts (never the helpers' shared, evictable ones)
        self._pipes = {}
        self._stale_pipes = []                           # pipelines over a subset of the lanes now in use, until their last frames are collected
        self._seg_val = None
        self._center = None
        # the result images (processor.py:364-374): only an explicit images_path turns them on
        self.images_path = images_path
        # the processed.mp4 frames (processor.py:376-392) as a PNG sequence: only an explicit processed_path turns them on
        self.processed_path = processed_path
        self._png_pool = None
        self._png_jobs = deque()
        self._dirs_made = set()

    def is_active(self) -> bool:
        return self.frame_index < self.dataset.N - 1 and not self.is_exiting

    def analyze_radial_error(self) -> None:
        """Compare the angular error in flow to the magnitude of the flow (processor.py:267-275): the current frame's flow_uv against
        gt_flow_uv over the non-sky pixels.  Where the reference saves two full-frame arrays per frame and bins them afterwards
        (plot_radial_error.py:38-39), the histogram over those bins builds up on the device: self.radial_error is the accumulator
        (Context.radial_error_accumulator; .counts() -> counts, non_sky, in_range).  Nothing calls it inside the loops, as in the reference."""
        if self.flow_uv is None:
            raise ValueError("analyze_radial_error: no flow_uv of a current frame")
        i = self.frame_index
        gt = self.gt_flow_uv if self.gt_flow_uv is not None else utils.assert_type(self.dataset.get_gt_of(i))     # (processor.py:309)
        sky = getattr(self, "sky_mask", None)
        sky = sky if sky is not None else self.dataset.get_sky_segmentation(i)
        on_dev = isinstance(self.flow_uv, pipeline.DeviceArray) and self.flow_uv.on_device
        ctx = self.flow_uv.ctx if on_dev else self._own_ctxs(1, 1)[0]
        if self.radial_error is None or self.radial_error.ctx is not ctx or not ctx.alive:
            if self.radial_error is not None:
                self.radial_error.close()
            self.radial_error = ctx.radial_error_accumulator()
        self.radial_error.add(self.flow_uv, gt, sky)

    radial_error = None
    gt_flow_uv = None

    # -- device plumbing --------------------------------------------------------------------------------------------------------
    def _pipeline(self, ctxs, batch: int) -> "pipeline.LanedPipeline":
        """The (cached) pipeline over these contexts for `batch` pairs per submit."""
        key = (tuple(id(c) for c in ctxs), batch)
        pipe = self._pipes.get(key)
        if pipe is None or any(a is not b or not b.alive for a, b in zip(pipe.ctxs, ctxs)):
            if pipe is not None:
                pipe.close()
            # a seam that shows its lanes one by one (_flow_ctxs' fallback) makes this grow [c0] -> [c0, c1] -> ...: the pipelines over
            # the smaller sets would keep their three slots of device and page-locked buffers on the same contexts until release()
            # (closed by _drop_stale_pipes once the loop has collected what it still has in flight on them)
            mine = set(key[0])
            for k in [k for k in self._pipes if k[1] == batch and k != key and set(k[0]) < mine]:
                self._stale_pipes.append(self._pipes.pop(k))
            pipe = pipeline.LanedPipeline(ctxs, batch)
            pipe.set_params(foe_params=self.focus_of_expansion._foe_params(1000), **({} if self.blobs is None else {"cc_params": self.blobs}),
                            **({} if self.roc is None else {"roc": self.roc}))
            self._pipes[key] = pipe
        return pipe

    def _own_ctxs(self, batch: int = 1, lanes: int = 1):
        """This loop's own contexts (never the helpers' shared, evictable ones): `lanes` of them, each for `batch` pairs."""
        W, H = self.dataset.capture_size
        ok = len(self._ctxs) >= lanes and all(c.alive and c.max_batch >= batch and (c.W, c.H) == (W, H) for c in self._ctxs[:lanes])
        if not ok:
            self._close_pipes()
            self._free_global_motion_slots()
            for c in self._ctxs:
                c.close()
            self._ctxs = [_lib.Context(W, H, batch) for _ in range(lanes)]
        return self._ctxs[:lanes]

    def _flow_ctxs(self, flow) -> list:
        """The contexts a device-resident flow seam works on: every lane of the stage that produced this handle when the dataset shows
        it (SyntheticDataset, FarnebackFlowProvider: attribute _stage), else the handle's own context."""
        for holder in (self.dataset, getattr(self.dataset, "_flow", None)):
            st = getattr(holder, "_stage", None)
            if isinstance(st, pipeline.LanedFlowStage) and any(s.ctx is flow.ctx for s in st.stages):
                return [s.ctx for s in st.stages]
        # a seam that does not show its stage: the contexts its handles have come from so far (a seam that takes two or three contexts
        # in turn is recognised within its first frames; the pipeline is then rebuilt once over all of them)
        self._lane_seen = [c for c in getattr(self, "_lane_seen", []) if c.alive]
        if not any(c is flow.ctx for c in self._lane_seen):
            self._lane_seen.append(flow.ctx)
        return list(self._lane_seen)

    def _drop_stale_pipes(self) -> None:
        for pipe in self._stale_pipes:
            pipe.close()
        self._stale_pipes = []

    def _close_pipes(self) -> None:
        self._drop_stale_pipes()
        for pipe in self._pipes.values():
            pipe.close()
        self._pipes = {}

    # -- validation tail shared by the loops (processor.py:343-362) ---------------------------------------------------
    def _fill_result(self, i: int, foe_dense, sky_scores, counts_fixed=None, counts_dyn=None, estimate_fixed=None, total_mask=None) -> FrameResult:
        """The FrameResult of frame i.  The TPR / FPR pairs come from the counts the device took of both masks (the fast loops), or,
        when masks are given instead, from calculate_tpr_fpr on them as the reference's lines read (the staged loop)."""
        r = FrameResult()
        r.foe_dense = foe_dense
        r.foe_gt = utils.assert_type(self.dataset.get_gt_foe(i))
        tail = self._tails.pop(i, None)                        # validation="device": what the batch's gt_stats call found for this frame
        if tail is not None:
            segmentation, center, drone_flow_avg_gt, size = tail["seg"], tail["center"], tail["flow_avg"], tail["size"]
        else:
            segmentation, rows, cols = self._segmentation(i)
            # ground-truth flow of the drone: derotated at the drone's pixels only (pointwise, same values as derotating the frame)
            gt = utils.assert_type(self.dataset.get_gt_of(i))
            with np.errstate(all="ignore"):
                drone_flow_avg_gt = np.average(self.detector.derotate_at(i - self.frame_step_size, i, gt[rows, cols], rows, cols), axis=0)
            center = self._gt_center(segmentation)
            size = np.int64(rows.size)                         # == np.sum(segmentation > 127), a numpy integer as in the reference
        r.center_phi = np.rad2deg(np.arctan2(center[1] - r.foe_gt[1], center[0] - r.foe_gt[0]))
        if counts_fixed is not None:
            r.tpr_fixed, r.fpr_fixed = im_helpers._rates(counts_fixed)
            r.tpr, r.fpr = im_helpers._rates(counts_dyn)
        else:
            r.tpr_fixed, r.fpr_fixed = im_helpers.calculate_tpr_fpr(segmentation, 255 * estimate_fixed)     # as processor.py:350-351
            r.tpr, r.fpr = im_helpers.calculate_tpr_fpr(segmentation, 255 * total_mask)
        r.sky_tpr, r.sky_fpr = sky_scores
        r.drone_flow_pixels = (drone_flow_avg_gt[0], drone_flow_avg_gt[1])
        r.drone_size_pixels = size
        r.time = self.dataset.get_time(i)
        return r

    def _store(self, i: int, r: FrameResult) -> None:
        self.detection_results[i] = r
        self.config.results[i] = r
        if self.results_path is not None:                      # what write() leaves per frame (processor.py:83-84), same text
            os.makedirs(self.results_path, exist_ok=True)
            with open(f"{self.results_path}/image_{i:05d}.json", "w") as f:
                f.write(json.dumps(utils.get_json(r), indent=4, sort_keys=True))

    # -- result images (processor.py:364-374) ----------------------------------------------------------------------------------------
    def _queue_png(self, d: str, i: int, img) -> None:
        """Queue the PNG file {d}/image_{i:05d}.png on the encoder pool (at most PNG_BACKLOG files queued).  img: an image to encode, or
        the stream of one encoded on the device (png_wrap's argument tuple), which only remains to be framed and written."""
        if d not in self._dirs_made:
            os.makedirs(d, exist_ok=True)
            self._dirs_made.add(d)
        if self._png_pool is None:
            self._png_pool = ThreadPoolExecutor(max_workers=min(PNG_WORKERS, os.cpu_count() or 1), thread_name_prefix="png")
        while len(self._png_jobs) >= PNG_BACKLOG:
            self._png_jobs.popleft().result()
        job = _write_stream if isinstance(img, tuple) else frame_source.imwrite
        self._png_jobs.append(self._png_pool.submit(job, os.path.join(d, f"image_{i:05d}.png"), img))

    def _write_images(self, ids, imgs) -> None:
        """Queue the PNG files of frames `ids`; imgs: Context.render's dict of (n, H, W, 3) BGR arrays, or render_last_png's of files."""
        for k, i in enumerate(ids):
            for name, d in IMAGE_DIRS.items():
                self._queue_png(os.path.join(self.images_path, d), i, imgs[name][k])

    def _write_processed(self, ids, frames, written) -> None:
        """Queue the processed.mp4 frames of frames `ids` (processor.py:385-394): a frame the reference does not write (nothing in the
        fixed mask and no disc pixel in the image) gets its message instead of a file."""
        for k, i in enumerate(ids):
            if written[k]:
                self._queue_png(self.processed_path, i, frames[k])
            else:
                self.logger.warning("An error occured while processing frames.")

    def _flush_images(self) -> None:
        """Every queued file written (raises what an encoder raised)."""
        while self._png_jobs:
            self._png_jobs.popleft().result()

    def _segmentation(self, i: int):
        """Channel 0 of the dataset's segmentation image, contiguous, with the coordinates of its drone pixels (> 127) and the
        centre of its bounding box (processor.py:332,344-347).  Derived per frame, as the reference's loop does, unless the dataset
        DECLARES its segmentation constant (attribute `constant_segmentation`, SyntheticDataset): then once.  (Caching on the
        array's identity alone would hand a dataset that refills one preallocated array the first frame's pixels for ever.)"""
        seg3 = self.dataset.get_segmentation(i)
        if getattr(self.dataset, "constant_segmentation", False) and self._seg_val is not None:
            return self._seg_val
        seg = np.ascontiguousarray(seg3[..., 0])
        rows, cols = np.nonzero(seg > 127)
        self._seg_val = (seg, rows, cols)
        self._center = None
        return self._seg_val

    def _gt_center(self, segmentation: np.ndarray):
        """get_simple_bounding_box(segmentation).get_center() (processor.py:346-347) of the image _segmentation() last derived."""
        if self._center is None:
            self._center = im_helpers.get_simple_bounding_box(segmentation).get_center()
        return self._center

    # The reference's loop also leaves flow_uv_derotated and flow_mag behind (processor.py:306-307).  The fused call never forms
    # them on the host; they are derived on first access from the frame's flow, through the same shims the staged loop uses.
    @property
    def flow_uv_derotated(self):
        if self._derot is None and self.flow_uv is not None:
            self._derot = self.detector.derotate(self._derot_frame - self.frame_step_size, self._derot_frame, np.asarray(self.flow_uv))
        return self._derot

    @flow_uv_derotated.setter
    def flow_uv_derotated(self, v):
        self._derot = v

    @property
    def flow_mag(self):
        d = self.flow_uv_derotated
        return None if d is None else im_helpers.get_magnitude(d)

    def _rates(self, i: int):
        dt = self.dataset.get_delta_time(i)
        return np.asarray(self.dataset.get_angular_difference(i - self.frame_step_size, i), np.float64) / dt, dt

    def _sky_and_gt(self, ids, segs=None):
        """(submit() keywords for the sky masks and the ground truth of these frames, their sky masks).  A dataset that declares
        an image constant has it uploaded once for the run; otherwise one image per frame travels with the batch.  segs: the frames'
        segmentation images (channel 0) where the caller has them already (validation="device": no drone pixels are derived here)."""
        kw = {}
        skies = [self.dataset.get_sky_segmentation(i) for i in ids]
        if getattr(self.dataset, "constant_sky_segmentation", False):
            kw["sky_shared"] = skies[0]
        else:
            kw["sky"] = skies
        if segs is None:
            segs = [self._segmentation(i)[0] for i in ids]
        if getattr(self.dataset, "constant_segmentation", False):
            kw["gt_shared"] = segs[0]
        else:
            kw["gt"] = list(segs)
        return kw, skies

    def _seg_plane(self, i: int) -> np.ndarray:
        """Channel 0 of the dataset's segmentation image, contiguous (once for a dataset that declares it constant): no pixel list."""
        seg3 = self.dataset.get_segmentation(i)
        if getattr(self.dataset, "constant_segmentation", False):
            if self._seg_plane_val is None:
                self._seg_plane_val = np.ascontiguousarray(seg3[..., 0])
            return self._seg_plane_val
        return np.ascontiguousarray(seg3[..., 0])

    _seg_plane_val = None

    def _validation_tail(self, ctxs, ids):
        """validation="device": ONE Context.gt_stats call for frames `ids` on one of the loop's contexts `ctxs`, at the point where the
        host path runs _sky_and_gt and dataset.validate_sky_segment.  Returns what those give -- (submit() keywords, sky masks, sky
        scores per frame) -- and leaves every frame's tail (segmentation, drone size, box centre, average ground-truth flow of the
        drone) in self._tails for _fill_result.
        The ground-truth flow: device handles of one of these contexts that follow each other in memory (one frame always does) are
        summed on the device (the record's flow_sum); anything else is read as host arrays, gathered at the listed pixels and averaged
        as the host path does (Detector.derotate_at, np.average).  A frame with more drone pixels than validation_max_pixels takes
        the host path's np.nonzero for its list."""
        W, H = self.dataset.capture_size
        n = len(ids)
        segs = [self._seg_plane(i) for i in ids]
        kw, skies = self._sky_and_gt(ids, segs)
        depths = [utils.assert_type(self.dataset.get_depth(i)) for i in ids]
        gts = [utils.assert_type(self.dataset.get_gt_of(i)) for i in ids]
        ctx = ctxs[0]
        on_dev = all(isinstance(g, pipeline.DeviceArray) and g.on_device and np.dtype(g.dtype) == np.float32 and tuple(g.shape) == (H, W, 2) for g in gts)
        if on_dev:
            ctx = next((c for c in ctxs if c is gts[0].ctx), None)
            on_dev = ctx is not None and all(g.ctx is ctx for g in gts) and all(gts[k + 1].ptr == gts[k].ptr + gts[k].nbytes for k in range(n - 1))
            ctx = ctx if on_dev else ctxs[0]
        gt_arg = pipeline.DeviceArray(ctx, gts[0].ptr, (n, H, W, 2), np.float32) if on_dev else None
        rates = [self._rates(i) if i >= 1 else (np.zeros(3), 1.0) for i in ids]
        out = ctx.gt_stats(np.stack(segs), gt_flow=gt_arg, sky=np.stack([np.asarray(sk) for sk in skies]), depth=np.stack(depths),
                           omega=np.stack([r[0] for r in rates]), dt=[r[1] for r in rates], frame0=[i < 1 for i in ids],
                           max_pixels=self.validation_max_pixels, indices=True)
        for k, i in enumerate(ids):
            avg = out["drone_flow_avg"][k] if on_dev else None
            if avg is None:
                if out["truncated"][k]:
                    rows, cols = np.nonzero(segs[k] > 127)
                else:
                    rows, cols = np.divmod(out["indices"][k].astype(np.intp), W)
                gt = np.asarray(gts[k])
                with np.errstate(all="ignore"):
                    avg = np.average(self.detector.derotate_at(i - self.frame_step_size, i, gt[rows, cols], rows, cols), axis=0)
            self._tails[i] = dict(seg=segs[k], size=out["drone_size_pixels"][k], center=out["box"][k].get_center(), flow_avg=avg)
        return kw, skies, out["sky_tpr_fpr"]

    def run_detection(self) -> Dict[int, FrameResult]:
        """The reference's loop (processor.py:283-341): one frame index at a time, flow from the dataset's seam (get_flow_uv: a
        .flo file -> a host array, or Farneback on the GPU -> a DeviceArray), then derotation -> FoE -> phi -> masks -> box -> the
        calculate_tpr_fpr counts of both masks in ONE enqueue on the context that holds the flow (pipeline.DetectPipeline): a host
        field crosses PCIe once, a device field not at all; a 32-byte record and eight counts come back.  estimate_fixed /
        total_mask are DeviceArray handles (read them and they are host arrays).  Frame 0 takes the reference's float32 path
        (detector.py:80-81).  The sample coordinates are drawn from np.random exactly where get_FOE_dense draws them.
        Software-pipelined: frame i's FrameResult is filled in (and its JSON written) after the following frames -- as many as the
        pipeline has lanes (pipeline.auto_lanes: 3 - 4 contexts taken in turn for frames up to 1080p, whose one-pair chains of launches
        then interleave on the GPU) -- have been enqueued; results, files and their order are those of the plain loop.
        With Processor(validation="device") the frame's drone size, box centre, sky scores and average ground-truth flow come from one
        Context.gt_stats call (_validation_tail); the sky scores then follow the reference's Dataset.validate_sky_segment rule whatever
        the dataset overrides.  The same holds for run_detection_batched() (one call per batch) and run_detection_staged()."""
        from collections import deque
        if self.detector.is_homography_based():
            return self._run_global_motion()
        pending = deque()

        def finish(n_keep: int) -> None:
            while len(pending) > n_keep:
                self._finish_frame(*pending.popleft())

        pipe = None
        while self.is_active():
            i = self.frame_index
            orig_frame = self.dataset.get_frame()
            self.flow_uv = self.dataset.get_flow_uv(i)
            if self.flow_uv is None:
                raise ValueError("Could not load flow field.")
            self._derot, self._derot_frame = None, i
            if self.flow_uv.dtype != np.float32:
                # a float64 field is evaluated in float64 from the start by the reference: the fused float32 call would narrow
                # it, so this frame goes through the float64 kernels (the staged calls)
                finish(0)
                self._staged_frame(i, orig_frame)
                continue
            on_dev = isinstance(self.flow_uv, pipeline.DeviceArray) and self.flow_uv.on_device
            # (a host flow field -- the .flo seam -- is a 3-launch chain behind a 16.6 MB upload at 1080p: PCIe-bound, one lane; measured
            # 0.43 ms per frame with one context, 0.47 - 0.53 with two)
            ctxs = self._flow_ctxs(self.flow_uv) if on_dev else self._own_ctxs(1, 1)
            now = self._pipeline(ctxs, 1)
            if now is not pipe:                                         # the flow moved to other contexts: drain the old pipeline first
                finish(0)
                self._drop_stale_pipes()
                pipe = now
            if self.validation == "device":
                kw, skies, scores = self._validation_tail(ctxs, [i])
                self.sky_mask, sky = skies[0], scores[0]
            else:
                kw, skies = self._sky_and_gt([i])
                self.sky_mask = skies[0]
                sky = self.dataset.validate_sky_segment(self.sky_mask, utils.assert_type(self.dataset.get_depth(i)))
            rand1 = np.empty((2000, 2), dtype=np.uint32)                 # focus_of_expansion.py:69-71
            rand1[..., 0] = np.random.randint(0, self.flow_uv.shape[0], 2000)
            rand1[..., 1] = np.random.randint(0, self.flow_uv.shape[1], 2000)
            omega, dt = self._rates(i) if i >= 1 else (np.zeros(3), 1.0)
            ticket = pipe.submit(rand1, flow=self.flow_uv, omega=omega, dt=dt, frame0=[i < 1], **kw)
            pending.append((pipe, i, ticket, sky, orig_frame))
            # with images the frame is finished at once: its images are rendered from what its step left on the lane's context
            finish(0 if self._renders else pipe.depth)
            self.frame_index += 1
        finish(0)
        self._flush_images()
        return self.detection_results

    # -- the global-motion branch (processor.py:286-303) ----------------------------------------------------------------------------
    def _run_global_motion(self) -> Dict[int, FrameResult]:
        """processor.py:286-303 outside debug mode, one frame at a time: the flow from the dataset's seam, then
        get_transformation_matrix -> flow_vec_subtract as ONE enqueue (mav_global_motion_step_dev: pair gather, homography fit,
        subtraction, normalised image, window search, optimize_window with detector.use_optimization) on the context that holds the
        flow -- a device handle is not moved, a host field crosses PCIe once, the matrix never visits the host before the record does.
        Back come the 88-byte record, the matrix and, with a processed_path, the u8 image: cluster_vis is written there as
        image_{i:05d}.png, the reference's write(cluster_vis).  Sets detector.homography / confidence / flow_max / iou (and
        cluster_vis when it is fetched) per frame, detection_windows[i] and detection_iou[i]; the returned dict is empty, as the reference's is outside debug
        mode.  A field that is not float32 goes through the Detector's two calls (host float64 arithmetic).  flow_vis (:288) is formed
        in debug mode only, which this branch does not reproduce."""
        self._no_blobs_here()
        self._no_roc_here()
        if self.debug_mode and self.debug_path is None:
            raise NotImplementedError("debug_mode in the global-motion branch draws with cv2.rectangle and writes a six-image mosaic "
                                      "(processor.py:295-301): not reproduced")
        det = self.detector
        W, H = self.dataset.capture_size
        while self.is_active():
            i = self.frame_index
            orig_frame = self.dataset.get_frame()
            self.flow_uv = self.dataset.get_flow_uv(i)
            if self.flow_uv is None:
                raise ValueError("Could not load flow field.")
            self.dataset.get_annotation(i)
            dev = det._device_flow(self.flow_uv)
            if dev is None and np.asarray(self.flow_uv).dtype != np.float32:
                if self.debug_path is not None:
                    raise NotImplementedError("debug_path composes the debug frame from the device's float32 pictures; this flow field is "
                                              f"{np.asarray(self.flow_uv).dtype}")
                det.get_transformation_matrix(orig_frame, self.flow_uv)
                _, cluster_vis, _, _ = det.flow_vec_subtract(orig_frame, self.flow_uv)
                window = det.opt_window[1]
            else:
                ctx, ptr = dev if dev is not None else (self._own_ctxs(1, 1)[0], None)
                b = self._global_motion_buffers(ctx)
                if ptr is None:
                    ptr = b["flow"].upload(np.ascontiguousarray(self.flow_uv, dtype=np.float32)).ptr
                if det.use_sparse_of:                    # the pairs come from the tracker (host), the rest stays one call
                    det.get_transformation_matrix(orig_frame, self.flow_uv)
                    b["M"].upload(np.ascontiguousarray(det.homography[:2, :]))
                    _lib.check(ctx.lib.mav_global_motion_dev(ctx.h, ptr, b["M"].ptr, 1, 1.5, int(bool(det.use_optimization)), None, None,
                                                             b["gray"].ptr, b["res"].ptr))
                else:
                    ctx.global_motion_step(ptr, det.coords, 1, b["res"].ptr, optimize=det.use_optimization, H_ptr=b["H"].ptr,
                                           ok_ptr=b["ok"].ptr, gray_ptr=b["gray"].ptr)
                    if not int(b["ok"].download(np.int32, (1,))[0]):
                        raise RuntimeError(self.GM_MESSAGE.format(i))
                    det.homography = b["H"].download(np.float64, (3, 3))
                    det.confidence = np.ones((det.coords.shape[0], 1), np.uint8)
                rec = b["res"].download(_lib.MOTION_DTYPE, (1,))[0]
                det.flow_max = (int(rec["max_row"]), int(rec["max_col"]))
                x, y, w, h = (int(v) for v in rec["opt_window"])
                window = utils.Rectangle.from_points((x, y), (x + w, y + h))
                cluster_vis = None
                if self.processed_path is not None:
                    cluster_vis = np.repeat(b["gray"].download(np.uint8, (H, W))[..., None], 3, axis=2)
                    det.cluster_vis = cluster_vis
                for gt in self.dataset.ground_truth:
                    det.iou = utils.Rectangle.calculate_iou(window, gt)
                det.prev_frame = orig_frame
                if self.debug_path is not None:
                    self._queue_png(self.debug_path, i, self._debug_frame(ctx, ptr, b["gray"].ptr, orig_frame))
                    det.frame_result = FrameResult()                   # flow_vec_subtract's fresh record (detector.py:154)
                    self.detection_results[i] = det.frame_result
            self.detection_windows[i] = window
            if hasattr(det, "iou"):
                self.detection_iou[i] = det.iou
            if self.processed_path is not None:
                self._queue_png(self.processed_path, i, cluster_vis)
            self.frame_index += 1
        self._flush_images()
        return self.detection_results

    def _debug_frame(self, ctx, flow_ptr, gray_ptr, orig_frame: np.ndarray) -> np.ndarray:
        """processor.py:295-299 on the device, behind the frame's global-motion step on `ctx`: detector.draw on the uploaded frame
        (the ground-truth rectangles, one table), get_flow_vis of the flow, of flow_uv_warped and of global_motion rendered where the
        flow and the matrix are, and np.vstack((np.hstack((orig_frame, global_motion_vis, flow_uv_warped_vis)), np.hstack((flow_vis,
        global_motion_vis, cluster_vis)))) as one mosaic launch -- cluster_vis is the step's gray plane, replicated.  One download, the
        (2H, 3W, 3) frame; orig_frame receives its drawn tile, as the reference draws into it."""
        from . import shapes
        W, H = ctx.W, ctx.H
        n = W * H
        frame = np.asarray(orig_frame)
        if frame.shape != (H, W, 3) or frame.dtype != np.uint8:
            raise ValueError(f"debug_path: the frame is {frame.dtype} {frame.shape}; the debug frame takes uint8 ({H}, {W}, 3)")
        frame = np.ascontiguousarray(frame)
        table = shapes.table(self.detector.ground_truth_shapes())
        if len(table) > self.DEBUG_MAX_BOXES:
            raise ValueError(f"debug_path: {len(table)} ground-truth boxes; the debug frame's table holds {self.DEBUG_MAX_BOXES}")
        blk = self._global_motion_buffers(ctx)["debug"]               # four pictures, the table, the scratch field, the mosaic
        o_tab = 3 * n * 4
        o_field = o_tab + 32 * self.DEBUG_MAX_BOXES
        o_out = o_field + 8 * n
        pic = [blk.ptr + 3 * n * k for k in range(4)]
        _lib.check(ctx.lib.mav_memcpy_h2d(ctx.h, pic[0], _lib._ptr(frame), frame.nbytes))
        if len(table):
            _lib.check(ctx.lib.mav_memcpy_h2d(ctx.h, blk.ptr + o_tab, _lib._ptr(table), table.nbytes))
            ctx.draw_shapes_enqueue(pic[0], blk.ptr + o_tab, len(table), 3, 1)              # one colour: the direct form
        ctx.motion_pictures_enqueue(1, flow_ptr, blk.ptr + o_field, pic[1], pic[2], pic[3])
        ctx.mosaic_enqueue([pic[0], pic[3], pic[2], pic[1], pic[3], gray_ptr], [3, 3, 3, 3, 3, 1], 2, 3, blk.ptr + o_out, 1)
        out = np.empty((2 * H, 3 * W, 3), np.uint8)
        _lib.check(ctx.lib.mav_memcpy_d2h(ctx.h, _lib._ptr(out), blk.ptr + o_out, out.nbytes))
        if isinstance(orig_frame, np.ndarray) and orig_frame.flags.writeable:
            orig_frame[...] = out[:H, :W]
        return out

    DEBUG_MAX_BOXES = 64

    def _global_motion_buffers(self, ctx) -> dict:
        if self._gm_bufs is None or self._gm_bufs[0] is not ctx:
            self._free_global_motion_buffers()
            n0 = ctx.W * ctx.H
            sizes = dict(res=_lib.MOTION_DTYPE.itemsize, H=72, ok=4, M=48, gray=n0, flow=8 * n0)
            if self.debug_path is not None:                             # _debug_frame's block: 12 + 8 + 18 bytes per pixel and the table
                sizes["debug"] = 38 * n0 + 32 * self.DEBUG_MAX_BOXES
            self._gm_bufs = (ctx, {k: ctx.alloc(v) for k, v in sizes.items()})
        return self._gm_bufs[1]

    def _free_global_motion_buffers(self) -> None:
        if self._gm_bufs is not None:
            ctx, bufs = self._gm_bufs
            self._gm_bufs = None
            if ctx.alive:
                for buf in bufs.values():
                    buf.free()

    def _no_global_motion(self, what: str) -> None:
        if self.detector.is_homography_based():
            raise NotImplementedError(f"{what} runs the FoE branch only; the global-motion branch (algorithm HOMOGRAPHY) is run_detection() "
                                      "or run_detection_batched(batch)")

    # -- the global-motion branch, `batch` frames per enqueue ---------------------------------------------------------------------------
    GM_MESSAGE = "frame {}: the sampled flow vectors do not determine a homography"

    def _run_global_motion_batched(self, batch: int) -> Dict[int, FrameResult]:
        """_run_global_motion with the frame indices taken `batch` at a time, two buffer sets: batch k + 1's upload and step are enqueued
        before the host waits for batch k's records (one marker per set, recorded behind the set's downloads).  A dataset that hands out
        frame pairs and whose flow seam is Farneback on them (frame_pair(i); attribute use_farneback true or absent) goes through the
        fused call, frames in and records out (mav_global_motion_batch_dev; consecutive pairs that share their frame objects are sent as
        one run of frames).  Any other dataset hands the host float32 fields of get_flow_uv(i) to one gather upload in front of
        mav_global_motion_step_dev; a device handle of the flow seam is read back and sent with them; a field of another dtype is a
        ValueError (run_detection() serves it).  Per-frame state as the one-frame loop leaves it, in frame order: get_annotation(i),
        detection_windows[i], detection_iou[i], detector.homography / confidence / flow_max / iou, cluster_vis files with a
        processed_path (png_encoder="device": deflated from the gray planes where they are, one channel; they decode to the same
        pixels, and detector.cluster_vis, which only the host encoder brings back, stays as it was).  A frame whose fit fails ends the
        loop as it ends the one-frame loop: every earlier frame is stored and written,
        frame_index is the failing index, nothing of later frames is stored."""
        det = self.detector
        self._no_blobs_here()
        self._no_roc_here()
        if self.debug_mode:
            raise NotImplementedError("debug_mode in the global-motion branch draws with cv2.rectangle and writes a six-image mosaic "
                                      "(processor.py:295-301): not reproduced")
        if self.debug_path is not None:
            raise NotImplementedError("debug_path writes the debug frame of run_detection(), one frame at a time; run_detection_batched "
                                      "does not compose it")
        if det.use_sparse_of:
            raise NotImplementedError("run_detection_batched takes the pairs from the flow field at detector.coords; use_sparse_of (pairs from "
                                      "the sequential tracker, frame after frame) is served by run_detection()")
        batch = int(batch)
        if batch < 1:
            raise ValueError(f"batch must be >= 1, got {batch}")
        idx = list(range(self.frame_index, self.dataset.N - 1))
        if not idx:
            return self.detection_results
        fused = hasattr(self.dataset, "frame_pair") and bool(getattr(self.dataset, "use_farneback", True))
        ctx = self._own_ctxs(batch, 1)[0]
        slots = self._global_motion_slots(ctx, batch, fused)
        pending = deque()
        try:
            for k, b0 in enumerate(range(0, len(idx), batch)):
                pending.append(self._submit_global_motion(ctx, slots[k % 2], idx[b0:b0 + batch], fused))
                while len(pending) > 1:
                    self._collect_global_motion(ctx, *pending.popleft())
            while pending:
                self._collect_global_motion(ctx, *pending.popleft())
        finally:
            for slot, _, _ in pending:                       # a failed frame: what is in flight behind it finishes, nothing of it is kept
                slot["fence"].wait()
            self._flush_images()
        return self.detection_results

    def _global_motion_slots(self, ctx, batch: int, fused: bool) -> list:
        """The two buffer sets of the batched loop on `ctx` (kept until release() or until the loop moves to another context)."""
        key = (ctx, batch, fused, self.png_encoder, self.processed_path is not None)
        cur = self._gm_slots
        if cur is not None and cur[0][0] is ctx and cur[0][1:] == key[1:]:
            return cur[1]
        self._free_global_motion_slots()
        n0, B = ctx.W * ctx.H, batch
        pin = lambda shape, dtype: _lib._pinned.empty(ctx, shape, dtype)
        slots = []
        for _ in range(2):
            # fused: prev frames then next frames, or a run of B + 1 frames; else the B flow fields
            s = dict(dev=dict(src=ctx.alloc(2 * B * n0 if fused else 8 * B * n0), H=ctx.alloc(72 * B), ok=ctx.alloc(4 * B), gray=ctx.alloc(B * n0),
                              res=ctx.alloc(_lib.MOTION_DTYPE.itemsize * B)),
                     res=pin((B,), _lib.MOTION_DTYPE), H=pin((B, 3, 3), np.float64), ok=pin((B,), np.int32), fence=pipeline._Fence(ctx))
            if self.processed_path is not None and self.png_encoder == "device":
                s["dev"]["png"] = ctx.alloc(ctx.lib.mav_png_bound(ctx.W, ctx.H, 1) * B)
                s["dev"]["index"] = ctx.alloc(16 * B)
                s["index"] = pin((B, 2), np.uint64)
            elif self.processed_path is not None:
                s["gray"] = pin((B, ctx.H, ctx.W), np.uint8)
            slots.append(s)
        self._gm_slots = (key, slots)
        return slots

    def _free_global_motion_slots(self) -> None:
        if self._gm_slots is not None:
            (ctx, *_), slots = self._gm_slots
            self._gm_slots = None
            for s in slots:
                if ctx.alive:
                    s["fence"].wait()
                    for buf in s["dev"].values():
                        buf.free()
                s["fence"].destroy()

    def _submit_global_motion(self, ctx, slot, ids, fused: bool):
        """Upload and step of frames `ids` on buffer set `slot` (idle: its last batch has been collected), the downloads of what the host
        reads, the set's marker.  -> (slot, ids, frames)."""
        det, dev, n, n0 = self.detector, slot["dev"], len(ids), ctx.W * ctx.H
        lib, h = ctx.lib, ctx.h
        # the frames the reference's loop draws on, one get_frame() per frame index as it calls it (only when they are drawn)
        frames = [self.dataset.get_frame() for _ in ids] if self.processed_path is not None else None
        optimize = bool(det.use_optimization)
        if fused:
            pairs = [self.dataset.frame_pair(i) for i in ids]
            prev = pipeline._as_frames([p[0] for p in pairs], ctx.H, ctx.W, "prev")
            nxt = pipeline._as_frames([p[1] for p in pairs], ctx.H, ctx.W, "next")
            run = all(pairs[k][1] is pairs[k + 1][0] for k in range(n - 1))        # one run of n + 1 frames (a video)
            arrs = prev + nxt[-1:] if run else prev + nxt
            _lib.check(lib.mav_upload_gather(h, dev["src"].ptr, pipeline._ptr_array(arrs), len(arrs), n0, 0))
            _lib.check(lib.mav_upload_fence(h))
            ctx.global_motion_batch_dev(dev["src"].ptr, dev["src"].ptr + (1 if run else n) * n0, det.coords, n, dev["res"].ptr, optimize=optimize,
                                        H_ptr=dev["H"].ptr, ok_ptr=dev["ok"].ptr, gray_ptr=dev["gray"].ptr)
        else:
            fields = []
            for i in ids:
                f = self.dataset.get_flow_uv(i)
                if f is None:
                    raise ValueError("Could not load flow field.")
                if f.dtype != np.float32:
                    raise ValueError(f"frame {i}: run_detection_batched() takes float32 flow fields, got {f.dtype}; run_detection() serves "
                                     "a field of another dtype (host float64 arithmetic)")
                a = np.ascontiguousarray(np.asarray(f))                            # (a device handle of the flow seam is read back here)
                if a.shape != (ctx.H, ctx.W, 2):
                    raise ValueError(f"frame {i}: expected a ({ctx.H}, {ctx.W}, 2) flow field, got {a.shape}")
                fields.append(a)
            _lib.check(lib.mav_upload_gather(h, dev["src"].ptr, pipeline._ptr_array(fields), n, 8 * n0, 0))
            _lib.check(lib.mav_upload_fence(h))
            ctx.global_motion_step(dev["src"].ptr, det.coords, n, dev["res"].ptr, optimize=optimize, H_ptr=dev["H"].ptr, ok_ptr=dev["ok"].ptr,
                                   gray_ptr=dev["gray"].ptr)
        if "index" in slot:
            _lib.check(lib.mav_png_encode_dev(h, dev["gray"].ptr, n, 1, dev["png"].ptr, dev["png"].nbytes, dev["index"].ptr))
        for name in ("res", "H", "ok", "gray", "index"):
            if name in slot:
                host = slot[name][:n]
                _lib.check(lib.mav_download_async(h, _lib._ptr(host), dev[name].ptr, host.nbytes))
        slot["fence"].record()
        return slot, ids, frames

    def _collect_global_motion(self, ctx, slot, ids, frames) -> None:
        """Batch `ids` on `slot` has finished: its frames in frame order, as the one-frame loop leaves them."""
        det = self.detector
        slot["fence"].wait()
        for k, i in enumerate(ids):
            self.dataset.get_annotation(i)
            if not int(slot["ok"][k]):
                self.frame_index = i
                raise RuntimeError(self.GM_MESSAGE.format(i))
            det.homography = np.array(slot["H"][k])
            det.confidence = np.ones((det.coords.shape[0], 1), np.uint8)
            rec = slot["res"][k]
            det.flow_max = (int(rec["max_row"]), int(rec["max_col"]))
            x, y, w, h = (int(v) for v in rec["opt_window"])
            window = utils.Rectangle.from_points((x, y), (x + w, y + h))
            for gt in self.dataset.ground_truth:
                det.iou = utils.Rectangle.calculate_iou(window, gt)
            self.detection_windows[i] = window
            if hasattr(det, "iou"):
                self.detection_iou[i] = det.iou
            if self.processed_path is not None:
                det.prev_frame = frames[k]
                if "index" in slot:                          # the stream alone crosses PCIe; the pool adds the chunk framing
                    off, size = (int(v) for v in slot["index"][k])
                    z = np.empty(size, np.uint8)
                    _lib.check(ctx.lib.mav_memcpy_d2h(ctx.h, _lib._ptr(z), slot["dev"]["png"].ptr + off, size))
                    self._queue_png(self.processed_path, i, (ctx.W, ctx.H, 1, z.tobytes()))
                else:
                    det.cluster_vis = np.repeat(slot["gray"][k][..., None], 3, axis=2)
                    self._queue_png(self.processed_path, i, det.cluster_vis)
            self.frame_index = i + 1

    @property
    def _renders(self) -> bool:
        """Images or processed frames are rendered from what a step left resident: the loops finish each step before the next."""
        return self.images_path is not None or self.processed_path is not None

    @staticmethod
    def _blob_list(records) -> list:
        """mav_blob records -> [(Rectangle, area, (cx, cy))]: the box in get_simple_bounding_box's convention, the exact centroid."""
        return [(im_helpers.blob_rectangle(b), int(b["area"]), (int(b["sum_x"]) / int(b["area"]), int(b["sum_y"]) / int(b["area"])))
                for b in records]

    def _no_blobs_here(self) -> None:
        if self.blobs is not None:
            raise NotImplementedError("blobs= labels the FoE branch's fixed mask; the global-motion branch (algorithm HOMOGRAPHY) has no mask")

    def _no_roc_here(self) -> None:
        if self.roc is not None:
            raise NotImplementedError("roc= sweeps the FoE branch's fixed mask; the global-motion branch (algorithm HOMOGRAPHY) has no mask")

    def roc_rates(self) -> dict:
        """The sweep's rates: tpr / fpr per frame (n, Ka, Km) float64 = tp / pos and fp / neg as calculate_tpr_fpr divides (NaN where a
        frame has no positives / negatives), frames in index order; tpr_pooled / fpr_pooled (Ka, Km): the sums over the frames, then
        one division."""
        if self.roc is None:
            raise ValueError("roc_rates() needs Processor(roc=dict(angles=, mags=))")
        ka, km = self.roc["angles"].size, self.roc["mags"].size
        c = (np.stack([self.roc_counts[i] for i in sorted(self.roc_counts)]) if self.roc_counts else np.zeros((0, ka, km, 4), np.int64)).astype(np.float64)
        tot = c.sum(axis=0)
        with np.errstate(divide="ignore", invalid="ignore"):
            return dict(angles=self.roc["angles"], mags=self.roc["mags"], tpr=c[..., 2] / c[..., 0], fpr=c[..., 3] / c[..., 1],
                        tpr_pooled=tot[..., 2] / tot[..., 0], fpr_pooled=tot[..., 3] / tot[..., 1])

    def _finish_frame(self, pipe, i: int, ticket, sky, orig_frame) -> None:
        out = pipe.collect(ticket)
        if self.roc is not None:
            self.roc_counts[i] = out["roc"][0]
        if self.blobs is not None:
            self.detection_blobs[i] = self._blob_list(out["blobs"][0])
        rec = out["results"][0]
        self.estimate_fixed, self.total_mask = out["mask_fixed"][0], out["mask_dyn"][0]
        r = self._fill_result(i, (float(rec["foe"][0]), float(rec["foe"][1])), sky, out["counts_fixed"][0], out["counts_dyn"][0])
        self.detection_boxes[i] = utils.Rectangle.from_box(rec["box"])
        self._store(i, r)
        ctx = pipe.pipes[ticket[0]].ctx
        dev = self.png_encoder == "device"
        if self.images_path is not None:
            self._write_images([i], ctx.render_last_png(1, wrap=False) if dev else ctx.render_last(1))
        if self.processed_path is not None:
            self._write_processed([i], *(ctx.overlay_last_png(orig_frame, [r.foe_gt], wrap=False) if dev else ctx.overlay_last(orig_frame, [r.foe_gt])))

    def run_detection_staged(self) -> Dict[int, FrameResult]:
        """The same loop through the reference-named calls one by one (Detector.derotate, get_FOE_dense, the masks): every call
        ships its arrays across PCIe, as a maintainer who only swaps the imports would get.  Kept as the parity check of
        those shims; run_detection() is the fast form."""
        self._no_global_motion("run_detection_staged")
        while self.is_active():
            i = self.frame_index
            orig_frame = self.dataset.get_frame()
            self.flow_uv = self.dataset.get_flow_uv(i)
            if self.flow_uv is None:
                raise ValueError("Could not load flow field.")
            self._staged_frame(i, orig_frame)
        self._flush_images()
        return self.detection_results

    def _staged_frame(self, i: int, orig_frame) -> None:
        """One frame through the reference-named calls (processor.py:306-341), flow already in self.flow_uv."""
        self._derot_frame = i
        self.flow_uv_derotated = self.detector.derotate(i - self.frame_step_size, i, np.asarray(self.flow_uv))
        if self.validation == "device":
            _, skies, scores = self._validation_tail(self._own_ctxs(1, 1), [i])
            self.sky_mask, sky = skies[0], scores[0]
        else:
            self.sky_mask = self.dataset.get_sky_segmentation(i)
            sky = self.dataset.validate_sky_segment(self.sky_mask, utils.assert_type(self.dataset.get_depth(i)))
        foe = self.focus_of_expansion.get_FOE_dense(self.flow_uv_derotated)
        fixed, total = self.focus_of_expansion.get_masks(self.flow_uv_derotated, foe, self.sky_mask)
        self.estimate_fixed, self.total_mask = fixed, total
        if self.blobs is not None:                            # the fixed mask get_masks left on the helpers' context: not moved again
            b = self.blobs
            out = im_helpers._ctx(fixed.shape[1], fixed.shape[0]).components_last(1, "fixed", b.connectivity, b.min_area, b.max_blobs)
            self.detection_blobs[i] = self._blob_list(out["blobs"][0])
        if self.roc is not None:                              # the field, FoE and sky get_masks left on the helpers' context: not moved again
            seg = self._tails[i]["seg"] if i in self._tails else self._segmentation(i)[0]
            out = im_helpers._ctx(fixed.shape[1], fixed.shape[0]).roc_sweep_last(1, seg, self.roc["angles"], self.roc["mags"])
            self.roc_counts[i] = out["counts"][0]
        r = self._fill_result(i, foe, sky, estimate_fixed=fixed, total_mask=total)
        self._store(i, r)
        if self.images_path is not None:                      # the reference-named helpers, as processor.py:364-374 reads
            phi = self.focus_of_expansion.get_phi(self.flow_uv_derotated, foe)
            with np.errstate(invalid="ignore"):               # an empty mask: 0 / 0 -> 0, as in the reference
                result = im_helpers.to_rgb(255 * np.asarray(fixed))
            self._write_images([i], dict(result=result[None], flow=im_helpers.get_flow_vis(self.flow_uv_derotated)[None],
                                         phi=im_helpers.apply_colormap(im_helpers.to_rgb(phi, max_value=180.0))[None]))
        if self.processed_path is not None:                   # processor.py:376-394 on a copy: the dataset's array stays as it is
            frame = np.array(orig_frame, copy=True)
            with np.errstate(invalid="ignore"):
                result_img = im_helpers.to_rgb(255 * np.asarray(fixed))
            for img in (frame, result_img):
                self.focus_of_expansion.draw_FoE(img, foe, [0, 255, 0])
                self.focus_of_expansion.draw_FoE(img, r.foe_gt, [255, 255, 255])
            mask_rgb = np.copy(frame)
            mask_rgb[fixed] = (150, 0, 150)
            mask_vis = im_helpers.add_weighted(frame, 0.2, mask_rgb, 1.0 - 0.2, 0.0)
            self._write_processed([i], [mask_vis], [np.sum(result_img) > 0])
        self.frame_index += 1

    def run_detection_batched(self, batch: Optional[int] = None) -> Dict[int, FrameResult]:
        """The same loop with frame pairs in flight `batch` at a time through the fused entry point (frames -> flow -> derotation ->
        FoE -> masks -> box -> counts), two batches in flight: while batch k computes, batch k + 1's frames are gathered from the
        dataset's arrays and cross PCIe, and batch k - 1's FrameResults are filled in.  Needs a dataset that hands out frame pairs
        (frame_pair(i)).  The sample coordinates are drawn per frame in frame order, as get_FOE_dense draws them.
        batch None: 8 pairs.  With algorithm HOMOGRAPHY and a batch given: the global-motion branch `batch` frames at a time
        (_run_global_motion_batched); without one the call refuses that algorithm as it always has -- the branch's buffer sets and its
        context are sized by the batch, and no default is chosen for the caller."""
        from collections import deque
        if self.detector.is_homography_based():
            if batch is None:
                self._no_global_motion("run_detection_batched() without a batch")
            return self._run_global_motion_batched(batch)
        batch = 8 if batch is None else batch
        W, H = self.dataset.capture_size
        idx = list(range(self.frame_index, self.dataset.N - 1))
        # small batches (one pair at 720p / 1080p ...) are spread over 2 - 3 contexts taken in turn; a big batch keeps two pairs in
        # flight inside its one context
        pipe = self._pipeline(self._own_ctxs(batch, pipeline.auto_lanes(W, H, batch)), batch)
        pending = deque()
        for b0 in range(0, len(idx), batch):
            ids = idx[b0:b0 + batch]
            pairs = [self.dataset.frame_pair(i) for i in ids]
            # the frames the reference's loop draws on, one get_frame() per frame index as it calls it (only when they are drawn)
            frames = [self.dataset.get_frame() for _ in ids] if self.processed_path is not None else None
            samples = np.empty((len(ids), 2000, 2), np.uint32)
            for k in range(len(ids)):                      # same draws, same order as get_FOE_dense
                samples[k, :, 0] = np.random.randint(0, H, 2000)
                samples[k, :, 1] = np.random.randint(0, W, 2000)
            dts = np.array([self.dataset.get_delta_time(i) for i in ids], np.float64)
            # frame 0 is never derotated and runs in float32 (detector.py:80-81): flagged per pair
            omega = np.stack([np.asarray(self.dataset.get_angular_difference(i - self.frame_step_size, i), np.float64) / dt
                              for i, dt in zip(ids, dts)])
            if self.validation == "device":
                kw, skies, sky_scores = self._validation_tail(pipe.ctxs, ids)
            else:
                kw, skies = self._sky_and_gt(ids)
                sky_scores = [self.dataset.validate_sky_segment(sk, utils.assert_type(self.dataset.get_depth(i))) for i, sk in zip(ids, skies)]
            ticket = pipe.submit(samples, prev=[p[0] for p in pairs], nxt=[p[1] for p in pairs], omega=omega, dt=dts,
                                 frame0=[i < 1 for i in ids], **kw)
            pending.append((ids, ticket, sky_scores, frames))
            while len(pending) > (0 if self._renders else pipe.depth):     # images: rendered behind the batch's step
                self._finish_batch(pipe, *pending.popleft())
        while pending:
            self._finish_batch(pipe, *pending.popleft())
        self.frame_index = self.dataset.N - 1
        self._flush_images()
        return self.detection_results

    def _finish_batch(self, pipe, ids, ticket, sky_scores, frames) -> None:
        out = pipe.collect(ticket)
        gts = []
        for k, i in enumerate(ids):
            rec = out["results"][k]
            r = self._fill_result(i, (float(rec["foe"][0]), float(rec["foe"][1])), sky_scores[k], out["counts_fixed"][k], out["counts_dyn"][k])
            self.detection_boxes[i] = utils.Rectangle.from_box(rec["box"])
            if self.blobs is not None:
                self.detection_blobs[i] = self._blob_list(out["blobs"][k])
            if self.roc is not None:
                self.roc_counts[i] = out["roc"][k]
            self._store(i, r)
            gts.append(r.foe_gt)
        ctx = pipe.pipes[ticket[0]].ctx
        dev = self.png_encoder == "device"
        if self.images_path is not None:
            self._write_images(ids, ctx.render_last_png(len(ids), wrap=False) if dev else ctx.render_last(len(ids)))
        if self.processed_path is not None:
            frames = np.stack(frames)
            self._write_processed(ids, *(ctx.overlay_last_png(frames, gts, wrap=False) if dev else ctx.overlay_last(frames, gts)))
        self.estimate_fixed, self.total_mask = out["mask_fixed"][-1], out["mask_dyn"][-1]     # of the last frame, as the loop leaves them

    def release(self) -> None:
        self._flush_images()
        if self._png_pool is not None:
            self._png_pool.shutdown()
            self._png_pool = None
        self._free_global_motion_buffers()
        self._free_global_motion_slots()
        self.detector._free_dev_buffers()
        if self.radial_error is not None:
            self.radial_error.close()
            self.radial_error = None
        self._close_pipes()
        for c in self._ctxs:
            c.close()
        self._ctxs = []
        self.dataset.release()
