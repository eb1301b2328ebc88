"""The reference's src/airsim_optical_flow.py over libmavflow: the ground-truth optical flow of an AirSim recording from its depth
buffers, the two camera states' view-projection matrices and the MAV's velocity.  Same names and argument meaning; the per-pixel
reprojection (screen_to_world, world_to_screen: the reference's float64 numpy over the full frame) runs in one HIP kernel
(Context.gt_flow, include/mavflow_truth.h), bit for bit.  Reading AirSim's .pfm depth files is not here: the depth comes from the
dataset (get_depth), the segmentation likewise."""
from __future__ import annotations

import json
import os
from typing import Any, Dict, Tuple

import numpy as np

from . import frame_source, im_helpers, utils


class Vector3r:
    """airsim.types.Vector3r as far as write_flow uses it: three fields and a product with a scalar."""

    def __init__(self, x_val: float = 0.0, y_val: float = 0.0, z_val: float = 0.0):
        self.x_val, self.y_val, self.z_val = x_val, y_val, z_val

    def __mul__(self, k):
        return Vector3r(self.x_val * k, self.y_val * k, self.z_val * k)


def get_state(filepath: str) -> Dict[str, Any]:
    with open(filepath, "r") as f:
        return json.load(f)


def get_view_proj_mat(state: dict) -> np.ndarray:
    """the camera's view-projection matrix of a state file: UE4 prints it row-vector style, hence the transpose (:81-85)"""
    view_proj_str = state["Drone1"]["ue4"]["viewProjectionMatrix"]
    view_proj = view_proj_str.replace("[", "").replace("]", "").strip().split(" ")
    return np.array([float(x) for x in view_proj]).reshape((4, 4)).T


def _pixel_grid(screen_res) -> np.ndarray:
    """write_flow's coords (:114-116): (W, H, 2) with [x, y] = (x, y)"""
    W, H = int(screen_res[0]), int(screen_res[1])
    return np.stack((np.tile(np.arange(W), (H, 1)), np.tile(np.arange(H), (W, 1)).T)).swapaxes(0, 2)


def calculate_flow(view_proj1: np.ndarray, view_proj2: np.ndarray, screen_res: Tuple[int, int], screen_pos2: np.ndarray, depth_img: np.ndarray,
                   drone_displacement, segmentation: np.ndarray) -> np.ndarray:
    """screen_pos1 - screen_pos2 as (W, H, 2) float64 from the reference's transposed (W, H) depth (float32) and segmentation arrays.
    screen_pos2 must be the pixel grid, which is what write_flow passes: the kernel derives the positions from the pixel index
    (NotImplementedError otherwise)."""
    W, H = int(screen_res[0]), int(screen_res[1])
    pos = np.asarray(screen_pos2)
    if pos.shape != (W, H, 2) or not np.array_equal(pos, _pixel_grid((W, H))):
        raise NotImplementedError("calculate_flow: screen_pos2 other than the pixel grid of screen_res is not implemented")
    depth = np.asarray(depth_img)
    if depth.shape != (W, H):
        raise ValueError(f"calculate_flow: expected a transposed ({W}, {H}) depth image, got {depth.shape}")
    seg = np.ascontiguousarray((np.asarray(segmentation) > 0).T.astype(np.uint8))
    d = drone_displacement
    out = im_helpers._ctx(W, H).gt_flow(np.ascontiguousarray(depth.T), seg, view_proj1, view_proj2, (d.x_val, d.y_val, d.z_val), dtype=np.float64)
    return -out.swapaxes(0, 1)                    # the library returns write_flow's `-result.swapaxes(0, 1)`


def write_flow(dataset) -> None:
    """The reference's loop (:109-149): for every state but the last, the flow between states[i - 1] and states[i] -- index 0 takes its
    first state from the end of the list, as the reference's indexing does -- written as image_%05d.flo with its colour rendering
    beside it.  The depth is dataset.get_depth(i) times 100 (in float32, as the reference scales the .pfm's metres), the segmentation
    dataset.get_segmentation(i) as a grayscale array."""
    print("Calculating ground truth optical flow...")
    screen_res = dataset.capture_size
    states = [x for x in dataset.get_state_filenames() if "timestamp" not in x]
    W, H = int(screen_res[0]), int(screen_res[1])
    ctx = im_helpers._ctx(W, H)
    for d in (dataset.gt_of_path, dataset.gt_of_vis_path):
        os.makedirs(d, exist_ok=True)
    for i, _ in enumerate(states[1:]):
        if i % max(int(len(states[1:]) / 10), 1) == 0 and getattr(dataset, "logger", None) is not None:
            dataset.logger.info(f"{i / len(states[1:]) * 100:.2f}%")
        state1 = get_state(states[i - 1])
        state2 = get_state(states[i])
        view_proj1 = get_view_proj_mat(state1)
        view_proj2 = get_view_proj_mat(state2)
        delta_time = dataset.get_delta_time(i)
        drone_velocity = state1["Drone2"]["ue4"]["linearVelocity"]
        drone_displacement = Vector3r(drone_velocity["X"], drone_velocity["Y"], drone_velocity["Z"]) * delta_time * 100
        if np.isnan(drone_displacement.x_val):
            drone_displacement = Vector3r()
        depth = np.asarray(dataset.get_depth(i))
        if depth.dtype != np.float32:
            raise TypeError(f"write_flow: the depth buffer must be float32 (as AirSim's .pfm is), got {depth.dtype}")
        seg = np.asarray(dataset.get_segmentation(i))
        if seg.ndim == 3:
            raise ValueError("write_flow: the segmentation must be a grayscale (H, W) array")
        result = ctx.gt_flow(depth, (seg > 0).astype(np.uint8), view_proj1, view_proj2,
                             (drone_displacement.x_val, drone_displacement.y_val, drone_displacement.z_val), depth_scale=100.0, dtype=np.float64)
        utils.write_flow(f"{dataset.gt_of_path}/image_{i:05d}.flo", result)
        frame_source.imwrite(f"{dataset.gt_of_vis_path}/image_{i:05d}.png", im_helpers.get_flow_vis(result))
