"""The cases of the ground-truth and radial-error tests as a table, with the launchers' decisions (csrc/kernels_truth.hip:
launch_gt_flow, launch_radial_hist) restated as predicates, so that tests/test_truth_cases_cpu.py can say without a GPU that every
dispatch form is reached and every histogram field keeps its pixels away from the bin edges (the device's atan2f is not glibc's: a
pixel a few float32 ulps from an edge could fall either way, so no field has one).  Inputs are seeded and built once per process."""
import functools
import os
import re
from dataclasses import dataclass

import numpy as np

import truth_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INTERNAL = os.path.join(ROOT, "mav-detection_amd", "csrc", "mavflow_internal.h")

# the launchers' constants (held against csrc/mavflow_internal.h by the CPU test)
GT_FLOW_BLOCK, GT_FLOW_GRID_CAP = 256, 1024
RADIAL_STEP, RADIAL_GRID_CAP, RADIAL_LDS_CELLS = 2048, 256, 32768
MIN_EDGE_DISTANCE_PX, MIN_EDGE_DISTANCE_DEG = 1e-4, 1e-3


def internal_constants() -> dict:
    with open(INTERNAL) as f:
        return {k: int(v) for k, v in re.findall(r"#define (MAV_GT_FLOW_GRID_CAP|MAV_RADIAL_LDS_CELLS|MAV_RADIAL_GRID_CAP) (\d+)", f.read())}


# ---- the reprojection --------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class GtCase:
    name: str
    W: int
    H: int
    B: int = 1
    seg: bool = True
    scale: float = 100.0

    @property
    def npx(self):
        return self.W * self.H

    def forms(self) -> set:
        """launch_gt_flow's decisions for this shape (each output depth is run by every test)"""
        blocks = -(-self.npx // GT_FLOW_BLOCK)
        f = {"loop" if blocks > GT_FLOW_GRID_CAP else "one pass", "seg" if self.seg else "no seg", "batch" if self.B > 1 else "single"}
        if self.npx % GT_FLOW_BLOCK:
            f.add("ragged tail")
        if blocks == 1:
            f.add("one workgroup")
        return f


GT_CASES = (GtCase("1x1", 1, 1), GtCase("5x3", 5, 3, seg=False), GtCase("97x71", 97, 71), GtCase("516x37", 516, 37, scale=1.0),
            GtCase("64x16", 64, 16),                                    # a whole number of workgroups: no tail
            GtCase("past the grid cap", 7087, 37),                      # 262 219 pixels: one more row of workgroups than the cap
            GtCase("batch 3", 97, 71, B=3))
GT_FORMS = {"loop", "one pass", "seg", "no seg", "batch", "single", "ragged tail", "one workgroup"}


def _rotation(angles):
    cx, cy, cz = np.cos(angles)
    sx, sy, sz = np.sin(angles)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def view_proj(seed, W, H):
    """a reversed-z perspective projection times a small rotation and a translation (tools/gen_golden_truth.py's recipe)"""
    r = np.random.default_rng(seed)
    P = np.array([[1.0, 0, 0, 0], [0, W / H, 0, 0], [0, 0, 0, 10.0], [0, 0, 1.0, 0]])
    V = np.eye(4)
    V[:3, :3] = _rotation(r.normal(0, 0.02, 3))
    V[:3, 3] = r.normal(0, 30.0, 3)
    return P @ V


@functools.lru_cache(maxsize=None)
def gt_inputs(name: str) -> dict:
    """depth (B, H, W) float32, seg (B, H, W) uint8 or None, vp1 / vp2 / inv (B, 4, 4), disp (B, 3), scale; and "ref64": truth_ref's field.
    Every pair of a batch has a parameter block of its own.  Nothing writes them."""
    c = {k.name: k for k in GT_CASES}[name]
    rng = np.random.default_rng(7000 + [k.name for k in GT_CASES].index(name))
    depth = rng.uniform(1, 200, (c.B, c.H, c.W)).astype(np.float32)
    if c.scale == 1.0:
        depth = depth * np.float32(100)
    seg = ((rng.random((c.B, c.H, c.W)) < 0.2) * rng.integers(1, 256, (c.B, c.H, c.W))).astype(np.uint8) if c.seg else None
    vp1 = np.stack([view_proj(7100 + 2 * b, c.W, c.H) for b in range(c.B)])
    vp2 = np.stack([view_proj(7101 + 2 * b, c.W, c.H) for b in range(c.B)])
    inv = np.stack([np.linalg.inv(m) for m in vp2])
    disp = rng.normal(0, 8, (c.B, 3))
    ref = np.stack([R.gt_flow(depth[b], None if seg is None else seg[b], vp1[b], inv[b], disp[b], c.scale) for b in range(c.B)])
    v = dict(depth=depth, seg=seg, vp1=vp1, vp2=vp2, inv=inv, disp=disp, scale=c.scale, ref64=ref)
    for a in v.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return v


def fixture_inputs(g, name: str) -> dict:
    """case `name` of tests/golden/truth.npz in the same form (B = 1), "ref64" = the reference's own result as write_flow turns it"""
    res = g[f"{name}_result"]
    return dict(depth=g[f"{name}_depth"][None], seg=g[f"{name}_seg"][None], vp1=g[f"{name}_vp1"][None], vp2=g[f"{name}_vp2"][None],
                inv=g[f"{name}_inv"][None], disp=g[f"{name}_disp"][None], scale=float(g[f"{name}_scale"]),
                ref64=np.ascontiguousarray(-res[..., [0, 1]].swapaxes(0, 1))[None])


# ---- the histogram ---------------------------------------------------------------------------------------------------------------------------
DEFAULT_EDGES = (R.DEFAULT_MAG_EDGES, R.DEFAULT_ERR_EDGES)
EDGE_SETS = {
    "default": DEFAULT_EDGES,                                                            # 159 x 159 = 25 281 cells: LDS counters
    "3 edges": (np.array([0.5, 2.5, 10.0]), np.array([-20.0, 0.5, 20.0])),               # the smallest lists but one; magnitudes below the range exist
    "257 x 256": (np.linspace(0, 10, 257), np.linspace(-20, 20, 256)),                   # 65 280 cells: past what LDS holds
}


@dataclass(frozen=True)
class HistCase:
    name: str
    W: int
    H: int
    B: int = 1
    edges: str = "default"
    field: str = "scene"         # "scene": targets inside random bins; "one cell": a constant field
    sky: bool = True

    @property
    def npx(self):
        return self.W * self.H

    def grid(self) -> int:
        """radial_hist_grid"""
        return min(-(-self.npx // RADIAL_STEP), max(RADIAL_GRID_CAP // self.B, 1))

    def forms(self) -> set:
        em, ee = EDGE_SETS[self.edges]
        f = {"lds counters" if (len(em) - 1) * (len(ee) - 1) <= RADIAL_LDS_CELLS else "table counters",
             "loop" if -(-self.npx // RADIAL_STEP) > self.grid() else "one pass", "sky" if self.sky else "no sky",
             "batch" if self.B > 1 else "single", "one cell per wave" if self.field == "one cell" else "mixed waves"}
        if self.npx % RADIAL_STEP:
            f.add("ragged tail")
        return f


HIST_CASES = (HistCase("1x1", 1, 1), HistCase("5x3", 5, 3, sky=False), HistCase("97x71", 97, 71), HistCase("516x37 one cell", 516, 37, B=3, field="one cell"),
              HistCase("64x32", 64, 32),                                                  # one whole step: no tail
              HistCase("past the grid cap", 4706, 37, B=3),                                # 174 122 pixels a pair: one more step than 85 workgroups take
              HistCase("3 edges", 97, 71, edges="3 edges"), HistCase("257 x 256", 97, 71, B=2, edges="257 x 256"),
              HistCase("257 x 256 one cell", 53, 37, edges="257 x 256", field="one cell", sky=False))
HIST_FORMS = {"lds counters", "table counters", "loop", "one pass", "sky", "no sky", "batch", "single", "one cell per wave", "mixed waves", "ragged tail"}


def scene(seed, W, H, B, mag_edges, err_edges):
    """flow, ground truth (B, H, W, 2) float32 and sky (B, H, W) bool whose (magnitude, error) pairs aim at the inside of bins (0.2 .. 0.8 of
    the bin's width from its left edge); a tenth beyond the range on the high side of either axis, a twentieth below the errors' range
    and, where the magnitudes' range starts above zero, below it; angles cover the circle, so some errors wrap past +-180 degrees
    (they land a turn away: far outside)."""
    rng = np.random.default_rng(seed)
    shape = (B, H, W)
    bm, be = rng.integers(0, len(mag_edges) - 1, shape), rng.integers(0, len(err_edges) - 1, shape)
    tm = mag_edges[bm] + (mag_edges[bm + 1] - mag_edges[bm]) * rng.uniform(0.2, 0.8, shape)
    te = err_edges[be] + (err_edges[be + 1] - err_edges[be]) * rng.uniform(0.2, 0.8, shape)
    tm[rng.random(shape) < 0.1] += (mag_edges[-1] - mag_edges[0]) + 0.5
    te[rng.random(shape) < 0.1] += (err_edges[-1] - err_edges[0]) + 5.0
    te[rng.random(shape) < 0.05] -= 2 * (err_edges[-1] - err_edges[0]) + 10.0
    if mag_edges[0] > 0:
        low = rng.random(shape) < 0.05
        tm[low] = mag_edges[0] * rng.uniform(0.2, 0.8, int(low.sum()))
    ga, gm = rng.uniform(-np.pi, np.pi, shape), rng.uniform(0.5, 6, shape)
    gt = np.stack((gm * np.cos(ga), gm * np.sin(ga)), -1).astype(np.float32)
    fa = ga + np.deg2rad(te)
    flow = np.stack((tm * np.cos(fa), tm * np.sin(fa)), -1).astype(np.float32)
    return flow, gt, rng.random(shape) < 0.15


ONE_CELL_FLOW, ONE_CELL_GT = (3.0, 0.0), (1.5, 0.0)      # magnitude 3 (inside a bin of every edge set), error exactly 0 whatever atan2f is


@functools.lru_cache(maxsize=None)
def hist_inputs(name: str) -> dict:
    """flow, gt (B, H, W, 2) float32, sky (B, H, W) uint8 or None, mag_edges, err_edges; and "ref": truth_ref.radial_hist of them."""
    c = {k.name: k for k in HIST_CASES}[name]
    em, ee = EDGE_SETS[c.edges]
    if c.field == "one cell":
        flow = np.broadcast_to(np.array(ONE_CELL_FLOW, np.float32), (c.B, c.H, c.W, 2)).copy()
        gt = np.broadcast_to(np.array(ONE_CELL_GT, np.float32), (c.B, c.H, c.W, 2)).copy()
        sky = np.random.default_rng(9).random((c.B, c.H, c.W)) < 0.15
    else:
        flow, gt, sky = scene(8000 + [k.name for k in HIST_CASES].index(name), c.W, c.H, c.B, em, ee)
    sky = sky.astype(np.uint8) if c.sky else None
    v = dict(flow=flow, gt=gt, sky=sky, mag_edges=em, err_edges=ee, ref=R.radial_hist(flow, gt, sky, em, ee))
    for a in v.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return v
