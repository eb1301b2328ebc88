"""The reference-named layer over the truth kernels: mavflow.airsim_optical_flow.calculate_flow returns the reference's own arrays
(tests/golden/truth.npz), write_flow writes the .flo files of tests/truth_ref.py's fields for a three-state recording -- index 0 takes
its first state from the end of the list, as the reference's indexing does -- and Processor.analyze_radial_error accumulates what
Context.radial_error_hist returns."""
import json
import logging
import os

import numpy as np
import pytest

import truth_cases as T
import truth_ref as R

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "truth.npz")


def test_calculate_flow_returns_the_references_arrays():
    from mavflow import airsim_optical_flow as A
    g = np.load(GOLDEN, allow_pickle=False)
    for name in g["cases"]:
        raw, seg, scale = g[f"{name}_depth"], g[f"{name}_seg"], float(g[f"{name}_scale"])
        H, W = raw.shape
        depth = raw.T * 100 if scale == 100.0 else raw.T.copy()            # the generator's own lines: the reference's (W, H) float32 array
        got = A.calculate_flow(g[f"{name}_vp1"], g[f"{name}_vp2"], (W, H), A._pixel_grid((W, H)), depth, A.Vector3r(*g[f"{name}_disp"]), seg.T)
        assert got.shape == (W, H, 2) and got.dtype == np.float64 and R.same_bits(got, g[f"{name}_result"]), name
    with pytest.raises(NotImplementedError):
        A.calculate_flow(np.eye(4), np.eye(4), (5, 3), A._pixel_grid((5, 3)) + 1, np.ones((5, 3), np.float32), A.Vector3r(), np.zeros((5, 3), np.uint8))


def _state(vp, velocity):
    rows = " ".join("[" + " ".join(repr(float(v)) for v in r) + "]" for r in vp.T)      # UE4 prints the transpose (get_view_proj_mat undoes it)
    return {"Drone1": {"ue4": {"viewProjectionMatrix": rows}}, "Drone2": {"ue4": {"linearVelocity": dict(zip("XYZ", velocity))}}}


class _Recording:
    """what write_flow asks of a dataset: three states on disk, depth and segmentation per frame"""
    W, H, DT = 37, 23, 0.05

    def __init__(self, root):
        rng = np.random.default_rng(31)
        self.capture_size = (self.W, self.H)
        self.logger = logging.getLogger("t")
        self.gt_of_path, self.gt_of_vis_path = str(root / "optical-flow"), str(root / "optical-flow-vis")
        self.vps = [T.view_proj(900 + k, self.W, self.H) for k in range(3)]
        # pair i takes the velocity of states[i - 1]: the last state's for pair 0, the first state's (unknown: NaN) for pair 1
        self.velocities = [(float("nan"), 1.0, 1.0), (9.0, 9.0, 9.0), (-2.0, 0.5, 1.0)]
        self.files = []
        for k in range(3):
            path = root / f"state_{k:05d}.json"
            path.write_text(json.dumps(_state(self.vps[k], self.velocities[k])))
            self.files.append(str(path))
        self.depth = rng.uniform(1, 200, (2, self.H, self.W)).astype(np.float32)
        self.seg = ((rng.random((2, self.H, self.W)) < 0.25) * 180).astype(np.uint8)

    def get_state_filenames(self):
        return self.files[:2] + [os.path.join(os.path.dirname(self.files[0]), "timestamps.json")] + self.files[2:]

    def get_delta_time(self, i):
        return self.DT * (i + 1)

    def get_depth(self, i):
        return self.depth[i]

    def get_segmentation(self, i):
        return self.seg[i]


def test_write_flow_writes_the_restatements_fields(tmp_path):
    from mavflow import airsim_optical_flow as A
    from mavflow import frame_source, im_helpers, utils
    ds = _Recording(tmp_path)
    for k in range(3):                                                     # the state files hold the matrices digit for digit
        assert np.array_equal(A.get_view_proj_mat(A.get_state(ds.files[k])), ds.vps[k])
    A.write_flow(ds)
    assert sorted(os.listdir(ds.gt_of_path)) == ["image_00000.flo", "image_00001.flo"]
    for i, (first, second) in enumerate(((2, 0), (0, 1))):                 # states[i - 1], states[i]: index 0 starts at the END of the list
        v = np.array(ds.velocities[first])
        disp = np.zeros(3) if np.isnan(v[0]) else v * ds.get_delta_time(i) * 100
        want = R.gt_flow(ds.depth[i], ds.seg[i], ds.vps[first], np.linalg.inv(ds.vps[second]), disp, 100.0)
        ref_file = tmp_path / f"want_{i}.flo"
        utils.write_flow(str(ref_file), want)
        got = open(os.path.join(ds.gt_of_path, f"image_{i:05d}.flo"), "rb").read()
        assert got == ref_file.read_bytes(), i
        assert np.array_equal(utils.read_flow(os.path.join(ds.gt_of_path, f"image_{i:05d}.flo")), want.astype(np.float32))
        png = open(os.path.join(ds.gt_of_vis_path, f"image_{i:05d}.png"), "rb").read()
        assert png == frame_source.encode_png(im_helpers.get_flow_vis(want)), i
    assert np.isnan(ds.velocities[0][0])                                   # pair 1 ran on the NaN rule: no displacement


def test_analyze_radial_error_accumulates_the_histogram():
    from mavflow import _lib
    from mavflow.processor import Processor, SyntheticDataset
    from mavflow.run_config import RunConfig
    W, H = 97, 71
    x = T.hist_inputs("97x71")
    flow2, gt2, sky2 = T.scene(5151, W, H, 1, *T.DEFAULT_EDGES)
    dm, de = R.edge_distance(flow2, gt2, sky2)
    assert dm >= T.MIN_EDGE_DISTANCE_PX and de >= T.MIN_EDGE_DISTANCE_DEG

    class Fields(SyntheticDataset):
        def get_gt_of(self, i):
            return (x["gt"][0], gt2[0])[i]

        def get_sky_segmentation(self, i):
            return (x["sky"][0] != 0, sky2[0])[i]

    ds = Fields(W, H, 3, use_farneback=False)
    p = Processor(RunConfig(logging.getLogger("t"), ds, "", False, False, False, True, False, False, "FLOW_FOE_CLUSTERING"))
    try:
        assert p.radial_error is None
        with pytest.raises(ValueError):
            p.analyze_radial_error()                                       # no current frame's flow
        want = np.zeros(R.table_of(x["ref"]).shape, np.int64)
        with _lib.Context(W, H, 1) as ctx:
            for i, (flow, gt, sky) in enumerate(((x["flow"][0], x["gt"][0], x["sky"][0]), (flow2[0], gt2[0], sky2[0]))):
                p.frame_index, p.flow_uv = i, flow
                p.analyze_radial_error()
                want += R.table_of(ctx.radial_error_hist(flow, gt, sky))
                assert np.array_equal(R.table_of(p.radial_error.counts()), want), i
        assert p.radial_error.frames == 2
        assert np.array_equal(want, R.table_of(x["ref"]) + R.table_of(R.radial_hist(flow2, gt2, sky2)))
        # the attributes the reference's loop sets take precedence over the dataset's getters
        p.gt_flow_uv, p.sky_mask = x["gt"][0], np.ones((H, W), bool)
        p.analyze_radial_error()
        assert np.array_equal(R.table_of(p.radial_error.counts()), want)   # all sky: nothing added
    finally:
        p.release()
    assert p.radial_error is None
