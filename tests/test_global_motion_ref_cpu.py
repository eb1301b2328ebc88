"""The numpy restatement of the global-motion branch (tests/global_motion_ref.py) against what pins it, and the host-only parts of the
Detector / Processor shims.  No GPU.

Full-frame part: every array of tests/golden/global_motion.npz -- recorded from the reference's own flow_vec_subtract by
tools/gen_golden_global_motion.py -- bit for bit.

Fit: nothing of cv2 is available, so the DLT stage is held to two independent float64 solvers of the same system instead:
np.linalg.eigh of the same LtL and np.linalg.svd of L.  The two LAPACK routes bracket what rounding alone does to this problem, and
Jacobi is a third route, so the Jacobi result must lie within 100x the largest elementwise gap between the two (of the denormalised H
scaled to H[2, 2] == 1, over fit_cases()).  Measured: gap eigh vs svd = 2.5e-12, so the bound in force is 2.5e-10; Jacobi
vs eigh came out at 2.3e-12 at most, and exact pairs recover the known H to 6.4e-13 (the far-from-origin case) or better.  The bound is recomputed from the two LAPACK solvers on every run, never from Jacobi.
"""
import os

import numpy as np
import pytest

import global_motion_ref as R
from global_motion_cases import H_TRUE, degenerate_pairs, fit_cases, project as _project

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "global_motion.npz"))
CASES = [str(c) for c in G["cases"]]


# ---- the full-frame part against the reference's arrays ----------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_restatement_equals_the_reference_fixture(case):
    flow, M = G[f"{case}_flow"], G[f"{case}_M"]
    got = R.subtract(flow, M)
    for key, name in (("warped", "warped"), ("mag", "mag"), ("gray", "image")):
        exp = G[f"{case}_{name}"]
        assert got[key].dtype == exp.dtype and got[key].shape == exp.shape, (case, key)
        assert got[key].tobytes() == exp.tobytes(), (case, key)
    assert got["flow_max"] == tuple(int(v) for v in G[f"{case}_flow_max"]), case
    if f"{case}_coords" in G.files:
        cn = R.coords_new(G[f"{case}_coords"], flow)
        assert cn.dtype == np.float64 and cn.tobytes() == G[f"{case}_coords_new"].tobytes(), case


def test_fixture_covers_the_edge_cases():
    assert not G["z64_image"].any() and not G["z64_mag"].any()                    # 0 / 0 -> NaN -> 0
    assert (G["t64_image"] == 255).all() and tuple(G["t64_flow_max"]) == (0, 0)  # every pixel ties: the first wins
    assert G["tiny64_mag"].max() == 0 and np.abs(G["tiny64_warped"]).max() > 0    # squares underflow
    assert G["big97_mag"].max() > 1e3


# ---- the fit -----------------------------------------------------------------------------------------------------------------
def _finish(h0, norm):
    H = np.array(R.dlt_from_vector([float(v) for v in h0], norm))
    return H / H[2, 2]


def dlt_eigh(src, dst):
    LtL, norm = R.dlt_matrix(src, dst)
    w, V = np.linalg.eigh(np.array(LtL))
    return _finish(V[:, 0], norm)


def dlt_svd(src, dst):
    Lx, Ly, norm = R.dlt_rows(src, dst)
    L = np.concatenate([np.stack(Lx, axis=1), np.stack(Ly, axis=1)])
    return _finish(np.linalg.svd(L)[2][-1], norm)


@pytest.fixture(scope="module")
def dlt_bound():
    gap = max(float(np.abs(dlt_eigh(s, d) - dlt_svd(s, d)).max()) for _, s, d, _ in fit_cases())
    print(f"largest elementwise gap eigh vs svd: {gap:.3e}; bound {100 * gap:.3e}")
    assert gap > 0
    return 100.0 * gap


def test_dlt_agrees_with_two_lapack_solvers(dlt_bound):
    for name, src, dst, _ in fit_cases():
        H, ok = R.dlt(src, dst)
        assert ok == 1 and H[2, 2] == 1.0, name
        err = float(np.abs(H - dlt_eigh(src, dst)).max())
        print(f"{name}: Jacobi vs eigh {err:.3e}")
        assert err <= dlt_bound, (name, err, dlt_bound)


def test_lm_error_never_rises_and_exact_pairs_recover_H(dlt_bound):
    for name, src, dst, exact in fit_cases():
        hist = []
        H, ok = R.find_homography(src, dst, hist)
        assert ok == 1 and H[2, 2] == 1.0 and len(hist) >= 1, name
        assert all(b < a for a, b in zip(hist, hist[1:])), (name, hist)            # exact comparison: accepted steps only ever fall
        assert len(hist) <= R.LM_ITERATIONS + 1
        if exact:
            err = float(np.abs(H - H_TRUE).max())
            print(f"{name}: |H - H_true| {err:.3e}")
            assert err <= dlt_bound, (name, err)
        else:                                                                       # the refinement does not lose to the DLT it starts from
            d, _ = R.dlt(src, dst)
            e_dlt = float(np.sum((_project(d, src) - dst) ** 2))
            e_fit = float(np.sum((_project(H, src) - dst) ** 2))
            assert e_fit <= e_dlt * (1 + 1e-12), (name, e_fit, e_dlt)


def test_four_pairs_work():
    name, src, dst, _ = fit_cases()[0]
    H, ok = R.find_homography(src, dst)
    assert ok == 1 and np.abs(_project(H, src) - dst).max() < 1e-9


@pytest.mark.parametrize("kind", ["collinear", "repeated", "collinear_dst_axis"])
def test_degenerate_pairs_give_ok_0(kind):
    H, ok = R.find_homography(*degenerate_pairs(kind))
    assert ok == 0 and not H.any()


def test_jacobi_has_a_fixed_bound_on_bad_input():
    A = [[float("nan")] * 9 for _ in range(9)]
    w, V = R.jacobi_eigen(A, 9)                # returns at once: no finite off-diagonal sum
    assert len(w) == 9


# ---- host-only parts of the shims --------------------------------------------------------------------------------------------
class _DS:
    capture_size = (96, 80)
    ground_truth: list = []


def test_other_estimators_are_not_implemented(mav):
    from mavflow.detector import Detector
    flow = np.zeros((80, 96, 2), np.float32)
    for alg in (Detector.Algorithm.AFFINE, Detector.Algorithm.FUNDAMENTAL, Detector.Algorithm.ESSENTIAL):
        with pytest.raises(NotImplementedError, match="RANSAC"):
            Detector(_DS(), alg).get_transformation_matrix(None, flow)
    det = Detector(_DS(), Detector.Algorithm.FOE)
    assert det.get_transformation_matrix(None, flow) is None and det.use_optimization is False
    mag, ang = det.get_gradient_and_magnitude(np.array([[[3.0, 4.0], [0.0, -2.0]]]))
    assert mag.tolist() == [[5.0, 2.0]] and ang[0, 1] == -np.pi / 2


def _processor(**kw):
    from mavflow.processor import Processor, SyntheticDataset
    from mavflow.run_config import RunConfig
    import logging
    ds = SyntheticDataset(W=96, H=80, N=3, use_farneback=False)
    cfg = RunConfig(logging.getLogger("t"), ds, "", False, False, False, True, False, False, "FLOW_FOE_CLUSTERING")
    return Processor(cfg, **kw), ds


def test_processor_algorithm_keyword_and_dataset_additions(mav):
    from mavflow import utils
    from mavflow.detector import Detector
    np.random.seed(3)
    p0, ds = _processor()
    np.random.seed(3)
    p1, _ = _processor(algorithm=None)
    assert p0.detector.algorithm == p1.detector.algorithm == Detector.Algorithm.ESSENTIAL and not p0.detector.is_homography_based()
    assert np.array_equal(p0.detector.coords, p1.detector.coords)                  # same draws from the global RNG
    ph, _ = _processor(algorithm=Detector.Algorithm.HOMOGRAPHY)
    assert ph.detector.is_homography_based() and ph.detection_windows == {} and ph.detection_iou == {}
    for call in (ph.run_detection_batched, ph.run_detection_staged):
        with pytest.raises(NotImplementedError):
            call()
    ph.debug_mode = True
    with pytest.raises(NotImplementedError, match="debug"):
        ph.run_detection()
    gt = ds.ground_truth
    assert len(gt) == 1 and isinstance(gt[0], utils.Rectangle) and gt[0].get_topleft() == (24, 20) and gt[0].size == (24, 24)
    assert ds.get_annotation(0) is None
    seg = ds.get_segmentation(0)[..., 0]
    ys, xs = np.nonzero(seg)
    assert (xs.min(), ys.min(), xs.max() + 1, ys.max() + 1) == (24, 20, 48, 44)      # the rectangle is the patch's


def test_new_exports_are_declared(mav):
    from mavflow import _lib
    for name in ("mav_find_homography", "mav_find_homography_dev", "mav_flow_homography", "mav_flow_homography_dev", "mav_global_motion",
                 "mav_global_motion_dev", "mav_global_motion_step_dev", "mav_last_global_motion_render"):
        assert name in _lib.EXPORTS and hasattr(_lib.load(), name)
    for m in ("find_homography", "flow_homography", "global_motion", "global_motion_step", "render_last_global_motion"):
        assert callable(getattr(_lib.Context, m))
