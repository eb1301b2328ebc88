"""numpy restatements of the two passes of include/mavflow_truth.h, in the reference's own operation order: the ground-truth flow
(src/airsim_optical_flow.py:12-107 with write_flow's `-result.swapaxes(0, 1)`, :142) and the radial-error histogram
(src/processor.py:267-275 with src/plot_radial_error.py:38-39).  tests/test_truth_ref_cpu.py holds them bit for bit to arrays the
reference's functions produced (tests/golden/truth.npz); the GPU tests hold the library to them."""
import numpy as np

DEFAULT_MAG_EDGES = np.linspace(0, 10, 160)          # plot_radial_error.py:38
DEFAULT_ERR_EDGES = np.linspace(-20, 20, 160)


def _row(M, i, a, b, c, d):
    """mat4x4_vec4_mult's row i: four products added left to right"""
    return ((M[i, 0] * a + M[i, 1] * b) + M[i, 2] * c) + M[i, 3] * d


def gt_flow(depth, seg, view_proj_prev, view_proj_inv, displacement, depth_scale=1.0) -> np.ndarray:
    """depth (H, W) float32, seg (H, W) uint8 or None -> (H, W, 2) float64 (u, v): the array write_flow hands to utils.write_flow.
    view_proj_inv: numpy.linalg.inv of the second state's matrix, from the caller."""
    depth = np.asarray(depth)
    assert depth.dtype == np.float32 and depth.ndim == 2
    H, W = depth.shape
    Mp, Mi = np.asarray(view_proj_prev, np.float64).reshape(4, 4), np.asarray(view_proj_inv, np.float64).reshape(4, 4)
    x = np.broadcast_to(np.arange(W, dtype=np.float64)[None, :], (H, W))
    y = np.broadcast_to(np.arange(H, dtype=np.float64)[:, None], (H, W))
    with np.errstate(all="ignore"):
        nx, ny = x / np.float64(W), y / np.float64(H)
        sx, sy = 2.0 * (nx - 0.5), 2.0 * ((1.0 - ny) - 0.5)
        s = [_row(Mi, i, sx, sy, 1.0, 1.0) for i in range(4)]
        e = [_row(Mi, i, sx, sy, 0.5, 1.0) for i in range(4)]
        S = [s[i] / s[3] for i in range(3)]
        E = [e[i] / e[3] for i in range(3)]
        d = [E[i] - S[i] for i in range(3)]
        n = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        z = (depth * np.float32(depth_scale)).astype(np.float64)             # the product in float32
        P = [S[i] + (d[i] / n) * z for i in range(3)]
        if seg is not None:
            mav = np.asarray(seg) > 0
            P = [np.where(mav, P[i] - np.float64(displacement[i]), P[i]) for i in range(3)]
        p = [_row(Mp, i, P[0], P[1], P[2], 1.0) for i in (0, 1, 3)]
        rhw = 1.0 / p[2]
        px, py = p[0] * rhw, p[1] * rhw
        rx = (px * 0.5 + 0.5) * np.float64(W) - x
        ry = ((-py) * 0.5 + 0.5) * np.float64(H) - y
        return np.stack((-rx, -ry), -1)


def gt_flow_f32(*a, **kw) -> np.ndarray:
    """what the .flo file holds: the float64 field rounded"""
    with np.errstate(all="ignore"):
        return gt_flow(*a, **kw).astype(np.float32)


def same_bits(a, b) -> bool:
    """equal bytes where neither is NaN, NaN in the same places (the sign and payload of a NaN are nobody's contract)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(u)[~na], b.view(u)[~nb]))


def radial_values(flow, gt_flow_, sky):
    """analyze_radial_error's two arrays (what it hands to numpy.save): float32 magnitudes and angular errors of the non-sky pixels"""
    flow, g = np.asarray(flow, np.float32), np.asarray(gt_flow_, np.float32)
    with np.errstate(all="ignore"):
        mag = np.sqrt(flow[..., 0] * flow[..., 0] + flow[..., 1] * flow[..., 1])
        err = np.rad2deg(np.arctan2(flow[..., 1], flow[..., 0]) - np.arctan2(g[..., 1], g[..., 0]))
    keep = np.ones(mag.shape, bool) if sky is None else ~(np.asarray(sky) != 0)
    return mag[keep].flatten(), err[keep].flatten()


def bin_index(v, edges):
    """numpy.histogram2d's rule per axis: k with edges[k] <= v < edges[k+1], the last bin closed on the right -> (k, inside)"""
    v, edges = np.asarray(v, np.float64), np.asarray(edges, np.float64)
    k = np.searchsorted(edges, v, side="right") - 1
    k = np.where(v == edges[-1], len(edges) - 2, k)
    with np.errstate(invalid="ignore"):
        ok = (v >= edges[0]) & (v <= edges[-1])
    return k, ok


def radial_hist(flow, gt_flow_, sky, mag_edges=DEFAULT_MAG_EDGES, err_edges=DEFAULT_ERR_EDGES) -> dict:
    """fields of any leading shape (..., H, W, 2) -> counts (Nm, Ne) int64, non_sky, in_range"""
    mag, err = radial_values(flow, gt_flow_, sky)
    i, oi = bin_index(mag, mag_edges)
    j, oj = bin_index(err, err_edges)
    ok = oi & oj
    counts = np.zeros((len(mag_edges) - 1, len(err_edges) - 1), np.int64)
    np.add.at(counts, (i[ok], j[ok]), 1)
    return dict(counts=counts, non_sky=int(mag.size), in_range=int(ok.sum()))


def table_of(h: dict) -> np.ndarray:
    """the library's table: non_sky, in_range, counts row-major"""
    return np.concatenate(([h["non_sky"], h["in_range"]], h["counts"].reshape(-1))).astype(np.int64)


def edge_distance(flow, gt_flow_, sky, mag_edges=DEFAULT_MAG_EDGES, err_edges=DEFAULT_ERR_EDGES):
    """the smallest distance of any non-sky pixel's (magnitude, error) to an edge of its list -> (px, degrees)"""
    mag, err = radial_values(flow, gt_flow_, sky)

    def nearest(v, e):
        v, e = v.astype(np.float64), np.asarray(e, np.float64)
        k = np.searchsorted(e, v)
        return np.minimum(np.abs(v - e[np.clip(k - 1, 0, len(e) - 1)]), np.abs(v - e[np.clip(k, 0, len(e) - 1)])).min()

    return float(nearest(mag, mag_edges)), float(nearest(err, err_edges))
