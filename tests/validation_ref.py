"""TEST INFRASTRUCTURE -- a numpy restatement of the validation tail of the reference's loop, written from src/processor.py:343-347
(drone pixels, drone_flow_avg_gt, drone_size_pixels), src/im_helpers.py:55-84,244-252 (get_simple_bounding_box, calculate_tpr_fpr),
src/datasets/dataset.py:173-175 (validate_sky_segment) and src/detector.py:70-117 (derotate), in the form of the records and index
lists include/mavflow_validation.h describes.  tests/golden/validation.npz (tools/gen_golden_validation.py) holds what the reference's
own functions give for the same inputs; tests/test_validation_ref_cpu.py holds this file to it bit for bit, and the GPU tests hold the
device to this file byte for byte.  It imports nothing of the package."""
import numpy as np

FRAME0, THR_F64 = 1, 2                  # MAV_GT_STATS_FRAME0 / MAV_GT_STATS_THR_F64
TRUNCATED, DEPTH_NAN = 1, 2             # MAV_GT_STATS_TRUNCATED / MAV_GT_STATS_DEPTH_NAN
RECORD_DTYPE = np.dtype([("drone_pixels", np.int64), ("sky", np.int64, (4,)), ("flow_sum", np.float64, (2,)), ("box", np.int32, (4,)),
                         ("seg_max", np.int32), ("listed", np.int32), ("depth_max", np.float32), ("flags", np.uint32), ("pad", np.uint32, (2,))])
assert RECORD_DTYPE.itemsize == 96


def fraction_as_given(f) -> np.float64:
    """The double nearest to the shortest decimal n / 10^d (d = 1 .. 9) that rounds to the float32 f (0.8 for float32(0.8)): what the
    Python float in the reference's `0.80 * np.max(depth)` was before a float32 field carried it; float64(f) if there is none."""
    f = np.float32(f)
    v, p = np.float64(f), np.float64(1.0)
    for _ in range(9):
        p = p * np.float64(10.0)
        q = np.rint(v * p) / p
        if np.float32(q) == f:
            return q
    return v


def depth_threshold(depth_max, depth_fraction=0.8, legacy=False) -> np.float32:
    """`0.80 * np.max(depth_buffer)` as the float32 scalar the float32 depth is compared with.
    numpy >= 2: a Python float takes the float32 of np.max's result -- one float32 product.
    numpy 1.x (legacy): float64(0.80) * float32 is a float64 scalar; compared with a float32 ARRAY, value-based casting rounds it to float32."""
    m = np.float32(depth_max)
    with np.errstate(all="ignore"):
        if legacy:
            return np.float32(fraction_as_given(depth_fraction) * np.float64(m))
        return np.float32(depth_fraction) * m


def depth_max(depth) -> np.float32:
    """np.max: NaN as soon as one value is NaN (stored as the canonical quiet NaN)"""
    return np.float32(np.nan) if np.isnan(depth).any() else np.float32(np.max(depth))


def sky_counts(sky, depth, depth_fraction=0.8, legacy=False):
    """(pos, neg, tp, fp) of calculate_tpr_fpr((depth > thr) * 255, sky): the four sums of src/im_helpers.py:245-248 on the reference's
    int64 images, literally"""
    with np.errstate(all="ignore"):
        sky_mask_gt = depth > depth_threshold(depth_max(depth), depth_fraction, legacy)
    gt_img = sky_mask_gt * 255
    img = np.zeros(depth.shape, bool) if sky is None else np.asarray(sky) != 0
    return (int(np.sum(gt_img > 127)), int(np.sum((255 - gt_img) > 127)), int(np.sum((gt_img * img) > 127)), int(np.sum(((255 - gt_img) * img) > 127)))


def simple_box(seg, box_fraction=0.1):
    """(start_x, start_y, end_x, end_y) of get_simple_bounding_box (src/im_helpers.py:64-84), -1 where no pixel passes"""
    mask = seg > np.float64(box_fraction) * np.max(seg)
    ys, xs = np.nonzero(mask.any(axis=1))[0], np.nonzero(mask.any(axis=0))[0]
    if ys.size == 0:
        return (-1, -1, -1, -1)
    return (int(xs[0]), int(ys[0]), int(xs[-1]), int(ys[-1]))


def derotated_at(values, rows, cols, W, H, omega, dt):
    """Detector.derotate (src/detector.py:83-117) at the pixels (rows[k], cols[k]) whose float32 flow vectors are values[k]: float64"""
    o = np.asarray(omega, np.float64)
    x = -(np.asarray(cols) / W - 0.5) * 2.0
    y = -(np.asarray(rows) / H - 0.5) * 2.0
    d0 = +o[0] * x * y - o[1] * x ** 2 - o[1] + o[2] * y
    d1 = -o[2] * x + o[0] + o[0] * y ** 2 - o[1] * x * y
    d0 = d0 * (W * dt / 2)
    d1 = d1 * (H * dt / 2)
    return values - np.stack([d0, d1], axis=-1)


def sequential_sum(a):
    """the sum of the rows of a (n, 2) array accumulated row by row from 0 in a's own type: what np.average(a, axis=0) divides by n"""
    s = np.zeros(2, a.dtype)
    with np.errstate(all="ignore"):
        for row in a:
            s = s + row
    return s


def gt_stats(seg, gt_flow=None, sky=None, depth=None, omega=(0.0, 0.0, 0.0), dt=1.0, flags=0, max_pixels=16384, box_fraction=0.1,
             depth_fraction=0.8, seg_threshold=127):
    """One image: (record: a RECORD_DTYPE scalar array of shape (), indices: (max_pixels,) int32 with -1 behind the list)."""
    H, W = seg.shape
    r = np.zeros((), RECORD_DTYPE)
    rows, cols = np.nonzero(seg > seg_threshold)                   # raster order: the order of flow[segmentation > 127]
    n = rows.size
    listed = min(n, max_pixels)
    idx = np.full(max_pixels, -1, np.int32)
    idx[:listed] = (rows * W + cols)[:listed]
    r["drone_pixels"], r["listed"], r["seg_max"] = n, listed, int(np.max(seg))
    r["box"] = simple_box(seg, box_fraction)
    fl = 0
    if n > max_pixels:
        fl |= TRUNCATED
    if depth is not None:
        r["sky"] = sky_counts(sky, depth, depth_fraction, bool(flags & THR_F64))
        r["depth_max"] = depth_max(depth)
        if np.isnan(depth).any():
            fl |= DEPTH_NAN
    if gt_flow is not None and n <= max_pixels and n > 0:
        vals = gt_flow[rows, cols]
        if flags & FRAME0:
            r["flow_sum"] = sequential_sum(vals).astype(np.float64)                 # float32 rows, float32 sum (detector.py:80-81)
        else:
            r["flow_sum"] = sequential_sum(derotated_at(vals, rows, cols, W, H, omega, dt))
    r["flags"] = fl
    return r, idx


def gt_stats_batch(seg, gt_flow=None, sky=None, depth=None, omega=None, dt=None, flags=None, max_pixels=16384, **kw):
    """(records (B,), indices (B, max_pixels)) of (B, H, W) inputs; omega (B, 3), dt (B,), flags (B,) or None"""
    B = seg.shape[0]
    recs, idxs = np.zeros(B, RECORD_DTYPE), np.empty((B, max_pixels), np.int32)
    for b in range(B):
        recs[b], idxs[b] = gt_stats(seg[b], None if gt_flow is None else gt_flow[b], None if sky is None else sky[b], None if depth is None else depth[b],
                                    (0.0, 0.0, 0.0) if omega is None else omega[b], 1.0 if dt is None else dt[b], 0 if flags is None else int(flags[b]),
                                    max_pixels, **kw)
    return recs, idxs


def drone_flow_avg(record):
    """np.average(gt_flow_uv_derotated[segmentation > 127], axis=0) from a record: float64, NaN for an empty MAV"""
    with np.errstate(all="ignore"):
        return record["flow_sum"] / np.float64(record["drone_pixels"])


def drone_flow_avg_frame0(record):
    """... at frame index 0, where the reference averages the float32 rows: float32"""
    with np.errstate(all="ignore"):
        return record["flow_sum"].astype(np.float32) / np.float32(record["drone_pixels"])
