"""The contract of mav_components (include/mavflow.h) restated on the host: a plain raster-scan union-find, no device plan in it.

    labels   int32 (H, W): 0 on background, components numbered 1 .. n in raster order of their first pixel
    counts   (n_components, n_blobs): n_blobs = components with area >= min_area (may exceed max_blobs)
    table    max_blobs records {label, x, y, w, h, area, sum_x, sum_y}: the first min(n_blobs, max_blobs) components with
             area >= min_area in label order, all-zero records behind them

tests/test_components_ref_cpu.py holds it to scipy.ndimage.label; the GPU tests hold the library to it, bit for bit."""
import numpy as np

BLOB_DTYPE = np.dtype([("label", np.int32), ("x", np.int32), ("y", np.int32), ("w", np.int32), ("h", np.int32), ("area", np.int32),
                       ("sum_x", np.int64), ("sum_y", np.int64)])
COUNTS_DTYPE = np.dtype([("n_components", np.int32), ("n_blobs", np.int32)])


def check_params(connectivity, min_area, max_blobs):
    if connectivity not in (4, 8) or min_area < 1 or not 1 <= max_blobs <= 65535:
        raise ValueError((connectivity, min_area, max_blobs))


def label(mask, connectivity=8):
    """(labels, n_components) of one (H, W) mask; any non-zero entry is set."""
    m = np.asarray(mask) != 0
    H, W = m.shape
    parent = list(range(H * W))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    back = [(-1, 0), (0, -1)] + ([(-1, -1), (-1, 1)] if connectivity == 8 else [])
    rows = m.tolist()
    for y in range(H):
        for x in range(W):
            if not rows[y][x]:
                continue
            for dy, dx in back:
                yy, xx = y + dy, x + dx
                if 0 <= yy and 0 <= xx < W and rows[yy][xx]:
                    a, b = find(y * W + x), find(yy * W + xx)
                    if a != b:
                        parent[max(a, b)] = min(a, b)          # the smaller index stays root: the component's first pixel
    labels = np.zeros((H, W), np.int32)
    number = {}
    for y in range(H):
        for x in range(W):
            if rows[y][x]:
                r = find(y * W + x)
                if r not in number:
                    number[r] = len(number) + 1                # first met in raster order = raster order of the first pixels
                labels[y, x] = number[r]
    return labels, len(number)


def table_of(labels, n, min_area=1, max_blobs=256):
    """((n_components, n_blobs), table) from a label image numbered 1 .. n."""
    tab = np.zeros(max_blobs, BLOB_DTYPE)
    ys, xs = np.nonzero(labels)
    lab = labels[ys, xs]
    n_blobs = 0
    for k in range(1, n + 1):
        sel = lab == k
        area = int(sel.sum())
        if area < min_area:
            continue
        if n_blobs < max_blobs:
            x, y = xs[sel], ys[sel]
            tab[n_blobs] = (k, x.min(), y.min(), x.max() - x.min() + 1, y.max() - y.min() + 1, area, int(x.sum(dtype=np.int64)),
                            int(y.sum(dtype=np.int64)))
        n_blobs += 1
    return (n, n_blobs), tab


def components(mask, connectivity=8, min_area=1, max_blobs=256):
    """One (H, W) mask -> (labels, (n_components, n_blobs), table)."""
    check_params(connectivity, min_area, max_blobs)
    labels, n = label(mask, connectivity)
    counts, tab = table_of(labels, n, min_area, max_blobs)
    return labels, counts, tab


def components_batch(masks, connectivity=8, min_area=1, max_blobs=256):
    """(B, H, W) masks -> labels (B, H, W) int32, counts (B) COUNTS_DTYPE, tables (B, max_blobs) BLOB_DTYPE."""
    masks = np.asarray(masks)
    B = masks.shape[0]
    labels = np.zeros(masks.shape, np.int32)
    counts = np.zeros(B, COUNTS_DTYPE)
    tables = np.zeros((B, max_blobs), BLOB_DTYPE)
    for b in range(B):
        labels[b], c, tables[b] = components(masks[b], connectivity, min_area, max_blobs)
        counts[b] = c
    return labels, counts, tables


def hull(table):
    """x0, y0, x1, y1 (inclusive) of all records of a trimmed table, or four -1 for none: get_simple_bounding_box's corners."""
    t = table[table["area"] > 0]
    if len(t) == 0:
        return (-1, -1, -1, -1)
    return (int(t["x"].min()), int(t["y"].min()), int((t["x"] + t["w"]).max() - 1), int((t["y"] + t["h"]).max() - 1))
