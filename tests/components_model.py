"""A numpy model of the phases of csrc/kernels_components.hip -- tile-local roots, border unions, flatten, rank, slots -- with the
tile size taken from the one place the kernels' is held to (mavflow._lib, against include/mavflow.h in tests/test_abi_components.py).
The border unions are a LIST that can be applied in any order: tests/test_components_model_cpu.py shuffles it and expects the
restatement's outputs from every order, which is the scheduling-independence argument checked without a GPU."""
import numpy as np

import components_ref as R
from mavflow._lib import CC_TILE_H as T_H
from mavflow._lib import CC_TILE_W as T_W

NO_SLOT = -(1 << 31)


def tile_roots(mask, connectivity):
    """Phase 1: L[p] = image index of the first pixel (raster order) of p's component INSIDE its tile; -1 on background."""
    m = np.asarray(mask) != 0
    H, W = m.shape
    L = np.full(H * W, -1, np.int64)
    for y0 in range(0, H, T_H):
        for x0 in range(0, W, T_W):
            sub = m[y0:y0 + T_H, x0:x0 + T_W]
            lab, n = R.label(sub, connectivity)
            ys, xs = np.nonzero(lab)
            first = {}
            for y, x in zip(ys.tolist(), xs.tolist()):                  # np.nonzero walks in raster order
                first.setdefault(int(lab[y, x]), (y0 + y) * W + x0 + x)
            for y, x in zip(ys.tolist(), xs.tolist()):
                L[(y0 + y) * W + x0 + x] = first[int(lab[y, x])]
    return L


def border_unions(mask, connectivity, skip_redundant=True):
    """Phase 2's work list: (p, q) for every set pixel p on a tile's top row / left column and each set neighbour q across the border.
    skip_redundant: as the kernel, leave out a diagonal next to a set straight neighbour (it is joined through that neighbour)."""
    m = np.asarray(mask) != 0
    H, W = m.shape
    out = []

    def visit(x, y, dx, dy):
        if not m[y, x]:
            return
        straight = m[y + dy, x + dx]
        if straight:
            out.append((y * W + x, (y + dy) * W + x + dx))
        if connectivity != 8 or (straight and skip_redundant):
            return
        for s in (-1, 1):
            qx, qy = x + dx + (0 if dx else s), y + dy + (0 if dy else s)
            if 0 <= qx < W and 0 <= qy < H and m[qy, qx]:
                out.append((y * W + x, qy * W + qx))

    for y in range(T_H, H, T_H):
        for x in range(W):
            visit(x, y, 0, -1)
    for x in range(T_W, W, T_W):
        for y in range(H):
            visit(x, y, -1, 0)
    return out


def find(L, v):
    while L[v] != v:
        assert L[v] < v                       # the invariant the termination argument rests on
        v = L[v]
    return v


def union(L, a, b):
    """cc_union: every round ends the loop or lowers max(a, b); stores only lower a word."""
    a, b = find(L, a), find(L, b)
    rounds = 0
    while a != b:
        if a < b:
            a, b = b, a
        old = L[a]
        L[a] = min(old, b)                    # atomicMin
        rounds += 1
        if old == a:
            break
        a = old
    return rounds


def finish(L, W, min_area, max_blobs):
    """Phases 3 - 8 on a merged L: flatten, areas, rank, slots, statistics -> (labels (H*W), (n_components, n_blobs), table)."""
    n = L.size
    root = np.array([find(L, p) if L[p] >= 0 else -1 for p in range(n)], np.int64)
    area = np.bincount(root[root >= 0], minlength=n)
    is_root = root == np.arange(n)
    big = is_root & (area >= min_area)
    label_of = np.cumsum(is_root) * is_root                             # 1 + the roots before it, in raster order
    slot_of = np.where(big, np.cumsum(big) - 1, -1)
    labels = np.where(root >= 0, label_of[np.maximum(root, 0)], 0).astype(np.int32)
    table = np.zeros(max_blobs, R.BLOB_DTYPE)
    for p in np.nonzero(root >= 0)[0].tolist():
        s = slot_of[root[p]]
        if s < 0 or s >= max_blobs:
            continue
        x, y = p % W, p // W
        t = table[s]
        if t["area"] == 0:
            table[s] = (label_of[root[p]], x, y, x, y, area[root[p]], 0, 0)
            t = table[s]
        t["x"], t["w"], t["h"] = min(t["x"], x), max(t["w"], x), max(t["h"], y)
        t["sum_x"] += x
        t["sum_y"] += y
    used = table["area"] > 0
    table["w"][used] = table["w"][used] - table["x"][used] + 1
    table["h"][used] = table["h"][used] - table["y"][used] + 1
    return labels, (int(is_root.sum()), int(big.sum())), table


def run(mask, connectivity=8, min_area=1, max_blobs=256, order=None, skip_redundant=True):
    """The whole plan on one mask; order: a numpy Generator that shuffles the border unions, or None for the kernel's thread order."""
    H, W = np.asarray(mask).shape
    L = tile_roots(mask, connectivity)
    todo = border_unions(mask, connectivity, skip_redundant)
    if order is not None:
        todo = [todo[i] for i in order.permutation(len(todo))]
    for a, b in todo:
        union(L, a, b)
    labels, counts, table = finish(L, W, min_area, max_blobs)
    return labels.reshape(H, W), counts, table
