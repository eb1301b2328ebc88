"""TEST INFRASTRUCTURE -- the k-means of include/mavflow_cluster.h restated in numpy: cv2.kmeans' loop structure (as remembered from
OpenCV 4.x modules/core/src/kmeans.cpp; not pinned, there is no cv2 here) with the caller's initial centres, and the arithmetic
Detector.clustering does after the cv2 call (src/detector.py:414-427).

Distances are float32, one rounded operation at a time (numpy never fuses); the cluster sums are float64.  The header fixes the ORDER of
the device's float64 sums; this restatement does not mimic it (np.sum's order is its own): the two agree to the bit wherever the sums are
exact in any order -- samples that are multiples of 2^-8 below 2^12 with N <= 2^20 (cluster_cases.exact_condition), uint8 samples
always -- and the compactness, a sum of float32 distances that are not grid values, to rounding (1e-12 relative)."""
import numpy as np

MAX_K, MAX_ATTEMPTS, MAX_DIMS, CHUNK = 16, 16, 4, 4096
RECORD_DTYPE = np.dtype([("compactness", np.float64), ("shift", np.float64), ("best_attempt", np.int32), ("iterations", np.int32),
                         ("repairs", np.int32), ("skipped", np.int32), ("counts", np.int32, (16,))])


def dist(x: np.ndarray, c: np.ndarray) -> np.ndarray:
    """float32 squared distances of the rows of x (n, D) to c (D,) or, row by row, to c (n, D): the sum over d ascending, from 0"""
    x, c = np.asarray(x, np.float32), np.asarray(c, np.float32)
    s = np.zeros(x.shape[0], np.float32)
    for d in range(x.shape[1]):
        t = x[:, d] - c[..., d]
        s = s + t * t
    return s


def clamp_iter(max_iter: int) -> int:
    return min(max(int(max_iter), 2), 100)


def eps_squared(eps: float) -> float:
    return float(eps) * float(eps) if eps > 0 else 0.0


def assign(x: np.ndarray, c: np.ndarray):
    """(labels, the (n, K) float32 distances): the FIRST k of the smallest distance"""
    dm = np.stack([dist(x, c[k]) for k in range(c.shape[0])], axis=1)
    return np.argmin(dm, axis=1).astype(np.int64), dm


def attempt(samples: np.ndarray, init: np.ndarray, max_iter: int = 10, eps: float = 1.0) -> dict:
    """One attempt from the centres init (K, D).  Besides the results, `trace`: per assignment a dict of the centres it used, its labels
    (after repairs), n, the repairs it made as (k, donor, j, dist, tied) and how many samples had two nearest centres."""
    x = np.ascontiguousarray(samples).astype(np.float32)
    xd = x.astype(np.float64)
    N, D = x.shape
    c = np.array(init, np.float32).reshape(-1, D)
    K = c.shape[0]
    assert N >= K
    max_iter, eps2 = clamp_iter(max_iter), eps_squared(eps)
    trace, repairs, shift = [], 0, 0.0
    for it in range(1, max_iter):
        labels, dm = assign(x, c)
        ties = int(np.sum(np.sum(dm == dm.min(axis=1, keepdims=True), axis=1) > 1))
        n = np.bincount(labels, minlength=K).astype(np.int64)
        S = np.zeros((K, D), np.float64)
        for k in range(K):
            S[k] = xd[labels == k].sum(axis=0)
        moved = []
        for k in range(K):
            if n[k] != 0:
                continue
            donor = int(np.argmax(n))                                   # the first of the largest
            m = (S[donor] / np.float64(n[donor])).astype(np.float32)
            idx = np.nonzero(labels == donor)[0]
            dd = dist(x[idx], m)
            far = dd.max()
            j = int(idx[np.nonzero(dd == far)[0][-1]])                  # the highest index among equals
            moved.append((k, donor, j, float(far), int(np.sum(dd == far))))
            labels[j] = k
            n[donor] -= 1
            n[k] += 1
            S[donor] = S[donor] - xd[j]
            S[k] = S[k] + xd[j]
        repairs += len(moved)
        new = (S / n[:, None].astype(np.float64)).astype(np.float32)
        t = (new - c).astype(np.float64)                                # the float32 difference, widened
        per_k = np.zeros(K, np.float64)
        for d in range(D):
            per_k = per_k + t[:, d] * t[:, d]
        shift = float(per_k.max())
        trace.append(dict(centers=c.copy(), labels=labels.copy(), n=n.copy(), repairs=moved, ties=ties))
        c = new
        if it == max_iter - 1 or shift <= eps2:
            break
    compactness = float(np.sum(dist(x, c[labels]).astype(np.float64)))
    return dict(labels=labels.astype(np.int32), centers=c, compactness=compactness, iterations=len(trace), repairs=repairs, counts=n.astype(np.int32),
                shift=shift, trace=trace)


def kmeans(samples: np.ndarray, init: np.ndarray, max_iter: int = 10, eps: float = 1.0) -> dict:
    """samples (N, D) float32 or uint8, init (A, K, D): the attempt with the first strictly smallest compactness.  `attempts` holds every
    attempt's own dict."""
    init = np.asarray(init, np.float32)
    runs = [attempt(samples, init[a], max_iter, eps) for a in range(init.shape[0])]
    best = 0
    for a in range(1, len(runs)):
        if runs[a]["compactness"] < runs[best]["compactness"]:
            best = a
    r = runs[best]
    counts = np.zeros(16, np.int32)
    counts[:len(r["counts"])] = r["counts"]
    return dict(labels=r["labels"], centers=r["centers"], compactness=r["compactness"], best_attempt=best, iterations=r["iterations"],
                repairs=int(sum(q["repairs"] for q in runs)), counts=counts, shift=r["shift"], attempts=runs)


def lut(centers: np.ndarray) -> np.ndarray:
    """Detector.clustering's table (src/detector.py:414-418): uint8(center * 255 / max), max 1.0 when 0, in float32"""
    c = np.asarray(centers, np.float32)
    mx = np.max(c)
    if mx == 0.0:
        mx = np.float32(1.0)
    with np.errstate(invalid="ignore"):
        return np.uint8(c * np.float32(255) / mx)


def paint(labels: np.ndarray, centers: np.ndarray):
    """mav_kmeans_paint: (res (N, D) uint8, mask (N,) uint8 = res[:, 0] >= 225)"""
    res = lut(centers)[np.asarray(labels).reshape(-1)]
    return res, (res[:, 0] >= 225).astype(np.uint8)


def paint_image(labels: np.ndarray, centers: np.ndarray, shape, enable_raw: bool = False):
    """What Detector.clustering returns (src/detector.py:419-428) for an image of `shape` whose consecutive triples were the samples:
    (res, zeros(0)) with enable_raw, else (rgb, mask): res repeated to three channels with channel 1 cleared where res >= 225."""
    res = paint(labels, centers)[0].reshape(shape)
    if enable_raw:
        return res, np.zeros(0)
    rgb = np.repeat(res[..., None], 3, axis=-1)
    mask = rgb[..., 0] >= 225
    rgb[mask, 1] = 0
    return rgb, mask
