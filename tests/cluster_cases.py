"""TEST INFRASTRUCTURE -- the smallest inputs at which each piece of mav_kmeans (csrc/kernels_cluster.hip) can go wrong, with what
tests/kmeans_ref.py gives for them.  tests/test_gpu_kmeans.py runs every case through mav_kmeans and mav_kmeans_dev and demands the
restatement's labels, centres, counts, iterations, repairs and best attempt; tests/test_cluster_cases_cpu.py holds this table to its own
promises without a GPU: every case still reaches the instantiation or control path it is named after (the `reaches` sets are computed
from the inputs and the restatement's trace, not declared), and every float32 case meets the condition under which the float64 sums are
exact in any order."""
import functools
import os
import re
import zlib
from dataclasses import dataclass

import numpy as np

import kmeans_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mavflow_cluster.h")
INTERNAL = os.path.join(ROOT, "mav-detection_amd", "csrc", "mavflow_internal.h")
KERNELS = os.path.join(ROOT, "mav-detection_amd", "csrc", "kernels_cluster.hip")
CHUNK = 4096                                  # MAV_KMEANS_CHUNK: samples per workgroup step and per slab entry
GRID = 2.0 ** -8                              # float32 cases: every sample is a multiple of this ...
LIMIT = 2.0 ** 12                             # ... below this, with N <= 2^20: every float64 sum of samples is exact in any order


def source_constants() -> dict:
    out = {k: int(v) for k, v in re.findall(r"#define\s+(MAV_KMEANS_[A-Z_]+)\s+(\d+)\s", open(HEADER).read())}
    out.update({k: int(v) for k, v in re.findall(r"#define\s+(KM_[A-Z_]+)\s+(\d+)u?", open(INTERNAL).read())})
    return out


@dataclass(frozen=True)
class Case:
    name: str
    N: int
    D: int = 3
    u8: bool = False
    K: int = 8
    A: int = 10
    max_iter: int = 10
    eps: float = 1.0
    B: int = 1
    recipe: str = "blobs"
    wants: tuple = ()                   # what the case is there for: must be in reaches()

    @property
    def dtype(self):
        return np.uint8 if self.u8 else np.float32


def _seed(text: str) -> int:
    return zlib.crc32(text.encode()) & 0x7FFFFFFF


def _on_grid(v: np.ndarray) -> np.ndarray:
    return (np.clip(np.round(np.asarray(v, np.float64) / GRID) * GRID, 0.0, LIMIT - GRID)).astype(np.float32)


def _blobs(rng, N, D, nb, lo, hi, sigma):
    centres = rng.uniform(lo, hi, (nb, D))
    which = rng.integers(0, nb, N)
    which[:min(nb, N)] = np.arange(min(nb, N))
    return centres[which] + rng.normal(0, sigma, (N, D))


def _samples(c: Case, rng, b: int) -> np.ndarray:
    N, D, r = c.N, c.D, c.recipe
    if r in ("blobs", "far", "twin"):
        v = _blobs(rng, N, D, max(c.K, 2) + b, 20.0, 235.0, 6.0) if c.u8 else _blobs(rng, N, D, max(c.K, 2) + b, 100.0, 3000.0, 40.0)
    elif r == "identical":
        v = np.full((N, D), 7.5 if not c.u8 else 9.0) + np.arange(D)
    elif r == "equidistant":                   # few even values, many copies of each; the centres start on the odd numbers between them
        v = 2.0 * rng.integers(0, c.K + 1, (N, D))
        v[:c.K + 1] = 2.0 * np.arange(c.K + 1)[:, None]
    elif r == "frame":                         # a residual-magnitude-like image: a dim textured ground and one bright patch; rows of D values are the samples
        v = np.abs(rng.normal(0, 2.0, N * D)) + 3.0 * np.sin(np.arange(N * D) / 97.0) ** 2
        v[N * D // 3:N * D // 3 + 40 * D] += 60.0 if not c.u8 else 200.0
        v = v.reshape(N, D)
    else:
        raise KeyError(r)
    return np.clip(np.round(v), 0, 255).astype(np.uint8) if c.u8 else _on_grid(v)


def _init(c: Case, rng, x: np.ndarray) -> np.ndarray:
    xf = x.astype(np.float64)
    lo, hi = xf.min(axis=0), xf.max(axis=0)
    r = c.recipe
    if r == "far":                             # every centre beyond the data, centre 0 the nearest: K - 1 clusters start empty
        init = hi + 500.0 + 10.0 * np.arange(c.K)[None, :, None] + rng.uniform(0, 3, (c.A, c.K, c.D))
    elif r == "equidistant":
        init = np.broadcast_to((2.0 * np.arange(c.K) + 1.0)[None, :, None], (c.A, c.K, c.D)).copy()
        init[1:] += rng.integers(-1, 2, (c.A - 1, c.K, c.D))
    else:
        init = rng.uniform(lo - 1.0, hi + 1.0, (c.A, c.K, c.D))
    init = (np.round(init / GRID) * GRID).astype(np.float32)
    if r == "twin":
        init[1] = init[0]
    return init


@functools.lru_cache(maxsize=None)
def inputs(name: str) -> dict:
    """samples (B, N, D), init (B, A, K, D) float32 and `ref`: the restatement's result per image.  Read-only."""
    c = CASES[name]
    rng = np.random.default_rng(_seed(f"{c.recipe} {c.N} {c.D} {c.u8} {c.K} {c.A} {c.B}"))
    xs = np.stack([_samples(c, rng, b) for b in range(c.B)])
    init = np.stack([_init(c, rng, xs[b]) for b in range(c.B)])
    ref = [R.kmeans(xs[b], init[b], c.max_iter, c.eps) for b in range(c.B)]
    for a in (xs, init):
        a.setflags(write=False)
    return dict(samples=xs, init=init, ref=ref)


def exact_condition(x: np.ndarray) -> bool:
    """every float64 sum of these samples is exact in any order: multiples of 2^-8 below 2^12, at most 2^20 of them (53 > 12 + 8 + 20)"""
    v = np.asarray(x, np.float64)
    return bool(np.all(v / GRID == np.round(v / GRID)) and np.all(np.abs(v) < LIMIT) and x.shape[-2] <= 1 << 20)


def reaches(name: str) -> set:
    """the instantiation, the shapes and the control paths the case runs through, from its inputs and the restatement's trace"""
    c = CASES[name]
    got = {f"D{c.D} {'u8' if c.u8 else 'f32'}", f"K={c.K}", f"A={c.A}"}
    if c.N == c.K:
        got.add("N=K")
    if c.N == c.K + 1:
        got.add("N=K+1")
    for tag, n in (("one below a chunk", CHUNK - 1), ("one chunk", CHUNK), ("one above a chunk", CHUNK + 1)):
        if c.N == n:
            got.add(tag)
    if c.N > 2 * CHUNK and c.N % CHUNK and c.N % 256:
        got.add("chunks and a ragged tail")
    if c.max_iter == 2:
        got.add("max_iter 2")
    if c.eps == 0:
        got.add("eps 0")
    eps2 = R.eps_squared(c.eps)
    ins = inputs(name)
    if c.B == 3 and not np.array_equal(ins["samples"][0], ins["samples"][1]) and not np.array_equal(ins["samples"][1], ins["samples"][2]):
        got.add("batch 3")
    for ref in ins["ref"]:
        runs = ref["attempts"]
        early = [q for q in runs if q["iterations"] < R.clamp_iter(c.max_iter) - 1]
        ran_out = [q for q in runs if q["iterations"] == R.clamp_iter(c.max_iter) - 1 and q["shift"] > eps2]
        if ran_out:
            got.add("runs into max_iter")
        if ran_out and len({q["iterations"] for q in early}) >= 2:
            got.add("attempts stop at different iterations")
        comp = [q["compactness"] for q in runs]
        if comp.count(min(comp)) > 1:
            got.add("compactness tie")
        if ref["best_attempt"] > 0:
            got.add("a later attempt wins")
        for q in runs:
            for step in q["trace"]:
                if step["ties"]:
                    got.add("two nearest centres")
                if step["repairs"]:
                    got.add("repair")
                if c.K > 1 and len(step["repairs"]) == c.K - 1:
                    got.add("K-1 repairs in one update")
                for (_, _, _, far, tied) in step["repairs"]:
                    if far == 0.0:
                        got.add("repair at distance 0")
                    if tied > 1:
                        got.add("highest index among equals")
    return got


_C = Case
CASES = {c.name: c for c in (
    # every (D, element type) instantiation, at shapes the other rows need anyway
    _C("d1_f32", 1500, D=1, K=5, A=4, wants=("D1 f32",)),
    _C("d2_f32", CHUNK - 1, D=2, A=3, wants=("D2 f32", "one below a chunk")),
    _C("d3_f32", 3 * CHUNK + 517, D=3, max_iter=6, wants=("D3 f32", "chunks and a ragged tail", "K=8", "A=10", "runs into max_iter")),
    _C("d4_f32", CHUNK, D=4, K=16, A=3, wants=("D4 f32", "one chunk", "K=16")),
    _C("d1_u8", 131 * 67, D=1, u8=True, A=4, recipe="frame", wants=("D1 u8", "chunks and a ragged tail")),
    _C("d2_u8", CHUNK + 1, D=2, u8=True, K=4, A=16, max_iter=5, wants=("D2 u8", "one above a chunk", "A=16")),
    _C("d3_u8", 2000, D=3, u8=True, K=6, A=5, wants=("D3 u8",)),
    _C("d4_u8", 900, D=4, u8=True, K=3, A=2, wants=("D4 u8",)),
    # the reference's shape: the triples of a 66 x 33 residual-magnitude image, the defaults
    _C("frame_66x33", 66 * 33 // 3, recipe="frame", wants=("D3 f32",)),
    # the smallest sample counts
    _C("n_is_k", 8, D=2, A=3, wants=("N=K",)),
    _C("n_is_k_plus_1", 9, D=3, A=3, wants=("N=K+1",)),
    _C("k1_a1", 700, D=3, K=1, A=1, wants=("K=1", "A=1")),
    # repairs
    _C("far_centres", 600, D=2, K=8, A=3, recipe="far", wants=("repair", "K-1 repairs in one update")),
    _C("far_centres_k16_u8", CHUNK + 300, D=3, u8=True, K=16, A=2, max_iter=4, recipe="far", wants=("K-1 repairs in one update", "K=16")),
    _C("identical", 300, D=3, K=4, A=2, recipe="identical", wants=("repair at distance 0", "highest index among equals", "K-1 repairs in one update")),
    _C("identical_u8", CHUNK + 70, D=1, u8=True, K=3, A=2, max_iter=3, recipe="identical", wants=("repair at distance 0", "highest index among equals")),
    # the first minimum
    _C("equidistant", 500, D=1, K=4, A=3, recipe="equidistant", wants=("two nearest centres",)),
    _C("equidistant_u8", 500, D=2, u8=True, K=5, A=2, recipe="equidistant", wants=("two nearest centres",)),
    # the loop's ends
    _C("max_iter_2", 1200, D=3, K=6, A=4, max_iter=2, wants=("max_iter 2", "runs into max_iter")),
    _C("eps_0", 1200, D=2, K=5, A=4, eps=0.0, max_iter=30, wants=("eps 0",)),
    _C("twin_attempts", 1000, D=3, K=5, A=2, recipe="twin", wants=("compactness tie",)),
    _C("later_wins", 2500, D=2, K=8, A=10, wants=("a later attempt wins", "attempts stop at different iterations", "runs into max_iter")),
    # a batch of different images
    _C("batch3", CHUNK + 77, D=3, K=6, A=4, B=3, wants=("batch 3",)),
    _C("batch3_u8", 131 * 67, D=1, u8=True, K=4, A=3, B=3, max_iter=5, recipe="frame", wants=("batch 3",)),
)}
ALL_TAGS = sorted({t for c in CASES.values() for t in c.wants})


def hash_name(name: str) -> int:
    return _seed(name)


def general_samples(seed: int, N: int, D: int) -> np.ndarray:
    """float32 samples off every grid: noise x 1e3 with a spread of 34 binary exponents (24 + 34 + log2 N bits are more than
    float64's 53) -- float64 sums of these depend on their order"""
    rng = np.random.default_rng(seed)
    return (rng.normal(0, 1, (N, D)) * 1e3 * 2.0 ** rng.integers(-28, 6, (N, D))).astype(np.float32)


def general_init(seed: int, x: np.ndarray, A: int, K: int) -> np.ndarray:
    rng = np.random.default_rng(seed + 1)
    return x[rng.integers(0, x.shape[0], (A, K))].astype(np.float32) + rng.normal(0, 1, (A, K, x.shape[1])).astype(np.float32)
