"""mav_kmeans and mav_kmeans_dev (include/mavflow_cluster.h) on the device against tests/kmeans_ref.py: every case of
tests/cluster_cases.py through both forms -- labels, centres, counts, iterations, repairs, best attempt and shift EQUAL the restatement's
(the cases' samples are multiples of 2^-8 below 2^12, uint8 ones by construction: every float64 sum of samples is exact in any order, so
the restatement need not mimic the device's), the compactness, whose terms are no grid values, to 1e-12 relative.  The _dev runs hand in
every caller pointer at its minimum alignment.  Order-independence is demanded separately on GENERAL float32 samples, by equality of all
output bytes, compactness included: the same call twice, the same image at batch positions 0, 1 and 2, a context with another max_batch,
the host form against the _dev form.  A refused _dev call leaves canary-filled outputs untouched.  mav_kmeans_paint equals
kmeans_ref.paint.  One case at 150 000 000 samples puts label offsets past 2^31 and more chunks than a launch has workgroups."""
import ctypes as C
import os

import numpy as np
import pytest

import cluster_cases as T
import kmeans_ref as R

pytestmark = pytest.mark.gpu
W, H, MB = 160, 120, 3                  # a context's staging bound is max_batch * W * H * 4 values: above every case's batch * N * D
CANARY = 0xA5


@pytest.fixture(scope="module")
def ctx(mav):
    from mavflow import _lib
    with _lib.Context(W, H, MB) as c:
        yield c


def _params(K, A, max_iter, eps, D, dtype):
    from mavflow import clustering
    return clustering.kmeans_params(K, A, max_iter, D, dtype, eps)


def run_host(ctx, x, init, max_iter, eps):
    """mav_kmeans on host arrays x (B, N, D), init (B, A, K, D): (labels, centers, records)"""
    from mavflow import _lib, clustering
    B, N, D = x.shape
    A, K = init.shape[1:3]
    p = _params(K, A, max_iter, eps, D, x.dtype)
    labels, centers, rec = np.full((B, N), -1, np.int32), np.full((B, K, D), np.nan, np.float32), np.zeros(B, clustering.RECORD_DTYPE)
    _lib.check(clustering.load().mav_kmeans(ctx.h, _lib._ptr(np.ascontiguousarray(x)), N, B, C.byref(p), _lib._ptr(np.ascontiguousarray(init)),
                                            _lib._ptr(labels), _lib._ptr(centers), _lib._ptr(rec)))
    return labels, centers, rec


class DevBlocks:
    """Caller-owned device blocks of one _dev call, each handed in at its MINIMUM alignment (the element size; records and workspace 16)
    and filled with a canary first."""

    def __init__(self, ctx, x, init, ws_bytes):
        from mavflow import clustering
        self.ctx = ctx
        B, N, D = x.shape
        K = init.shape[2]
        self.shapes = dict(labels=((B, N), np.int32), centers=((B, K, D), np.float32), rec=((B,), clustering.RECORD_DTYPE))
        sizes = dict(x=(x.nbytes, x.dtype.itemsize), init=(init.nbytes, 4), labels=(B * N * 4, 4), centers=(B * K * D * 4, 4), rec=(B * 96, 16),
                     ws=(ws_bytes, 16))
        self.buf, self.ptr, self.size = {}, {}, {}
        for k, (n, off) in sizes.items():
            self.buf[k] = ctx.alloc(n + 256)
            self.buf[k].upload(np.full(n + 256, CANARY, np.uint8))
            self.ptr[k] = self.buf[k].ptr + off
            self.size[k] = n
            assert self.ptr[k] % (2 * off) != 0 or off == 1               # not aligned to anything more
        for k, a in (("x", x), ("init", init)):
            a = np.ascontiguousarray(a)
            ctx.lib.mav_memcpy_h2d(ctx.h, self.ptr[k], a.ctypes.data, a.nbytes)

    def get(self, k):
        shape, dtype = self.shapes[k]
        out = np.empty(shape, dtype)
        self.ctx.lib.mav_memcpy_d2h(self.ctx.h, out.ctypes.data, self.ptr[k], out.nbytes)
        return out

    def raw(self, k):
        return self.buf[k].download(np.uint8, (self.size[k] + 256,))

    def close(self):
        for b in self.buf.values():
            b.free()


def run_dev(ctx, x, init, max_iter, eps):
    from mavflow import _lib, clustering
    B, N, D = x.shape
    A, K = init.shape[1:3]
    p = _params(K, A, max_iter, eps, D, x.dtype)
    need = ctx.kmeans_workspace_bytes(N, B, K, A, D, x.dtype)
    d = DevBlocks(ctx, x, init, need)
    try:
        _lib.check(clustering.load().mav_kmeans_dev(ctx.h, d.ptr["x"], N, B, C.byref(p), d.ptr["init"], d.ptr["labels"], d.ptr["centers"], d.ptr["rec"],
                                                    d.ptr["ws"], need))
        ctx.sync()
        return d.get("labels"), d.get("centers"), d.get("rec")
    finally:
        d.close()


def _same_bytes(a, b):
    return all(u.tobytes() == v.tobytes() for u, v in zip(a, b))


@pytest.mark.parametrize("name", list(T.CASES))
def test_case_equals_the_restatement(ctx, name):
    c, ins = T.CASES[name], T.inputs(name)
    x, init = ins["samples"], ins["init"]
    outs = {"mav_kmeans": run_host(ctx, x, init, c.max_iter, c.eps), "mav_kmeans_dev": run_dev(ctx, x, init, c.max_iter, c.eps)}
    for form, (labels, centers, rec) in outs.items():
        for b, ref in enumerate(ins["ref"]):
            r = rec[b]
            got = (int(r["best_attempt"]), int(r["iterations"]), int(r["repairs"]))
            print(f"{name} {form} image {b}: best/iterations/repairs {got}, compactness {r['compactness']!r} (restatement {ref['compactness']!r}), "
                  f"launches that left at once {int(r['skipped'])}")
            assert got == (ref["best_attempt"], ref["iterations"], ref["repairs"]), (form, b)
            assert np.array_equal(r["counts"], ref["counts"]), (form, b)
            assert np.array_equal(labels[b], ref["labels"]), (form, b, int(np.sum(labels[b] != ref["labels"])))
            assert centers[b].tobytes() == ref["centers"].tobytes(), (form, b)
            assert r["shift"] == ref["shift"], (form, b)
            assert abs(r["compactness"] - ref["compactness"]) <= 1e-12 * abs(ref["compactness"]), (form, b)
    assert _same_bytes(outs["mav_kmeans"], outs["mav_kmeans_dev"])


# ---- order-independence on general samples: equality of every output byte -----------------------------------------------------------------
GN, GD, GK, GA, GITER = 3 * T.CHUNK + 517, 3, 8, 4, 6


@pytest.fixture(scope="module")
def general():
    xs = np.stack([T.general_samples(40 + b, GN, GD) for b in range(3)])
    init = np.stack([T.general_init(40 + b, xs[b], GA, GK) for b in range(3)])
    assert not T.exact_condition(xs)
    return xs, init


def test_general_samples_same_call_twice_and_host_against_dev(ctx, general):
    xs, init = general
    first = run_host(ctx, xs, init, GITER, 1.0)
    again = run_host(ctx, xs, init, GITER, 1.0)
    dev = run_dev(ctx, xs, init, GITER, 1.0)
    assert _same_bytes(first, again) and _same_bytes(first, dev)
    labels, centers, rec = first
    for b in range(3):                                      # and they are k-means results: the restatement's up to the order of its sums
        ref = R.kmeans(xs[b], init[b], GITER, 1.0)
        assert abs(rec[b]["compactness"] - ref["compactness"]) <= 1e-6 * ref["compactness"]
        assert np.mean(labels[b] == ref["labels"]) > 0.999 and rec[b]["counts"].sum() == GN


def test_general_samples_every_batch_position(ctx, general):
    xs, init = general
    base = run_host(ctx, xs, init, GITER, 1.0)
    for shift in (1, 2):
        order = [(b + shift) % 3 for b in range(3)]
        got = run_host(ctx, xs[order], init[order], GITER, 1.0)
        for pos, b in enumerate(order):
            assert _same_bytes([a[b] for a in base], [a[pos] for a in got]), (shift, pos, b)
    alone = run_dev(ctx, xs[2:3], init[2:3], GITER, 1.0)
    assert _same_bytes([a[2] for a in base], [a[0] for a in alone])


def test_general_samples_another_max_batch(ctx, general, mav):
    from mavflow import _lib
    xs, init = general
    base = run_host(ctx, xs, init, GITER, 1.0)
    with _lib.Context(W + 7, H + 2, 5) as other:
        five = run_host(other, np.concatenate([xs, xs[:2]]), np.concatenate([init, init[:2]]), GITER, 1.0)
        assert _same_bytes(base, [a[:3] for a in five]) and _same_bytes([a[:2] for a in base], [a[3:] for a in five])
        assert _same_bytes(base, run_dev(other, xs, init, GITER, 1.0))


def test_refused_dev_calls_leave_the_outputs_untouched(ctx):
    from mavflow import _lib, clustering
    c, ins = T.CASES["d3_u8"], T.inputs("d3_u8")
    x, init = ins["samples"], ins["init"]
    p = _params(c.K, c.A, c.max_iter, c.eps, c.D, x.dtype)
    need = ctx.kmeans_workspace_bytes(c.N, 1, c.K, c.A, c.D, x.dtype)
    d = DevBlocks(ctx, x, init, need)
    lib = clustering.load()
    try:
        args = [ctx.h, d.ptr["x"], c.N, 1, C.byref(p), d.ptr["init"], d.ptr["labels"], d.ptr["centers"], d.ptr["rec"], d.ptr["ws"], need]
        small = list(args)
        small[10] = need - 1
        crooked = list(args)
        crooked[8] = d.ptr["rec"] + 8
        many = list(args)
        many[3], many[10] = MB + 1, need * (MB + 1)
        for what, a in (("workspace of", small), ("records is not aligned", crooked), ("batch", many)):
            assert lib.mav_kmeans_dev(*a) == _lib.MAV_ERR_ARG, what
            assert b"mav_kmeans_dev:" in lib.mav_last_error() and what.encode() in lib.mav_last_error()
        ctx.sync()
        for k in ("labels", "centers", "rec", "ws"):
            assert np.all(d.raw(k) == CANARY), k
        _lib.check(lib.mav_kmeans_dev(*args))               # and the same blocks serve the good call: nothing outside them is written
        ctx.sync()
        assert np.array_equal(d.get("labels")[0], ins["ref"][0]["labels"])
        for k in ("labels", "centers", "rec", "ws"):
            raw, n, off = d.raw(k), d.size[k], d.ptr[k] - d.buf[k].ptr
            assert np.all(raw[:off] == CANARY) and np.all(raw[off + n:] == CANARY), k
        # every byte of the record is written: the canary-filled block holds what the host form puts into a zeroed one
        assert d.get("rec").tobytes() == run_host(ctx, x, init, c.max_iter, c.eps)[2].tobytes()
    finally:
        d.close()


# ---- paint -----------------------------------------------------------------------------------------------------------------------------
def _paint_cases():
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "clustering.npz"), allow_pickle=False)
    out = {str(n): (g[f"{n}_labels"].reshape(1, -1), g[f"{n}_centers"][None]) for n in g["cases"]}
    rng = np.random.default_rng(9)
    out["d1 k16 ragged"] = (rng.integers(0, 16, (1, 1031)).astype(np.int32), rng.uniform(0, 90, (1, 16, 1)).astype(np.float32))
    out["d4 batch3"] = (rng.integers(0, 5, (3, 700)).astype(np.int32), rng.uniform(0, 3, (3, 5, 4)).astype(np.float32))
    out["d2 all zero but one"] = (rng.integers(0, 3, (1, 300)).astype(np.int32), np.array([[[0, 0], [0, 7.5], [0, 0]]], np.float32))
    return out


@pytest.mark.parametrize("name", list(_paint_cases()))
def test_paint_equals_the_restatement(ctx, name):
    from mavflow import _lib, clustering
    labels, centers = _paint_cases()[name]
    B, N = labels.shape
    K, D = centers.shape[1:]
    want = [R.paint(labels[b], centers[b]) for b in range(B)]
    res, mask = ctx.kmeans_paint(labels, centers)
    bufs = [ctx.alloc(a.nbytes).upload(a) for a in (labels, centers)] + [ctx.alloc(B * N * D), ctx.alloc(B * N)]
    try:
        ctx.kmeans_paint_enqueue(bufs[0], bufs[1], N, B, K, D, bufs[2], bufs[3])
        ctx.sync()
        dres, dmask = bufs[2].download(np.uint8, (B, N, D)), bufs[3].download(np.uint8, (B, N))
        ctx.kmeans_paint_enqueue(bufs[0], bufs[1], N, B, K, D, bufs[2], None)      # without a mask
        ctx.sync()
        assert np.array_equal(bufs[2].download(np.uint8, (B, N, D)), dres)
    finally:
        for b in bufs:
            b.free()
    for b in range(B):
        assert np.array_equal(res[b], want[b][0]) and np.array_equal(mask[b], want[b][1]), b
        assert np.array_equal(dres[b], want[b][0]) and np.array_equal(dmask[b], want[b][1]), b
    assert set(np.unique(mask).tolist()) <= {0, 1}


# ---- indices past 2^31 and the strided grid -----------------------------------------------------------------------------------------------
def test_label_offsets_past_2_31_and_more_chunks_than_workgroups(ctx):
    """150 000 000 uint8 samples x 16 attempts: attempt 15's label bytes start at 15 * N = 2.25e9 > 2^31, the slab has 36 622 chunks for a grid
    of at most 1 024 workgroups per image (every other case has fewer chunks than that), and the repair's argmax packs indices above 2^27.
    The samples are i mod 251, so the restatement is taken per VALUE (251 of them) and weighted by how often each occurs -- every sum is an
    integer, exact in any order.  Attempts 0..14 start beyond the data (one repair each, all with the same result); attempt 15 splits it
    and wins."""
    from mavflow import _lib, clustering
    N, P, A, K = 150_000_000, 251, 16, 2
    assert (A - 1) * N > 1 << 31 and -(-N // T.CHUNK) > T.source_constants()["KM_GRID_CAP"]
    values = np.arange(P, dtype=np.float32).reshape(-1, 1)
    cnt = (N // P + (np.arange(P) < N % P)).astype(np.int64)
    init = np.array([[[300.0 + a], [400.0 + a]] for a in range(A - 1)] + [[[60.0], [190.0]]], np.float32)[None]
    # the winning attempt, per value
    lv, _ = R.assign(values, init[0, A - 1])
    n = np.array([cnt[lv == k].sum() for k in range(K)])
    S = np.array([(cnt * np.arange(P))[lv == k].sum() for k in range(K)], np.float64)
    centers = (S / n.astype(np.float64)).astype(np.float32).reshape(K, 1)
    compact = float(np.sum(cnt * R.dist(values, centers[lv]).astype(np.float64)))
    t = (centers - init[0, A - 1]).astype(np.float64)
    shift = float((t[:, 0] * t[:, 0]).max())
    # a far attempt: everything in cluster 0, the farthest value's last occurrence moves to cluster 1 -- a worse compactness
    m = np.float32(float((cnt * np.arange(P)).sum()) / float(N))
    dd = R.dist(values, np.array([m], np.float32))
    far_v = [int(v) for v in np.nonzero(dd == dd.max())[0]]
    j = max(v + P * ((N - 1 - v) // P) for v in far_v)
    c_far = np.array([[np.float32((float((cnt * np.arange(P)).sum()) - j % P) / float(N - 1))], [np.float32(j % P)]], np.float32)
    cnt_far = cnt.copy()
    cnt_far[j % P] -= 1
    assert float(np.sum(cnt_far * R.dist(values, c_far[0]).astype(np.float64))) > 2 * compact and j > 1 << 27
    x = np.tile(np.arange(P, dtype=np.uint8), N // P + 1)[:N]
    need = ctx.kmeans_workspace_bytes(N, 1, K, A, 1, np.uint8)
    assert need > 1 << 31
    bufs = [ctx.alloc(x.nbytes).upload(x), ctx.alloc(init.nbytes).upload(init), ctx.alloc(4 * N), ctx.alloc(4 * K), ctx.alloc(96), ctx.alloc(need)]
    try:
        ctx.kmeans_enqueue(bufs[0], N, 1, bufs[1], bufs[2], bufs[3], bufs[4], bufs[5], need, K=K, attempts=A, max_iter=2, eps=0.0, dims=1, dtype=np.uint8)
        ctx.sync()
        rec = bufs[4].download(clustering.RECORD_DTYPE, (1,))[0]
        got_c = bufs[3].download(np.float32, (K, 1))
        labels = bufs[2].download(np.int32, (N,))
    finally:
        for b in bufs:
            b.free()
    print(f"best/iterations/repairs {(int(rec['best_attempt']), int(rec['iterations']), int(rec['repairs']))}, compactness {rec['compactness']!r} (per value: {compact!r})")
    assert (int(rec["best_attempt"]), int(rec["iterations"]), int(rec["repairs"])) == (A - 1, 1, A - 1)
    assert list(rec["counts"][:K]) == list(n) and not rec["counts"][K:].any()
    assert got_c.tobytes() == centers.tobytes() and rec["shift"] == shift
    assert abs(rec["compactness"] - compact) <= 1e-12 * compact
    assert np.array_equal(labels, np.tile(lv.astype(np.int32), N // P + 1)[:N])
