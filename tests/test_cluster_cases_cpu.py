"""tests/cluster_cases.py held to its own promises without a GPU: every case reaches the instantiation, the shape or the control path it
is named after (computed from the inputs and the restatement's trace), the table as a whole names every (D, element type) instantiation
of csrc/kernels_cluster.hip and every control path, the chunk size is the source's, and every float32 case meets the condition under
which the float64 sums are exact in any order."""
import re

import numpy as np
import pytest

import cluster_cases as T
import kmeans_ref as R


def test_constants_are_the_sources():
    k = T.source_constants()
    assert k["MAV_KMEANS_CHUNK"] == T.CHUNK == R.CHUNK == k["KM_THREADS"] * k["KM_PER_THREAD"]
    assert (k["MAV_KMEANS_MAX_K"], k["MAV_KMEANS_MAX_ATTEMPTS"], k["MAV_KMEANS_MAX_DIMS"]) == (R.MAX_K, R.MAX_ATTEMPTS, R.MAX_DIMS) == (16, 16, 4)
    src = open(T.KERNELS).read()
    # the dispatch instantiates D = 1..4 for both element types
    assert all(f"km_run<{d}, T>" in src for d in (1, 2, 3, 4)) and "km_run_dims<uint8_t>" in src and "km_run_dims<float>" in src
    assert not re.search(r"atomicAdd\s*\(\s*\(?\s*(float|double)|unsafeAtomicAdd", src)       # no floating-point atomics


@pytest.mark.parametrize("name", list(T.CASES))
def test_case_reaches_what_it_is_there_for(name):
    c = T.CASES[name]
    got = T.reaches(name)
    assert set(c.wants) <= got, (name, sorted(set(c.wants) - got))
    assert 1 <= c.K <= 16 and 1 <= c.A <= 16 and 1 <= c.D <= 4 and c.N >= c.K
    ins = T.inputs(name)
    assert ins["samples"].shape == (c.B, c.N, c.D) and ins["samples"].dtype == c.dtype
    assert ins["init"].shape == (c.B, c.A, c.K, c.D) and ins["init"].dtype == np.float32 and np.isfinite(ins["init"]).all()
    assert T.exact_condition(ins["samples"])                              # uint8 cases meet it by construction
    for ref in ins["ref"]:
        assert ref["counts"][:c.K].min() >= 1 and ref["counts"].sum() == c.N and ref["labels"].shape == (c.N,)
        assert 1 <= ref["iterations"] <= R.clamp_iter(c.max_iter) - 1


def test_the_table_names_every_form_and_path():
    reached = set().union(*(T.reaches(n) for n in T.CASES))
    wanted = set().union(*(set(c.wants) for c in T.CASES.values()))
    forms = {f"D{d} {t}" for d in (1, 2, 3, 4) for t in ("f32", "u8")}
    paths = {"N=K", "N=K+1", "one below a chunk", "one chunk", "one above a chunk", "chunks and a ragged tail", "K=1", "K=8", "K=16", "A=1", "A=10",
             "A=16", "repair", "K-1 repairs in one update", "repair at distance 0", "highest index among equals", "two nearest centres",
             "attempts stop at different iterations", "runs into max_iter", "max_iter 2", "eps 0", "compactness tie", "a later attempt wins",
             "batch 3"}
    assert forms | paths <= wanted <= reached
    sizes = {T.CASES[n].N for n in T.CASES}
    assert {66 * 33 // 3, 131 * 67} <= sizes and 66 * 33 // 3 == 726


def test_general_samples_are_off_the_grid():
    x = T.general_samples(5, 3 * T.CHUNK + 517, 3)
    assert x.dtype == np.float32 and np.isfinite(x).all() and not T.exact_condition(x)
    e = np.frexp(x[x != 0])[1]
    assert e.max() - e.min() >= 16                                        # a wide spread of exponents
    s = x[:, 0].astype(np.float64)
    assert np.sum(s) != np.sum(s[::-1]) or np.sum(s) != sum(s.tolist())   # their float64 sum does depend on the order
