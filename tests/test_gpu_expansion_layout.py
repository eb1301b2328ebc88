"""The polynomial expansions lie (h, w, 5) on the device: the five values of a pixel together, the gather's row of two pixels 40
adjacent bytes.  The stage hooks keep their contract of five planes, so the stage, flow and schedule tests hold the kernels to the
oracle as before; this file holds what only the layout can break:

  * the whole call equals the chain of stage calls per layer, bit for bit -- the hooks transpose at the edge, the whole call never does,
    so a kernel and a hook that disagree about the layout part here;
  * the gather at the edges of the interleaved rows: floor(x + dx) at -1, 0, w - 2, w - 1 and floor(y + dy) at -1, 0, h - 2, h - 1 for
    EVERY pixel (the first and last lane of every wave among them), on layers 64, 65 and 127 wide and 1, 2 and 17 high.  One row: no
    neighbourhood is inside, the result is the outside branch's and owes nothing to R1;
  * the pair form equals the sequence form: the shared frame's expansion is R1 of one pair and R0 of the next.
"""
import numpy as np
import pytest

from mavflow import synth
from stage_cases import sweep_form

pytestmark = pytest.mark.gpu


def soa(a):
    return np.ascontiguousarray(np.moveaxis(a, -1, 0))


def _chain(ctx, prev, nxt, iterations):
    """farneback(prev, next) spelled as stage calls: per layer, coarsest first, blur + resize -> expansion -> initial M (zero flow at
    the top, the coarser layer's flow below it) -> `iterations` sweeps, all but the last rebuilding M."""
    flow = None
    for k in reversed(range(ctx.num_layers())):
        R0, R1 = (ctx.stage_polyexp(ctx.stage_blur_resize(img, k), k) for img in (prev, nxt))
        M = ctx.stage_update_matrices_from(R0, R1, flow, k)
        for it in range(iterations):
            flow, M = ctx.stage_blur_iter(R0, R1, M, k, it < iterations - 1)
    return flow


# (W, H, winsize, layers, the sweep form of every layer).  The first three are one-layer frames (a second layer needs 80 x 80 at the
# default pyr_scale 0.4): 66 x 18 is one 64 x 16 tile plus 2 pixels each way, 130 x 34 the same with two tiles each way, 40 x 21 at
# winsize 9 the generic sweep.  68 x 18 is the fast form as written (w % 4 == 0); the two 2-layer frames bring the initial M from the
# coarser flow (k_update_matrices<1>) next to the one from zero, in the fast form as written and in the relaxed one.
CHAIN_CASES = [(66, 18, 12, 1, ["fast<6,false>"]),
               (130, 34, 12, 1, ["fast<6,false>"]),
               (40, 21, 9, 1, ["generic<0>"]),
               (68, 18, 12, 1, ["fast<6>"]),
               (160, 90, 12, 2, ["fast<6>", "fast<6>"]),
               (166, 86, 12, 2, ["fast<6,false>", "fast<6,false>"])]


@pytest.mark.parametrize("W,H,winsize,layers,forms", CHAIN_CASES, ids=[f"{c[0]}x{c[1]}-win{c[2]}" for c in CHAIN_CASES])
def test_whole_call_equals_the_chain_of_stage_calls(mav, W, H, winsize, layers, forms):
    from mavflow import _lib
    fb = _lib.fb_defaults()                           # default levels
    fb.winsize = winsize
    prev, nxt, _ = synth.make_pair(W, H, 3)
    with _lib.Context(W, H, 1, fb) as ctx:
        assert ctx.num_layers() == layers
        assert [sweep_form(ctx.layer_dims(k)[0], winsize) for k in range(layers)] == forms
        whole = ctx.farneback(prev[None], nxt[None])[0].copy()
        chain = _chain(ctx, prev, nxt, fb.iterations)
    assert np.isfinite(whole).all()
    assert whole.tobytes() == chain.tobytes(), (W, H, int((whole != chain).any(axis=-1).sum()))


def _edge_flows(w, h):
    """16 fields; in field (i, j) every pixel is displaced to (tx + 0.25, ty + 0.75) with tx, ty the i-th / j-th of the edge columns / rows.
    All the sums are exact in float32."""
    x = np.arange(w, dtype=np.float32)[None, :]
    y = np.arange(h, dtype=np.float32)[:, None]
    for tx in (-1, 0, w - 2, w - 1):
        for ty in (-1, 0, h - 2, h - 1):
            flow = np.empty((h, w, 2), np.float32)
            flow[..., 0] = np.float32(tx + 0.25) - x
            flow[..., 1] = np.float32(ty + 0.75) - y
            assert (np.floor(x + flow[..., 0]) == tx).all() and (np.floor(y + flow[..., 1]) == ty).all()
            yield tx, ty, flow


@pytest.fixture(scope="module")
def expansions():
    """Two expansions per layer size, (h, w, 5) as the oracle takes them: every channel of every pixel its own value."""
    rng = np.random.default_rng(17)
    return {(w, h): [rng.normal(0, 1, (h, w, 5)).astype(np.float32) for _ in range(2)] for w in (64, 65, 127) for h in (1, 2, 17)}


@pytest.mark.parametrize("h", [1, 2, 17])
@pytest.mark.parametrize("w", [64, 65, 127])
def test_gather_at_the_edges_of_the_interleaved_rows(mav, fb_oracle, expansions, w, h):
    from mavflow import _lib
    R0, R1 = expansions[(w, h)]
    with _lib.Context(w, h, 1) as ctx:
        assert ctx.num_layers() == 1 and ctx.layer_dims(0)[:2] == (w, h)
        for tx, ty, flow in _edge_flows(w, h):
            got = ctx.stage_update_matrices(soa(R0), soa(R1), flow, 0)
            exp = soa(fb_oracle.update_matrices(R0, R1, flow))
            np.testing.assert_allclose(got, exp, rtol=1e-4, atol=1e-6 * np.abs(exp).max(), err_msg=f"{w}x{h} floor -> ({tx}, {ty})")   # tests/test_gpu_stages.py's bound
            inside = 0 <= tx < w - 1 and 0 <= ty < h - 1
            if not inside:                                      # the outside branch: R1 is not part of the result
                nan = ctx.stage_update_matrices(soa(R0), np.full((5, h, w), np.nan, np.float32), flow, 0)
                assert np.isfinite(nan).all() and nan.tobytes() == got.tobytes(), (w, h, tx, ty)
        # the sweep's own gather issues its loads whether the neighbourhood is inside or not and redirects the off-image ones (on a
        # one-row layer: all of them): one updating sweep leaves M' == UpdateMatrices(the flow it stored), as tests/test_gpu_stages.py pins it
        M = soa(fb_oracle.update_matrices(R0, R1, flow)).astype(np.float32)
        gflow, gM = ctx.stage_blur_iter(soa(R0), soa(R1), M, 0, True)
        assert np.isfinite(gM).all() and np.array_equal(gM, ctx.stage_update_matrices(soa(R0), soa(R1), gflow, 0)), (w, h)


def test_pair_form_equals_sequence_form(mav):
    from mavflow import _lib
    W, H = 130, 34
    frames = synth.make_sequence(W, H, 3, seed=5, k=0.02)
    with _lib.Context(W, H, 2) as ctx:
        seq = ctx.farneback_sequence(frames).copy()                              # one run of three frames: two expansions shared
        pairs = ctx.farneback(frames[:-1].copy(), frames[1:].copy()).copy()      # two pairs, four expansions
        alone = [ctx.farneback(frames[i:i + 1].copy(), frames[i + 1:i + 2].copy())[0].copy() for i in range(2)]
    assert np.isfinite(seq).all() and np.abs(seq).max() > 0
    assert seq.tobytes() == pairs.tobytes()
    assert all(seq[i].tobytes() == alone[i].tobytes() for i in range(2))
