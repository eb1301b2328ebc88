"""The flow history's ring in the context's memory ledger, and what a refused push leaves behind: nothing."""
import ctypes as C

import numpy as np
import pytest

import history_cases as hc
import history_ref as R

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("L,dtype", [(3, np.float32), (20, np.float32), (5, np.float64), (64, np.float64)])
def test_ring_is_counted_and_returned(mav, L, dtype):
    from mavflow import _lib
    W, H = 53, 31
    with _lib.Context(W, H, 1) as ctx:
        before = ctx.mem_info()
        hist = ctx.flow_history(L, dtype)
        ring = L * W * H * 2 * np.dtype(dtype).itemsize
        after = ctx.mem_info()
        assert hist.ring_bytes == ring and after["ctx_bytes"] - before["ctx_bytes"] == ring
        assert after["workspace_bytes"] == before["workspace_bytes"] == 0            # not the Farneback workspace
        hist.close()
        assert ctx.mem_info()["ctx_bytes"] == before["ctx_bytes"]
        hist.close()                                                                  # closing twice is harmless
    # a history left open goes with its context; closing it afterwards is harmless too
    ctx = _lib.Context(W, H, 1)
    hist = ctx.flow_history(L, dtype)
    ctx.close()
    hist.close()


def test_create_refuses_bad_parameters_and_keeps_nothing(mav):
    from mavflow import _lib
    with _lib.Context(16, 8, 1) as ctx:
        base = ctx.mem_info()["ctx_bytes"]
        for L in (2, 0, 65):
            with pytest.raises(ValueError):
                ctx.flow_history(L)
        for kw in (dict(dtype=np.uint8), dict(dtype=np.float16), dict(axes="yx")):
            with pytest.raises(ValueError):
                ctx.flow_history(4, **kw)
        assert ctx.mem_info()["ctx_bytes"] == base


def test_refused_push_leaves_ring_index_and_outputs_untouched(mav):
    from mavflow import _lib
    c = hc.BY_NAME["planted37x23_f32tof32_reference_reference"]
    fields, (want, _) = hc.fields_of(c), hc.reference(c.name)
    lib = _lib.load()
    with _lib.Context(c.W, c.H, 1) as ctx, _lib.Context(c.W, c.H, 1) as other:
        hist, foreign = ctx.flow_history(c.L), other.flow_history(c.L)
        for i in range(3):
            hist.push(fields[i])
        state = (hist.index, hist.pushes)
        out = np.full((2, c.H, c.W, 2), np.float64(-77.0))
        f32, f64 = np.ascontiguousarray(fields[3:5]), np.ascontiguousarray(fields[3:5]).astype(np.float64)
        p = _lib._ptr
        refused = {
            "float64 into a float32 ring": (ctx.h, hist._h, p(f64), _lib.DEPTH_64F, 1, 0, p(out)),
            "flow_depth": (ctx.h, hist._h, p(f32), _lib.DEPTH_16U, 1, 0, p(out)),
            "out_form": (ctx.h, hist._h, p(f32), _lib.DEPTH_32F, 1, 5, p(out)),
            "count 0": (ctx.h, hist._h, p(f32), _lib.DEPTH_32F, 0, 0, p(out)),
            "count too large": (ctx.h, hist._h, p(f32), _lib.DEPTH_32F, 2 ** 30, 0, p(out)),
            "another context's history": (ctx.h, foreign._h, p(f32), _lib.DEPTH_32F, 1, 0, p(out)),
            "NULL out": (ctx.h, hist._h, p(f32), _lib.DEPTH_32F, 1, 0, None),
            "overlap": (ctx.h, hist._h, p(out), _lib.DEPTH_32F, 1, 0, C.c_void_p(p(out).value + 8)),
            "misaligned": (ctx.h, hist._h, C.c_void_p(p(f32).value + 2), _lib.DEPTH_32F, 1, 0, p(out)),
        }
        for fn in (lib.mav_history_push, lib.mav_history_push_dev):
            for what, args in refused.items():
                assert fn(*args) == _lib.MAV_ERR_ARG, what
                assert lib.mav_last_error(), what
                assert (hist.index, hist.pushes) == state, what
        assert (out == -77.0).all()
        with pytest.raises(ValueError):
            hist.push(f64[0])
        with pytest.raises(ValueError):
            hist.push(f32[0], out="uv")
        with pytest.raises(ValueError):
            hist.push(np.zeros((c.H, c.W + 1, 2), np.float32))
        assert (hist.index, hist.pushes) == state and (foreign.index, foreign.pushes) == (0, 0)
        # the ring is what it was: the pushes that follow give the restatement's bytes
        for i in range(3, c.n_pushes):
            got = hist.push(fields[i])
            assert np.array_equal(R.bits(got), R.bits(want[i])), i
        hist.close()
        foreign.close()
