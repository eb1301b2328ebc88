"""What the mav_last_* readers return after every other entry point has run in between (tests/resident_cases.py is the table).

Per producer: the baseline -- the producer, then every reader that applies, each held to the direct call on the same inputs -- and
then, for every form of every intervener, the sequences  producer, intervener, readers  (twice: the second grows no memory) and
producer, reader, intervener, readers.  Class `keeps`: every reader returns MAV_OK and the baseline's bytes.  Class `drops`: every
reader of that kind returns MAV_ERR_STATE with its canary-filled outputs untouched, and a following producer plus reader gives the
baseline again.  A reader that returns OK with other bytes is reported as "silently different" under either class.

For the flow kind, whose reader has no error state, "drops" reads "replaced": mav_last_flow_dev must report where the intervener's flow
went and the bytes of that flow (resident_cases.alt_flows, from a context of its own).

A posted step is waited for, and the worker drained, before any reader runs.  A call that answers MAV_ERR_HIP or MAV_ERR_OOM -- as a
return code, or as the MavflowError / MemoryError that the bindings of the producers, ctx.sync() and the copies raise for it -- ends
the context's sequences at once (nothing is repeated).  Every refusal used is one the library makes from its arguments alone.

Measured on an MI355X: see profiles/resident/README.md (the slowest parametrised case, and which sequences fail on the parent)."""
import numpy as np
import pytest

import resident_cases as rc

pytestmark = pytest.mark.gpu
W, H, B = rc.W, rc.H, rc.B


@pytest.fixture(scope="module")
def ref(mav):
    """a context of its own for the direct calls, so that they disturb nothing resident"""
    from mavflow import _lib
    with _lib.Context(W, H, B) as ctx:
        yield ctx


@pytest.fixture(scope="module")
def alt_flows(ref):
    return rc.alt_flows(ref)


def _first_diff(a, b):
    fa = b"".join(x if isinstance(x, bytes) else repr(x).encode() for x in _flat(a))
    fb = b"".join(x if isinstance(x, bytes) else repr(x).encode() for x in _flat(b))
    n = next((i for i, (p, q) in enumerate(zip(fa, fb)) if p != q), min(len(fa), len(fb)))
    return f"first differing byte {n} of {len(fa)}"


def _flat(v):
    if isinstance(v, (tuple, list)):
        for x in v:
            yield from _flat(x)
    else:
        yield v


def _checked(rcode, what):
    if rcode in (rc.ERR_HIP, rc.ERR_OOM):
        from mavflow import _lib
        raise rc.HipFailure(f"{what}: [{rcode}] {_lib.load().mav_last_error().decode('utf-8', 'replace')}")
    return rcode


def _read(env, name):
    code, outs, value = rc.READERS[name][2](env)
    return _checked(code, name), outs, value


def _mem(env):
    m = env.ctx.mem_info()
    return m["ctx_bytes"], m["workspace_bytes"]


def _replaced_flow(env, form, value, base):
    """what is wrong with mav_last_flow_dev's answer after a form that computes flow (None: nothing): the place and the field are the
    intervener's, not the producer's"""
    which, own = form.flow
    ptr, got = value
    if own and ptr != env.out(3):
        return f"reports {ptr:#x}, the intervener's flow went to {env.out(3):#x}" + (" (still the producer's buffer)" if ptr == base[0] else "")
    if not own and (not ptr or ptr in {b.ptr for b in env.d.values()}):
        return f"reports {ptr}, a caller's block or none, for a flow that went to a block of the context's"
    want = env.alt_flow[which].tobytes()
    if got != want:
        return f"the field behind it is not the intervener's flow ({_first_diff(got, want)})" + (": it is the producer's" if got == base[1] else "")
    return None


def _judge(env, seq, form, readers, base, fails):
    """every reader after the sequence so far, against the form's class for the reader's kind"""
    dropped = False
    for name in readers:
        kind = rc.READERS[name][1]
        klass = form.klass(kind)
        code, outs, value = _read(env, name)
        where = f"{seq}, {name}"
        if kind == "flow" and klass != "keeps":      # no error state: the reader answers for the newest flow call (resident_cases' head)
            dropped = dropped or klass == "drops"
            wrong = _replaced_flow(env, form, value, base[name])
            if wrong:
                fails.append(f"{where}: class {klass}, mav_last_flow_dev {wrong}")
        elif klass == "replaces":
            if code != rc.OK:
                fails.append(f"{where}: the intervener leaves {kind} itself, the reader returned {code}")
        elif code == rc.OK and value != base[name]:
            fails.append(f"{where}: silently different -- class {klass}, MAV_OK with other bytes ({_first_diff(value, base[name])})")
        elif klass == "keeps" and code != rc.OK:
            fails.append(f"{where}: class keeps, the reader returned {code}")
        elif klass == "drops":
            dropped = True
            if code != rc.ERR_STATE:
                fails.append(f"{where}: class drops, the reader returned {code} instead of MAV_ERR_STATE")
            elif not all(rc.untouched(a) for a in outs):
                fails.append(f"{where}: a refused reader wrote into its outputs")
    return dropped


def _run_form(env, P, pname, form, readers, base, fails):
    try:
        _sequences(env, P, pname, form, readers, base, fails)
    except Exception as e:
        hip = rc.hip_failure(e)                  # a producer, ctx.sync() or a copy reports MAV_ERR_HIP / MAV_ERR_OOM by raising
        if hip is not None:
            raise rc.HipFailure(f"{pname}, {form.name}: {hip}") from e
        # any other: a form that cannot even be called is a failure of its own, not the end of the others
        fails.append(f"{pname}, {form.name}: {type(e).__name__}: {e}")


def _sequences(env, P, pname, form, readers, base, fails):
    mem = []
    for rep in ("first", "second"):
        P.run(env)
        got = _checked(form.run(env), form.name)
        want = rc.OK if form.refused is None else form.refused
        if got != want:
            fails.append(f"{pname}, {form.name}: returned {got}, expected {want}")
            return
        dropped = _judge(env, f"{pname}, {form.name}", form, readers, base, fails)
        if dropped and rep == "first":           # a following producer plus reader gives the baseline again
            P.run(env)
            for name in readers:
                code, _, value = _read(env, name)
                if code != rc.OK or value != base[name]:
                    fails.append(f"{pname}, {form.name}, {pname}, {name}: {code}, not the baseline again")
        mem.append(_mem(env))
    if mem[1] != mem[0]:
        fails.append(f"{pname}, {form.name}: the second identical sequence grew the context {mem[0]} -> {mem[1]}")
    # the intervener between two readers of the same producer
    P.run(env)
    code, _, value = _read(env, readers[0])
    if code != rc.OK or value != base[readers[0]]:
        fails.append(f"{pname}, {readers[0]}: {code}, not the baseline")
    if _checked(form.run(env), form.name) != (rc.OK if form.refused is None else form.refused):
        fails.append(f"{pname}, {readers[0]}, {form.name}: not the code of the first time")
    _judge(env, f"{pname}, {readers[0]}, {form.name}", form, readers, base, fails)


def _baseline(env, ref, P, pname, readers):
    x = env.x
    info = P.run(env)
    if isinstance(info.get("flow"), str) or "flow" in P.leaves:
        flow = np.array(ref.farneback(x["prev"], x["next"]))
        if not isinstance(info["flow"], str):
            assert info["flow"].tobytes() == flow.tobytes(), f"{pname}: its flow is not mav_farneback's"
        info["flow"] = flow
    if isinstance(info.get("Hm"), str):
        Hm, ok = ref.flow_homography(info["flow"], x["coords"])
        info["Hm"] = Hm
    base = {}
    for name in readers:
        code, _, value = _read(env, name)
        assert code == rc.OK, (pname, name, code)
        base[name] = value
    want = rc.direct(ref, x, info, P.leaves)
    for name in readers:
        assert base[name] == want[name], f"{pname}, {name}: the baseline is not the direct call's ({_first_diff(base[name], want[name])})"
    for name in readers:                         # ... and it survives its own readers
        code, _, value = _read(env, name)
        assert code == rc.OK and value == base[name], (pname, name, "read twice")
    return base


@pytest.mark.parametrize("group", list(rc.GROUPS))
@pytest.mark.parametrize("producer", list(rc.PRODUCERS))
def test_readers_after_every_call_between(mav, ref, alt_flows, producer, group):
    from mavflow import _lib
    P, readers = rc.PRODUCERS[producer], rc.readers_of(producer)
    forms = [f for i, f in enumerate(rc.FORMS) if rc.GROUPS[group](i)]
    fails = []
    with _lib.Context(W, H, B) as ctx:
        env = rc.Env(ctx)
        env.alt_flow = alt_flows
        try:
            try:
                base = _baseline(env, ref, P, producer, readers)
            except Exception as e:
                raise rc.hip_failure(e) or e
            for form in forms:
                _run_form(env, P, producer, form, readers, base, fails)
        except rc.HipFailure as e:               # the exit condition: nothing more runs on this context
            fails.append(f"stopped: {e}")
        finally:
            env.close()
    assert not fails, f"{len(fails)} sequence(s):\n" + "\n".join(fails)
