"""tests/resident_cases.py against include/mavflow.h and csrc/mavflow.cpp as text: every entry point of the header has a place in the
table -- producer, reader, intervener or exempt, exactly one -- and the classes the table states are those the source's own markers
give (HostCall::fresh drops, HostCall::after_last reads).  An entry point added without a word on what it does to resident state
fails here, without a GPU."""
import re

import resident_cases as rc


def _header():
    with open(rc.HEADER) as f:
        return rc.header_functions(f.read())


def _roles(names=None):
    """function -> the set of roles the table gives it"""
    producers = {e for p in rc.PRODUCERS.values() for e in p.entries}
    readers = {e for e, _, _ in rc.READERS.values()}
    forms = set(rc.intervener_entries())
    roles = {}
    for n in set(names or ()) | producers | readers | forms | set(rc.EXEMPT):
        r = set()
        if n in producers:
            r.add("producer")
        if n in readers:
            r.add("reader")
        if n in rc.EXEMPT:
            r.add("exempt")
        if n in forms and n not in producers:        # (a producer's own forms, accepted and refused, run between other producers too)
            r.add("intervener")
        roles[n] = r
    return roles


def _unplaced(names):
    roles = _roles(names)
    return sorted(n for n in names if len(roles[n]) != 1), sorted(n for n in roles if n not in names)


def test_every_entry_point_of_the_header_has_exactly_one_place():
    names = _header()
    assert len(names) == len(set(names)) and len(names) > 150
    wrong, unknown = _unplaced(names)
    assert not wrong, f"neither producer, reader, intervener nor exempt (or more than one): {wrong}"
    assert not unknown, f"in the table but not in the header: {unknown}"


def test_a_new_prototype_or_a_missing_intervener_is_noticed():
    names = _header()
    wrong, _ = _unplaced(names + ["mav_something_new_dev"])
    assert wrong == ["mav_something_new_dev"]
    forms = rc.FORMS
    try:
        rc.FORMS = [f for f in forms if f.entry != "mav_ransac"]
        wrong, _ = _unplaced(names)
    finally:
        rc.FORMS = forms
    assert wrong == ["mav_ransac"]


def test_producers_readers_and_classes_cover_each_other():
    kinds_left = {k for p in rc.PRODUCERS.values() for k in p.leaves}
    kinds_read = {k for _, k, _ in rc.READERS.values()}
    assert kinds_left == kinds_read == set(rc.KINDS)
    for name in rc.PRODUCERS:
        assert rc.readers_of(name), name
    names = [f.name for f in rc.FORMS]
    assert len(names) == len(set(names))
    by_name = {f.name: f for f in rc.FORMS}
    assert rc.FRESH_BEFORE_REFUSAL <= set(names) and rc.ENQUEUED_BEFORE_REFUSAL <= set(names)
    assert not rc.FRESH_BEFORE_REFUSAL & rc.ENQUEUED_BEFORE_REFUSAL
    for kind in rc.KINDS:
        got = {(f.klass(kind), f.refused is not None) for f in rc.FORMS}
        assert ("keeps", False) in got and ("drops", False) in got and ("keeps", True) in got, (kind, got)
    for f in rc.FORMS:
        assert f.rule in rc.RULES and (f.refused is None or f.refused in (rc.ERR_ARG, rc.ERR_STATE)), f.name
        if f.refused is not None and f.name not in rc.FRESH_BEFORE_REFUSAL | rc.ENQUEUED_BEFORE_REFUSAL:
            assert all(f.klass(k) == "keeps" for k in rc.KINDS), f.name
        # a form says which flow it computes exactly when mav_last_flow_dev answers for it afterwards
        assert (f.flow is not None) == (f.klass("flow") != "keeps"), f.name
        assert f.flow is None or (f.flow[0] in ("plain", "init") and f.flow[1] in (rc.OWN, rc.CTX)), f.name
    for n in rc.FRESH_BEFORE_REFUSAL:            # the named exceptions are refusals, of host-pointer calls / of the frame step
        assert by_name[n].refused is not None and by_name[n].rule in ("fresh", "fresh+flow"), n
        assert {k for k in rc.KINDS if by_name[n].klass(k) == "drops"} == rc.RULES["fresh"], n
    for n in rc.ENQUEUED_BEFORE_REFUSAL:
        assert by_name[n].refused is not None and by_name[n].entry == "mav_frame_step_dev", n
        assert {k for k in rc.KINDS if by_name[n].klass(k) == "drops"} == rc.RULES["flow"], n
    groups = [sum(1 for i in range(len(rc.FORMS)) if sel(i)) for sel in rc.GROUPS.values()]
    assert sum(groups) == len(rc.FORMS)


def test_a_hip_error_raised_by_the_bindings_is_the_exit_condition():
    """the producers, ctx.sync() and the copies report MAV_ERR_HIP / MAV_ERR_OOM by raising (mavflow._lib.check): both end a context's
    sequences like the return code does; a refusal, MAV_ERR_STATE or a mistake of the test's does not"""
    from mavflow import _lib
    for e in (_lib.MavflowError(f"[{rc.ERR_HIP}] hipErrorIllegalAddress"), _lib.MavflowError(f"[{rc.ERR_OOM}] x"), MemoryError("x"), rc.HipFailure("x")):
        assert isinstance(rc.hip_failure(e), rc.HipFailure), e
    for e in (_lib.MavflowError(f"[{rc.ERR_STATE}] nothing resident"), ValueError("n_pairs"), AssertionError("x"), KeyError("x")):
        assert rc.hip_failure(e) is None, e
    assert (rc.ERR_HIP, rc.ERR_OOM, rc.ERR_STATE) == (_lib.MAV_ERR_HIP, _lib.MAV_ERR_OOM, _lib.MAV_ERR_STATE)


def _bodies(src):
    """name -> body of every extern "C" function and of every static helper"""
    out = {}
    for m in re.finditer(r'(?:extern "C" [^;{}()]*?\b(mav_\w+)|static int (\w+))\s*\(', src):
        name = m.group(1) or m.group(2)
        close = src.index(")", m.end())
        i = close + 1
        while src[i] in " \n":
            i += 1
        if src[i] != "{":                            # a declaration
            continue
        depth, j = 0, i
        while True:
            depth += {"{": 1, "}": -1}.get(src[j], 0)
            j += 1
            if depth == 0:
                break
        out[name] = src[i:j]
    return out


def test_the_classes_are_those_the_source_marks():
    with open(rc.SOURCE) as f:
        bodies = _bodies(f.read())
    helpers = [n for n in bodies if not n.startswith("mav_") and "HostCall h(" in bodies[n]]      # process_host, stage_blur_resize ...
    assert {"process_host", "phi_mask_host", "foe_dense_host", "farneback_host", "components_host"} <= set(helpers)
    readers = {e for e, _, _ in rc.READERS.values()}
    by_entry = {}
    for f in rc.FORMS:
        for e in (f.entry,) + tuple(rc.ALSO.get(f.name, ())):
            by_entry.setdefault(e, []).append(f)
    seen_fresh = seen_reader = 0
    for name in _header():
        body = bodies.get(name)
        if body is None or name in rc.EXEMPT:
            continue
        text = body + "".join(bodies[h] for h in helpers if re.search(rf"\b{h}\(", body))
        fresh, after = bool(re.search(r"\.fresh(_layer)?\(", text)), ".after_last(" in text
        if fresh and after:                          # components_host: its `resident` argument chooses, and only mav_last_* pass one
            fresh, after = not name.startswith("mav_last_"), name.startswith("mav_last_")
        assert after == (name in readers and name != "mav_last_flow_dev"), f"{name}: HostCall::after_last and the READERS table disagree"
        seen_reader += after
        if fresh:
            seen_fresh += 1
            for f in by_entry.get(name, []):
                if f.refused is None:
                    assert f.rule in ("fresh", "fresh+flow"), f"{f.name}: its source calls HostCall::fresh, the table says {f.rule!r}"
                    for kind in rc.RULES["fresh"]:
                        assert f.klass(kind) in ("drops", "replaces"), (f.name, kind)
            assert name in by_entry or name in {e for p in rc.PRODUCERS.values() for e in p.entries}, name
        else:
            for f in by_entry.get(name, []):
                assert f.rule not in ("fresh", "fresh+flow"), f"{f.name}: the table says HostCall::fresh, its source has none"
    assert seen_fresh >= 40 and seen_reader == 8, (seen_fresh, seen_reader)      # (the scan found the markers at all)
