"""The cases of tests/test_gpu_schedule_pin.py and how one of them is recorded (shared with tools/gen_schedule_pin.py, which
writes tests/golden/schedule_pin.json).

A record is what the host scheduler of one `farneback` call did, seen through the library's own profile: the `mav_schedule_info`
string, and the (kernel class, stream) of every launch in host enqueue order, run-length encoded.  Frame content does not steer
the schedule; the frames are the synthetic ones the other tests use.
"""
import ctypes as C

import numpy as np

# (name, (W, H), levels, max_batch, group or None, options in the order they are set, call)
# call: "pairs" = farneback(prev, next) of max_batch pairs; "sequence" = farneback_sequence of max_batch + 1 frames;
#       "initial_flow" = farneback(prev, next, initial_flow=...); "uint16" = farneback of uint16 frames
HD, DEEP3, DEEP4 = ((1920, 1080), 1, 5, 2), ((1920, 1080), 3, 5, 2), ((1000, 562), 4, 7, 3)


def _cases():
    out = [("1080p-default", *HD, [], "pairs")]
    for b in (1, 2, 3):                                                     # one stream: whole M, then band-major
        out.append((f"1080p-one-stream-bands{b}", *HD, [("pairs_in_flight", 1), ("bands", b)], "pairs"))
    for s in (0, 1):                                                        # sub-groups of two, no bands
        out.append((f"1080p-one-stream-share_m{s}-fine2", *HD, [("pairs_in_flight", 1), ("share_m", s), ("group_fine", 2)], "pairs"))
    out.append(("1080p-coarse_half1", *HD, [("coarse_half", 1)], "pairs"))  # coarse sub-group sizing
    out.append(("1080p-coarse_cache0", *HD, [("coarse_cache_mb", 0)], "pairs"))
    out.append(("1080p-coarse_half1-coarse_cache0", *HD, [("coarse_half", 1), ("coarse_cache_mb", 0)], "pairs"))
    for deep in (0, 1):                                                     # deep layers, banded coarse layer
        for cb in (0, 1):
            out.append((f"1080p-3-levels-deep{deep}-coarse_bands{cb}", *DEEP3, [("band_mb", 8), ("deep_batch", deep), ("coarse_bands", cb)], "pairs"))
    banded = [("band_mb", 8), ("deep_batch", 1), ("coarse_bands", 1)]       # shifted partition, equal bands
    out.append(("1080p-3-levels-band_phase1", *DEEP3, banded + [("band_phase", 1)], "pairs"))
    out.append(("1080p-3-levels-band_skew0", *DEEP3, banded + [("band_skew", 0)], "pairs"))
    out.append(("1080p-3-levels-band_phase1-band_skew0", *DEEP3, banded + [("band_phase", 1), ("band_skew", 0)], "pairs"))
    out.append(("1000x562-4-levels-deep_frac32", *DEEP4, [("band_mb", 8), ("deep_frac", 32)], "pairs"))
    out.append(("642x480-default", (642, 480), 1, 3, 3, [("band_mb", 8)], "pairs"))        # width % 4 != 0: bands not possible
    out.append(("642x480-bands2", (642, 480), 1, 3, 3, [("band_mb", 8), ("bands", 2)], "pairs"))
    out.append(("58x174-default", (58, 174), 1, 3, 3, [], "pairs"))         # relaxed sweep form, fewer tile rows than a band needs
    for sb in (0, 1):                                                       # small-group pyramid, merged frames
        out.append((f"720p-one-pair-small_batch{sb}", (1280, 720), 1, 1, None, [("small_batch", sb)], "pairs"))
        out.append((f"720p-sequence-small_batch{sb}", (1280, 720), 1, 2, None, [("small_batch", sb)], "sequence"))
    for deep in (0, 1):                                                     # exact initial M at the top layer
        out.append((f"640x480-initial-flow-deep{deep}", (640, 480), 1, 5, 2, [("deep_batch", deep)], "initial_flow"))
    out.append(("640x480-uint16", (640, 480), 1, 2, 2, [], "uint16"))       # depth template path
    return out


CASES = _cases()
NAMES = [c[0] for c in CASES]


def expects_second_stream(case) -> bool:
    """Every case uses the second compute stream except those that ask for one stream or hold a single pair."""
    _, _, _, batch, _, options, _ = case
    return dict(options).get("pairs_in_flight", 2) == 2 and batch > 1


def _rle(classes, streams):
    runs = []
    for k, s in zip(classes, streams):
        if runs and runs[-1][0] == k and runs[-1][1] == s:
            runs[-1][2] += 1
        else:
            runs.append([k, s, 1])
    return runs


_frames = {}


def _batch(W, H, n):
    from mavflow import synth
    if (W, H) not in _frames:
        _frames[(W, H)] = synth.make_pair(W, H, 0)[:2]
    f0, f1 = _frames[(W, H)]
    return np.stack([f0] * n), np.stack([f1] * n)


def record(case) -> dict:
    """Run one case on the GPU -> {"info": the schedule string, "launches": [[class name, stream, count], ...]}."""
    from mavflow import _lib, synth
    name, (W, H), levels, batch, group, options, call = case
    prev, nxt = _batch(W, H, batch)
    dtype = np.uint8
    if call == "uint16":
        dtype = np.uint16
        prev, nxt = prev.astype(np.uint16) * 257, nxt.astype(np.uint16) * 257
    with _lib.Context(W, H, batch, _lib.fb_defaults(levels=levels)) as c:
        if group is not None:
            c.set_option("group", group)
        for key, value in options:
            c.set_option(key, value)
        buf = C.create_string_buffer(8192)
        if dtype == np.uint8:
            _lib.check(c.lib.mav_schedule_info(c.h, batch, buf, len(buf)))
        else:
            _lib.check(c.lib.mav_schedule_info_ex(c.h, batch, _lib.DEPTHS[np.dtype(dtype)], buf, len(buf)))
        c.profile_enable(1)
        if call == "sequence":
            c.farneback_sequence(synth.make_sequence(W, H, batch + 1))
        elif call == "initial_flow":
            c.farneback(prev, nxt, initial_flow=np.stack([synth.synthetic_flow(W, H, 1)] * batch))
        else:
            c.farneback(prev, nxt)
        kid, stream, _, _ = c.profile_intervals()
        class_names = list(c.profile_get())
        c.profile_enable(0)
    return {"info": buf.value.decode(), "launches": _rle([class_names[k] for k in kid], [int(s) for s in stream])}
