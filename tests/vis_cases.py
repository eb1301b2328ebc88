"""TEST INFRASTRUCTURE -- the case table of the flow pictures (include/mavflow_vis.h, csrc/kernels_vis.hip): the frames, the batches, the
pointer offsets and, for every case, the form of the pixel passes (mav_vis_form) it must reach, with what the form then has to handle (a
tail of single pixels behind the last group of 16; a group that straddles two images).  tests/test_vis_cases_cpu.py holds the table to
the library's mav_vis_form and fails when a form or a feature is reached by no case; tests/test_gpu_vis.py runs the device on every
case.  The fields of the tests are made here too, once per shape."""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

FORM_BYTES, FORM_FAST = 0, 1                     # MAV_VIS_FORM_*
GROUP = 16                                       # pixels of one thread in the FAST form
B = 3                                            # max_batch of every context here; calls run at batch 1 and 3
FRAMES = ((131, 67), (66, 33), (17, 5), (1, 1), (128, 8))          # (W, H)
BATCHES = (1, 3)
OFFSETS = (0, 1)                                 # bytes added to the BGR and HSV pointers of the enqueue forms
HUE_MARGIN = 5e-4                                # a hue this close to a whole number may fall either way (atan2f is the device's)

Case = namedtuple("Case", "W H batch offset form tail straddles")


def form_of(W: int, H: int, batch: int, *pointers) -> int:
    """mav_vis_form in Python: FAST when the call has at least 16 pixels and every non-NULL pointer is aligned to 16"""
    if W * H * batch < GROUP:
        return FORM_BYTES
    return FORM_BYTES if any(p is not None and p % 16 for p in pointers) else FORM_FAST


def _case(W, H, batch, offset) -> Case:
    n0, N = W * H, W * H * batch
    form = form_of(W, H, batch, 0, offset, offset)
    fast = form == FORM_FAST
    return Case(W, H, batch, offset, form, N % GROUP if fast else N, fast and batch > 1 and n0 % GROUP != 0)


CASES = [_case(W, H, b, o) for (W, H) in FRAMES for b in BATCHES for o in OFFSETS]
# what the table must reach: both forms; in the FAST form a call with no tail, one with a tail, one whose groups straddle images and
# one with more than one workgroup of 256 threads; in the BYTES form a call of one pixel and one of more than a workgroup
FEATURES = {
    "fast": lambda c: c.form == FORM_FAST,
    "bytes": lambda c: c.form == FORM_BYTES,
    "fast without a tail": lambda c: c.form == FORM_FAST and c.tail == 0,
    "fast with a tail": lambda c: c.form == FORM_FAST and c.tail > 0,
    "fast, a group in two images": lambda c: c.straddles,
    "fast, several workgroups": lambda c: c.form == FORM_FAST and c.W * c.H * c.batch // GROUP > 256,
    "bytes, one pixel": lambda c: c.form == FORM_BYTES and c.W * c.H * c.batch == 1,
    "bytes, too few pixels for a group": lambda c: c.offset == 0 and c.form == FORM_BYTES,
    "bytes, several workgroups, several images": lambda c: c.form == FORM_BYTES and c.batch > 1 and c.W * c.H > 256,
}


def case_id(c: Case) -> str:
    return f"{c.W}x{c.H}-b{c.batch}-off{c.offset}"


@functools.lru_cache(maxsize=None)
def constructed_fields(W: int, H: int, batch: int = B) -> np.ndarray:
    """(batch, H, W, 2) float32: angles (k + 0.5 +- 0.4) * 2 degrees with k uniform in 0 .. 179 -- so that trunc(angle / 2 degrees) is k
    whatever the last bits of atan2f are -- and magnitudes uniform in 0.1 .. 20.  Read-only."""
    rng = np.random.default_rng(W * 1000 + H)
    k = rng.integers(0, 180, (batch, H, W))
    deg = (k + 0.5 + rng.uniform(-0.4, 0.4, (batch, H, W))) * 2.0
    mag = rng.uniform(0.1, 20.0, (batch, H, W))
    f = np.stack([mag * np.cos(np.deg2rad(deg)), mag * np.sin(np.deg2rad(deg))], -1).astype(np.float32)
    f.setflags(write=False)
    return f


def load_fixture(path: str) -> dict:
    """tests/golden/vis.npz as a dict; the fields, stored as the float16 values they were made from, widened to float32 (exactly)"""
    with np.load(path, allow_pickle=False) as z:
        out = {k: z[k] for k in z.files}
    for k in out:
        if k.startswith("flow_"):
            assert out[k].dtype == np.float16
            out[k] = out[k].astype(np.float32)
    return out


def in_band(hue: np.ndarray, margin: float = HUE_MARGIN) -> np.ndarray:
    """the pixels whose hue (before it is cut) lies within `margin` of a whole number"""
    return np.abs(hue - np.rint(hue)) < margin


def lattice() -> np.ndarray:
    """(n, 3) uint8: every triple of the stride-3 lattice 0, 3, .., 255 (255 = 3 * 85 is on it): 86^3 = 636 056 triples"""
    v = np.arange(0, 256, 3)
    assert v[-1] == 255
    return np.stack(np.meshgrid(v, v, v, indexing="ij"), -1).reshape(-1, 3).astype(np.uint8)


def as_frames(triples: np.ndarray, W: int, H: int) -> np.ndarray:
    """(n, 3) triples -> (ceil(n / (W H)), H, W, 3), padded with zeros"""
    n0 = W * H
    nb = -(-len(triples) // n0)
    out = np.zeros((nb * n0, 3), np.uint8)
    out[:len(triples)] = triples
    return out.reshape(nb, H, W, 3)
