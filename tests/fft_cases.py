"""The case table of a 2-D Fourier transform and of the reference's log-magnitude spectrum (im_helpers.get_fft): shapes, seeds, inputs
and the lengths a mixed-radix transform with prime factors up to 31 and a limit of 4096 refuses.  The device form is not in the
library yet; this table, tests/fft_ref.py and the golden files are what it will be held to.

Inputs are seeded, so the golden files (tests/golden/fft*.npz, written by tools/gen_golden_fft.py from the reference's own get_fft and
from scipy.fft.fft2 in longdouble) store results only.  The shapes are the smallest at which each form of such a transform can go
wrong: every radix 2, 3, 4, 5, 7, the primes 11 .. 31, odd and even lengths and length 1 on both axes.

CONDITIONS on every uint8 input, asserted by the generator and again by tests/test_fft_ref_cpu.py from the stored truth: no bin with
|F_true| = 0, and no bin whose 20 ln|F_true| lies within INTEGER_MARGIN of an integer -- so that the truncation to uint8 is decided by
the mathematics and EVERY pixel of every case is compared.  Seed 7 satisfies both on the first eight shapes (the smallest distance is
1.4e-5, at 31 x 62); for the others the generator was asked for the first seed from 7 on that does."""
from collections import namedtuple

import numpy as np

INTEGER_MARGIN = 1e-6

# name, H, W, seeds: one uint8 frame per seed (more than one: a batch)
Case = namedtuple("Case", "name H W seeds")

CASES = (
    Case("18x30", 18, 30, (7,)),              # radix 2, 3, 5 on both axes
    Case("45x77", 45, 77, (7,)),              # odd on both axes: 3 3 5 and 7 11 (the generic butterfly on the rows)
    Case("26x34", 26, 34, (7,)),              # 2 13 and 2 17: the generic butterfly behind a radix-2 pass
    Case("31x62", 31, 62, (7,)),              # the largest prime served, alone (columns) and behind radix 2 (rows)
    Case("64x64", 64, 64, (7,)),              # radix 4 alone, three passes
    Case("1x8", 1, 8, (7,)),                  # height 1: the column pass is the identity
    Case("7x1", 7, 1, (7,)),                  # width 1: the row pass is the identity, one column that is its own mirror
    Case("135x240", 135, 240, (7,)),          # an eighth of 1080p: 4 4 3 5 rows, 3 3 3 5 columns, more than one column tile
    Case("58x221", 58, 221, (7,)),            # 13 17 rows, 2 29 columns: two generic passes in one transform
    Case("4x1920", 4, 1920, (7,)),            # the real frame width, a handful of rows
    Case("1080x6", 1080, 6, (7,)),            # the real frame height, a handful of columns: the column tile sized by H
    Case("27x125", 27, 125, (7,)),            # repeated odd radices 3 3 3 and 5 5 5
    Case("49x121", 49, 121, (7,)),            # 7 7 and 11 11: the generic butterfly twice
    Case("batch3_45x77", 45, 77, (8, 9, 10)), # a batch of three different frames
)
BY_NAME = {c.name: c for c in CASES}
FLOAT_CASES = tuple(c for c in CASES if len(c.seeds) == 1)      # a float32 and a float64 normal field per shape
DFT_MATRIX_MAX = 64                                             # tests/fft_ref.py's O(n^2) transform runs on shapes up to 64 x 64

# (H, W, the text the refusal must contain)
REFUSED = (
    (37, 8, "height 37 has the prime factor 37"),
    (8, 74, "width 74 has the prime factor 37"),
    (8, 2 * 4099, "width 8198 has the prime factor 4099"),
    (4374, 8, "height 4374 is above the limit of 4096"),       # 2 * 3^7: every factor is served, the length is not
)


def frame_u8(seed: int, H: int, W: int) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), np.uint8)


def frame_float(seed: int, H: int, W: int, dtype) -> np.ndarray:
    """a normal field (H, W, 3); float32 and float64 draw from different streams"""
    return np.random.default_rng(seed + (1000 if np.dtype(dtype) == np.float32 else 2000)).normal(size=(H, W, 3)).astype(dtype)


def frames_u8(case: Case) -> np.ndarray:
    """(batch, H, W, 3)"""
    return np.stack([frame_u8(s, case.H, case.W) for s in case.seeds])


def factorisation(n: int):
    """(prime factors of n with multiplicity, ascending); [] for 1"""
    out, d = [], 2
    while d * d <= n:
        while n % d == 0:
            out.append(d)
            n //= d
        d += 1
    if n > 1:
        out.append(n)
    return out


def supported(n: int, limit: int = 4096, max_factor: int = 31) -> bool:
    return 1 <= n <= limit and all(p <= max_factor for p in factorisation(n))
