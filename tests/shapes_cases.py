"""The case table of the shapes tests (include/mavflow_shapes.h): frames, tables of records, the forms each case must reach and the
geometric band every thick line has to meet.  tests/test_shapes_cases_cpu.py holds the table to its own conditions without a GPU;
tests/test_gpu_shapes.py runs every case on the device against tests/shapes_ref.py."""
import os
import re
from collections import namedtuple

import numpy as np

import shapes_ref as R

FRAMES = ((131, 67), (66, 33))                    # W x H: odd, no multiple of 16 or 64 in either; more than one workgroup of rows
B = 3
THICKNESSES = (1, 2, 3, 4, 5, 6, 7, 255)
GREEN, RED, BLUE, WHITE = (0, 255, 0), (0, 0, 255), (255, 0, 0), (255, 255, 255)
FILL = 0xA5

Case = namedtuple("Case", "name W H shapes channels")


def octant_lines(W, H, t, image=0, colour=GREEN):
    """axis-aligned, diagonal, shallow and steep lines in all eight octants around the middle of the frame"""
    cx, cy, r = W // 2, H // 2, min(W, H) // 2 - 3
    ends = [(r, 0), (-r, 0), (0, r), (0, -r), (r, r), (-r, r), (r, -r), (-r, -r),
            (r, r // 5), (r, -(r // 5)), (-r, r // 5), (-r, -(r // 5)), (r // 5, r), (-(r // 5), r), (r // 5, -r), (-(r // 5), -r),
            (r, r // 2), (-(r // 2), -r)]
    return [R.shape(R.LINE, image, cx, cy, cx + dx, cy + dy, t, colour) for dx, dy in ends]


def border_lines(W, H, t, image=0, colour=RED):
    """lines crossing each of the four borders and each corner, wholly outside, zero-length (inside, on the edge, outside), longer than
    the frame"""
    return [R.shape(R.LINE, image, *p, t, colour) for p in (
        (W // 2, 5, W // 3, -9), (W // 2, H - 6, W // 2 + 7, H + 11), (6, H // 2, -12, H // 2 + 5), (W - 5, H // 3, W + 14, H // 3 - 4),
        (4, 3, -6, -5), (W - 4, 4, W + 5, -7), (5, H - 4, -8, H + 6), (W - 6, H - 5, W + 9, H + 4),
        (-30, -20, -5, -40), (W + 10, 3, W + 40, H - 3), (3, H + 300, W - 3, H + 320), (-400, H // 2, -300, H // 2),
        (W // 4, H // 4, W // 4, H // 4), (0, 0, 0, 0), (W - 1, H - 1, W - 1, H - 1), (-2, H // 2, -2, H // 2), (W + 500, 3, W + 500, 3),
        (-3 * W, -2 * H, 4 * W, 3 * H), (-2 * W, H // 2 + 3, 3 * W, H // 2 - 2), (W // 3, -5 * H, W // 3 + 4, 6 * H))]


def rectangles(W, H, image=0):
    out = []
    for t, col in ((1, GREEN), (2, RED), (3, BLUE), (5, WHITE), (R.FILLED, (9, 200, 77))):
        out += [R.shape(R.RECT, image, 7, 5, W - 20, H - 12, t, col), R.shape(R.RECT, image, W - 30, H - 9, 12, 8, t, col),
                R.shape(R.RECT, image, -6, -4, 9, 7, t, col), R.shape(R.RECT, image, W - 5, H - 6, W + 30, H + 12, t, col),
                R.shape(R.RECT, image, W // 2, H // 2, W // 2, H // 2, t, col), R.shape(R.RECT, image, W + 4, 2, W + 9, 8, t, col)]
    return out


def circles(W, H, image=0):
    return [R.shape(R.CIRCLE, image, x, y, r, 0, R.FILLED, c) for x, y, r, c in (
        (W // 2, H // 2, 20, RED), (3, 2, 10, GREEN), (W - 2, H - 3, 7, BLUE), (W // 3, H // 3, 0, WHITE), (W // 4, H - 8, 1, RED),
        (-40, -40, 30, GREEN), (W // 2, H // 2, 3 * W, (1, 2, 3)), (W - 9, 9, 2, WHITE))] + (
        # a radius of hundreds of thousands whose rim crosses the frame's top rows: a row's span is no walk from the start
        [R.shape(R.CIRCLE, image, W // 2, 300000 + 9, 300000, 0, R.FILLED, (77, 66, 55))] if image == 0 else [])


def heavy_overlap(W, H, n=2000, seed=5, image=0):
    """FoE.draw's workload: n lines of thickness 2 in two colours with heavy overlap"""
    rng = np.random.RandomState(seed)
    p = rng.randint(-10, [W + 10, H + 10], (n, 2))
    q = p + rng.randint(-25, 26, (n, 2))
    col = rng.randint(0, 2, n)
    return [R.shape(R.LINE, image, p[i, 0], p[i, 1], q[i, 0], q[i, 1], 2, GREEN if col[i] else RED) for i in range(n)]


def skipped_records(W, H):
    """every kind of skipped record (batch = B), each next to valid records that must still be drawn"""
    big = R.MAX_COORD + 1
    bad = [R.shape(7, 0, 1, 1, 20, 20, 2, RED), R.shape(-1, 0, 1, 1, 20, 20, 2, RED),
           R.shape(R.LINE, -1, 1, 1, 20, 20, 2, RED), R.shape(R.LINE, B, 1, 1, 20, 20, 2, RED), R.shape(R.LINE, 1 << 30, 1, 1, 20, 20, 2, RED),
           R.shape(R.LINE, 0, 1, 1, 20, 20, 0, RED), R.shape(R.LINE, 0, 1, 1, 20, 20, 256, RED), R.shape(R.LINE, 0, 1, 1, 20, 20, -1, RED),
           R.shape(R.RECT, 0, 1, 1, 20, 20, -2, RED), R.shape(R.RECT, 0, 1, 1, 20, 20, 0, RED), R.shape(R.RECT, 0, 1, 1, 20, 20, 1 << 20, RED),
           R.shape(R.CIRCLE, 0, 10, 10, 5, 0, 2, RED), R.shape(R.CIRCLE, 0, 10, 10, -1, 0, R.FILLED, RED),
           R.shape(R.LINE, 0, big, 1, 20, 20, 2, RED), R.shape(R.LINE, 0, 1, -big, 20, 20, 2, RED), R.shape(R.LINE, 0, 1, 1, big, 20, 2, RED),
           R.shape(R.LINE, 0, 1, 1, 20, -(1 << 31), 2, RED), R.shape(R.CIRCLE, 0, 10, 10, 5, big, R.FILLED, RED),
           R.shape(R.RECT, 2, (1 << 31) - 1, 1, 20, 20, R.FILLED, RED)]
    good = [R.shape(R.LINE, 0, 2, 3, W - 4, H - 5, 3, GREEN), R.shape(R.RECT, 2, 4, 4, W // 2, H // 2, 2, BLUE),
            R.shape(R.CIRCLE, 0, W // 2, H // 2, 6, 0, R.FILLED, WHITE), R.shape(R.LINE, 0, 3000, -3000, -3000, 3000, 4, GREEN)]
    # the largest coordinates a record may have: a filled box over all of image 2, under everything drawn later.  (A thick LINE that
    # long is drawn too, but its 16.16 edge slopes drift by pixels over 2^20 rows, as OpenCV's do: the band is not a condition on it.)
    out = [R.shape(R.RECT, 2, -R.MAX_COORD, R.MAX_COORD, R.MAX_COORD, -R.MAX_COORD, R.FILLED, (3, 4, 5)),
           R.shape(R.LINE, 2, -R.MAX_COORD, 7, R.MAX_COORD, 7, 1, WHITE)]
    for i, b in enumerate(bad):
        out += [b, good[i % len(good)]]
    return out, len(bad)


def cases():
    out = []
    for W, H in FRAMES:
        for t in THICKNESSES:
            ch = 1 if t in (2, 6) else 3
            out.append(Case(f"octants-t{t}", W, H, R.table(octant_lines(W, H, t) + octant_lines(W, H, t, image=2, colour=BLUE)), ch))
            out.append(Case(f"borders-t{t}", W, H, R.table(border_lines(W, H, t) + border_lines(W, H, t, image=2)), ch))
        out.append(Case("rectangles", W, H, R.table(rectangles(W, H) + rectangles(W, H, image=2)), 3))
        out.append(Case("rectangles-gray", W, H, R.table(rectangles(W, H)), 1))
        out.append(Case("circles", W, H, R.table(circles(W, H) + circles(W, H, image=2)), 3))
        out.append(Case("mixed", W, H, R.table(octant_lines(W, H, 3) + rectangles(W, H, image=2) + circles(W, H) + border_lines(W, H, 2, image=2)), 3))
        for ch in (3, 1):                                              # one colour: the table the direct form may take
            out.append(Case("one-colour", W, H, R.table(octant_lines(W, H, 3) + border_lines(W, H, 2, image=2, colour=GREEN) + [
                R.shape(R.RECT, 0, 9, 6, W - 11, H - 8, 2, GREEN), R.shape(R.CIRCLE, 2, W // 2, H // 2, 9, 0, R.FILLED, GREEN)]), ch))
        out.append(Case("skipped", W, H, R.table(skipped_records(W, H)[0]), 3))
    W, H = FRAMES[0]
    out.append(Case("heavy-overlap", W, H, R.table(heavy_overlap(W, H) + heavy_overlap(W, H, 300, seed=9, image=2)), 3))
    return out


CASES = cases()


# ---- past the caps of the launches (outside CASES: the tests over every case do not grow) -------------------------------------------------
KERNELS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mav-detection_amd", "csrc", "kernels_shapes.hip")
RESOLVE_FRAME = (701, 499)      # x B = 1 049 397 elements = 4096 * 256 + 821: k_shapes_resolve's second trip is the last 821 pixels of image 2
ROWS_RECORDS = 8300             # k_shapes_rows: one workgroup per record up to 8192 workgroups; records 8192 .. 8299 on the second trip
ROWS_N_DEV = 8250               # a device count below n_max, both past the cap


def source_caps(text=None) -> dict:
    """SH_WG and the caps draw_shapes_launch gives sh_grid, read from kernels_shapes.hip as text"""
    if text is None:
        with open(KERNELS) as f:
            text = f.read()
    return dict(wg=int(re.search(r"^#define SH_WG (\d+)\b", text, re.M).group(1)),
                rows=int(re.search(r"rows_grid = sh_grid\(\(size_t\)n_max \* 4 \* 64, (\d+)\);", text).group(1)),
                resolve=int(re.search(r"k_shapes_resolve, dim3\(sh_grid\(N, (\d+)\)\)", text).group(1)), text=text)


def stride_forms(items: int, cap: int, per_group: int) -> set:
    """a loop `for (i = first; i < items; i += gridDim.x * per_group)` under sh_grid's min(ceil(items / per_group), cap) workgroups: the
    trips the first worker takes, and whether the last one leaves workers without an item"""
    g = min((items + per_group - 1) // per_group, cap) or 1
    T = g * per_group
    trips = (items + T - 1) // T
    if trips <= 1:
        return {"1"}
    return {">1"} | ({">1:partial-last"} if items % T else set())


def resolve_forms(W, H, batch, c=None) -> set:
    c = c or source_caps()
    return stride_forms(W * H * batch, c["resolve"], c["wg"])


def rows_forms(n_max, c=None) -> set:
    """(record, part) items, four per record, one wave each: a workgroup of SH_WG / 64 = 4 waves takes one record per trip"""
    c = c or source_caps()
    return stride_forms(4 * n_max, c["rows"], c["wg"] // 64)


def resolve_cap_table(W, H):
    """about 80 records over the three images; in the last rows of image 2 (the pixels past the cap) a filled rectangle under lines of
    other colours and a circle, then lines over those: order decides pixels there"""
    out = []
    for image in range(B):
        q = heavy_overlap(W, H, n=20, seed=20 + image, image=image)
        q += [R.shape(R.LINE, image, 5 + 97 * image, 3, W - 9, H - 7 - 50 * image, 3 + image, (RED, GREEN, WHITE)[image])]     # across the frame
        out += q
    out += [R.shape(R.RECT, 2, 40, H - 12, W - 30, H + 5, R.FILLED, (9, 200, 77)),
            R.shape(R.LINE, 2, 60, H - 2, W - 170, H - 1, 3, GREEN),                    # shallow, along the last two rows
            R.shape(R.LINE, 2, W - 200, H - 40, W - 20, H + 10, 2, RED),
            R.shape(R.CIRCLE, 2, W - 60, H - 3, 9, 0, R.FILLED, BLUE),
            R.shape(R.LINE, 2, W - 90, H - 1, W - 30, H - 1, 1, WHITE),
            R.shape(R.RECT, 2, W - 150, H - 6, W - 100, H + 3, 2, RED),
            R.shape(R.LINE, 2, W - 115, H - 30, W - 108, H + 20, 5, BLUE),               # steep, through the rectangle's outline
            R.shape(R.RECT, 0, 40, H - 12, W - 30, H + 5, R.FILLED, (9, 200, 77)),       # the same rows of image 0: before the cap
            R.shape(R.LINE, 0, 10, H - 2, W - 10, H - 1, 3, GREEN)]
    for k in range(12):                                                                  # a fan of lines down through the last rows
        out.append(R.shape(R.LINE, 2, W - 20 - 9 * k, H - 25 - k, W - 60 - 3 * k, H + 4, 1 + k % 4, (GREEN, RED, BLUE, WHITE)[k % 4]))
    out.append(R.shape(R.CIRCLE, 2, W - 3, H - 1, 4, 0, R.FILLED, (1, 2, 3)))             # the last pixel of the plane, under a circle
    return R.table(out)


def rows_cap_table(W, H, green=False):
    """heavy_overlap's lines, ROWS_RECORDS of them; green: all of one colour, the table the direct form may take"""
    t = R.table(heavy_overlap(W, H, n=ROWS_RECORDS))
    if green:
        t["colour"][:, :3] = GREEN
    return t


def case_id(c):
    return f"{c.name}-{c.W}x{c.H}-c{c.channels}"


def uses_image_1(c):
    return bool(np.any(c.shapes["image"][[R.valid(s, B) for s in c.shapes]] == 1))


def one_colour(shapes, channels):
    """what mav_shapes_form must say DIRECT for"""
    return len(shapes) == 0 or bool(np.all(shapes["colour"][:, :channels] == shapes["colour"][0, :channels]))


def canary(W, H, channels, seed=3):
    """the image every case is drawn into: (B, H, W, channels) of bytes no colour of the table has"""
    return np.random.RandomState(seed).randint(16, 64, (B, H, W, channels)).astype(np.uint8)


# ---- the geometric band of a thick line ----------------------------------------------------------------------------------------------------
def segment_distance(W, H, x0, y0, x1, y1) -> np.ndarray:
    """(H, W) float64: distance of every pixel centre to the segment"""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    dx, dy = float(x1 - x0), float(y1 - y0)
    L2 = dx * dx + dy * dy
    u = np.zeros_like(xx) if L2 == 0 else np.clip(((xx - x0) * dx + (yy - y0) * dy) / L2, 0.0, 1.0)
    return np.hypot(xx - (x0 + u * dx), yy - (y0 + u * dy))


def band_of(s, W, H):
    """(must, may_not) of a LINE or RECT-outline record of thickness t: every pixel within t / 2 - 1 of a segment must be drawn (t >= 3),
    none farther than t / 2 + 1.5 from all of them may be"""
    t = int(s["thickness"])
    x0, y0, x1, y1 = (int(s[k]) for k in ("x0", "y0", "x1", "y1"))
    segs = [(x0, y0, x1, y1)] if int(s["kind"]) == R.LINE else [(x0, y1, x0, y0), (x0, y0, x1, y0), (x1, y0, x1, y1), (x1, y1, x0, y1)]
    d = np.minimum.reduce([segment_distance(W, H, *g) for g in segs])
    must = d <= t / 2 - 1 if t >= 3 else np.zeros((H, W), bool)
    return must, d > t / 2 + 1.5


def banded_records(c):
    """the records of a case the band applies to: valid lines and rectangle outlines"""
    return [s for s in c.shapes if R.valid(s, B) and int(s["kind"]) in (R.LINE, R.RECT) and int(s["thickness"]) >= 1]


# ---- add and mosaic ---------------------------------------------------------------------------------------------------------------------
AddCase = namedtuple("AddCase", "name W H channels batch offset")           # offset: bytes behind a 16-aligned address
ADD_CASES = [AddCase("words", 131, 67, 3, B, 0), AddCase("bytes-unaligned", 131, 67, 3, B, 1), AddCase("gray-words", 66, 33, 1, B, 0),
             AddCase("gray-unaligned", 66, 33, 1, 1, 7), AddCase("tiny", 5, 1, 1, 1, 0), AddCase("four-channels", 66, 33, 4, 2, 0)]
MosaicCase = namedtuple("MosaicCase", "name W H rows cols channels batch offset")     # channels: per tile, 0 = NULL
MOSAIC_CASES = [MosaicCase("debug-frame", 131, 67, 2, 3, (3, 3, 3, 3, 1, 3), B, 0), MosaicCase("unaligned", 131, 67, 2, 3, (3, 1, 0, 3, 1, 3), B, 3),
                MosaicCase("small", 66, 33, 2, 3, (1, 3, 3, 0, 3, 1), 1, 0), MosaicCase("one-tile", 66, 33, 1, 1, (1,), 2, 0),
                MosaicCase("row", 66, 33, 1, 4, (3, 0, 1, 3), B, 5)]


def bytes_form_of(n, *offsets):
    """MAV_SHAPES_FORM_WORDS (1) / _BYTES (0) for a call of n bytes whose pointers lie these offsets behind 16-aligned addresses"""
    return int(n >= 16 and all(o % 16 == 0 for o in offsets))


def add_inputs(c, seed=11):
    rng = np.random.RandomState(seed)
    shape = (c.batch, c.H, c.W, c.channels)
    a, b = rng.randint(0, 256, shape).astype(np.uint8), rng.randint(0, 256, shape).astype(np.uint8)
    b.reshape(-1)[::5] = 0                                             # a mask is mostly black
    a.reshape(-1)[:4] = (255, 255, 0, 1)
    b.reshape(-1)[:4] = (255, 1, 0, 254)                               # the saturation's edges
    return a, b


def mosaic_inputs(c, seed=13):
    rng = np.random.RandomState(seed)
    return [None if ch == 0 else rng.randint(0, 256, (c.batch, c.H, c.W, ch)).astype(np.uint8) for ch in c.channels]
