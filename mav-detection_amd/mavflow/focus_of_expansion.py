"""FocusOfExpansion -- the dense FoE fit and the per-pixel radial residual on libmavflow, behind the reference's
call signatures (/root/reference/src/focus_of_expansion.py:13-184), and the sparse fit on the device tracker.

RNG ownership: get_FOE_dense draws its 2N sample coordinates from the global legacy numpy stream exactly as the
reference does (rows first, then columns, :70-71) and the constructor consumes the same draws (:24,26), so a seeded
run visits the same pixels.  The GPU never generates samples."""
from __future__ import annotations

from typing import List, Tuple

import numpy as np

from . import _lib, im_helpers


class FocusOfExpansion:
    def __init__(self, lucas_kanade) -> None:
        """`lucas_kanade`: any object with .total_num_corners and .old_frame (H, W[, 3]) -- see detector.LucasKanade."""
        self.lucas_kanade = lucas_kanade
        self.time = 0
        self.roll_back = 20
        self.num_features = 0
        self.enable_plots = False
        self.max_flow = 0.0                       # maximum phi in the image (degrees)
        self.radial_threshold = np.cos(np.deg2rad(15))
        self.magnitude_threshold = 2.5
        self.ransac_threshold = 30.0              # pixels
        n = int(lucas_kanade.total_num_corners)
        self.color = np.random.randint(0, 255, (n, 3))
        self.trace = np.zeros((n, 2000), dtype=np.int32)
        self.random_lines = np.random.randint(0, n, n)
        self.flow_height, self.flow_width = lucas_kanade.old_frame.shape[0], lucas_kanade.old_frame.shape[1]

    def _ctx(self, flow: np.ndarray) -> "_lib.Context":
        H, W = flow.shape[:2]
        return im_helpers._ctx(W, H)

    def _foe_params(self, n_pairs: int = 1000) -> "_lib.FoeParams":
        p = _lib.foe_defaults()
        p.n_pairs = n_pairs
        p.mag_threshold = float(self.magnitude_threshold)
        p.ransac_threshold = float(self.ransac_threshold)
        return p

    def ransac(self, estimates: np.ndarray) -> Tuple[float, float]:
        """First estimate with the strictly largest number of others within ransac_threshold; (0.0, 0.0) if none has any."""
        return im_helpers._ctx(self.flow_width, self.flow_height).ransac(estimates, self.ransac_threshold)

    def get_FOE_dense(self, flow_uv: np.ndarray) -> Tuple[float, float]:
        """FoE from N = 1000 random flow-line intersections + the RANSAC vote.  The arithmetic follows the array's dtype as
        numpy's does: a float32 field (frame index 0, which derotate hands back untouched) has its |flow2| gate evaluated in
        float32, a float64 field in double."""
        N = 1000
        rand1 = np.zeros((N * 2, 2), dtype=np.uint32)
        rand1[..., 0] = np.random.randint(0, flow_uv.shape[0], N * 2)
        rand1[..., 1] = np.random.randint(0, flow_uv.shape[1], N * 2)
        foe = self._ctx(flow_uv).foe_dense(flow_uv, rand1, self._foe_params(N))[0]
        return (float(foe[0]), float(foe[1]))

    def get_FOE_sparse(self, old_frame: np.ndarray, new_frame: np.ndarray) -> Tuple[float, float]:
        """FoE from sparse optical flow (:88-148): the tracker's features (lucas_kanade.get_features: corners and tracking on the
        device) extend per-feature traces; a trace of two or more points gives a line from its newest point back over up to
        roll_back steps, each line is intersected with one drawn at random (one np.random.randint per line, in the reference's
        order), and the device RANSAC vote picks the FoE.  The trace bookkeeping is the reference's host code, a few thousand scalars
        per frame -- including the line end's wrap through uint16 and the halving loop that tests the y coordinate against the frame
        WIDTH.  One departure: where the reference's halving loop would never end (a trace point with a negative y wraps to > 65000
        for every diff), it stops once diff has reached zero."""
        from . import utils
        if np.sum(old_frame) < 1:
            return (np.nan, np.nan)

        old_features, new_features, status = self.lucas_kanade.get_features(new_frame)
        self.mask = np.zeros_like(old_frame)
        self.lines = []
        intersections = np.zeros((len(new_features), 2))

        def as_uint16(v):            # ndarray.astype(np.uint16) of a float64 pair as x86 numpy does it: truncate, then wrap
            return (np.trunc(v).astype(np.int64) & 0xFFFF).astype(np.uint16)

        for i, (new, old) in enumerate(zip(new_features, old_features)):
            if status[i] != 1:
                continue
            a, b, c, d = [int(x) for x in [*new.ravel(), *old.ravel()]]
            l = self.trace[i, 0] + 1
            self.trace[i, l] = c
            self.trace[i, l + 1] = d
            self.trace[i, 0] += 2
            self.num_features += 1

            if l >= 3:
                k = 1 if l < 1 + self.roll_back * 2 else l - self.roll_back * 2
                a, b = self.trace[i, l:l + 2]
                c, d = self.trace[i, k:k + 2]
                diff = np.array([float(c) - float(a), float(d) - float(b)])
                new_xy = as_uint16(np.array([a, b]) + diff)
                # "Let flow vector fit inside image bounds" -- the reference's test, as it is
                while new_xy[1] < 0.0 or new_xy[1] > new_frame.shape[1]:
                    if not diff.any():
                        break
                    diff /= 2.0
                    new_xy = as_uint16(np.array([a, b]) + diff)
                self.lines.append(((a, b), (new_xy[0], new_xy[1])))

        with np.errstate(over="ignore"):     # the lines' end points are int32 / uint16 scalars, as in the reference: products may wrap
            for i, line_a in enumerate(self.lines):
                line_b = self.lines[np.random.randint(0, len(self.lines))]
                intersections[i, :] = utils.line_intersection(line_a, line_b)

        intersections = intersections[intersections[:, 0] != 0.0, :]
        return self.ransac(intersections)

    def get_phi(self, derotated_flow_uv: np.ndarray, FoE: Tuple[float, float]) -> np.ndarray:
        """Angle (degrees) between each flow vector and the ray from the FoE through its pixel; max goes to .max_flow.
        float32 flow in -> float32 arithmetic and float32 phi out (zeros_like in the reference), float64 otherwise."""
        if FoE[0] is np.nan:                      # identity test, as the reference (:160)
            return np.zeros(0)
        phi, _, _, mx = self._ctx(derotated_flow_uv).phi_mask(derotated_flow_uv, FoE)
        self.max_flow = mx[0]
        return phi[0]

    def get_masks(self, derotated_flow_uv: np.ndarray, FoE: Tuple[float, float], sky_mask=None, params=None):
        """The threshold block of processor.py:333-341 -> (estimate_fixed, total_mask); phi is not materialised."""
        _, fixed, total, _ = self._ctx(derotated_flow_uv).phi_mask(derotated_flow_uv, FoE, sky=sky_mask, params=params, want_phi=False)
        return fixed[0], total[0]

    def draw_FoE(self, frame: np.ndarray, FoE: Tuple[float, float], color: List[int] = [0, 42, 255], radius: int = 10) -> np.ndarray:
        """Draw the FoE as a filled disc, in place, and return the frame (:186-201): cv2.circle(frame, (int(x), int(y)), radius, color,
        -1) -- OpenCV's integer midpoint spans (disc_half_widths), clipped to the image.  Nothing is drawn when |x| or |y| > 1e9 or a
        coordinate IS the np.nan object; any other NaN raises ValueError, as int() does.  The kernel of Context.overlay draws the
        same spans."""
        if FoE[0] is np.nan or FoE[1] is np.nan or np.abs(FoE[0]) > 1e9 or np.abs(FoE[1]) > 1e9:
            return frame
        cx, cy = int(FoE[0]), int(FoE[1])
        H, W = frame.shape[:2]
        value = color[0] if frame.ndim == 2 else list(color)[:frame.shape[2]]
        for k, h in enumerate(disc_half_widths(radius)):
            for y in {cy - k, cy + k}:
                x0, x1 = max(cx - h, 0), min(cx + h, W - 1)
                if 0 <= y < H and x0 <= x1:
                    frame[y, x0:x1 + 1] = value
        return frame

    @staticmethod
    def line_colours(lines, FoE, radial_threshold) -> List[List[int]]:
        """The colour of every tracked line as draw (:218-236) decides it, in the reference's own arithmetic on the host: the cosine
        between the line and the ray from the FoE to its newest point, green [0, 255, 0] unless it is below radial_threshold, then red
        [0, 0, 255].  A zero-length line or a point on the FoE gives the quotient 0 / 0 = NaN, and `nan < t` is false: green."""
        out = []
        with np.errstate(all="ignore"):
            for line in lines:
                diff1 = np.asarray(line[0]) - np.asarray(line[1])
                diff2 = np.asarray(line[0]) - np.asarray(FoE)
                flow_magnitude = im_helpers.get_magnitude(diff1)
                img_distance = im_helpers.get_magnitude(diff2)
                angle_diff = np.dot(diff1, diff2) / (flow_magnitude * img_distance)
                out.append([0, 0, 255] if angle_diff < radial_threshold else [0, 255, 0])
        return out

    def draw(self, frame: np.ndarray, FoE: Tuple[float, float]) -> np.ndarray:
        """Draw the FoE algorithm's visualisation (:203-241): a filled disc of radius 20 at the FoE into `frame` (in place), every line
        of the latest get_FOE_sparse into self.mask with thickness 2, green or red by line_colours, in the lines' order, and
        cv2.add(frame, self.mask) as the result.  The disc, the lines and the add are one call of the shapes family each (the lines as
        ONE table, drawn in table order); the colours are a few thousand scalars on the host, like the trace bookkeeping.  old_gray and
        time are updated as the reference updates them."""
        from . import shapes
        if FoE[0] is np.nan:
            return frame
        ctx = im_helpers._ctx(frame.shape[1], frame.shape[0])
        ctx.draw_shapes(frame, [shapes.shape(shapes.CIRCLE, int(FoE[0]), int(FoE[1]), 20, 0, shapes.FILLED, [0, 42, 255])])
        frame_gray = ctx.bgr2gray(frame)
        frame_gray = frame_gray[0] if frame_gray.ndim == 3 else frame_gray
        colours = self.line_colours(self.lines, FoE, self.radial_threshold)
        table = [shapes.shape(shapes.LINE, int(l[0][0]), int(l[0][1]), int(l[1][0]), int(l[1][1]), 2, c) for l, c in zip(self.lines, colours)]
        if table:
            ctx.draw_shapes(self.mask, table)
        self.old_gray = frame_gray.copy()
        self.time += 1
        return ctx.add_saturate(frame, self.mask)


def disc_half_widths(radius: int) -> List[int]:
    """Half-width of each row offset 0..radius of cv2.circle(thickness=-1, LINE_8, shift 0): OpenCV's Circle(..., fill=1) emits the
    spans [cx +- dx] on rows cy +- dy and [cx +- dy] on rows cy +- dx of its integer midpoint walk; a row is its widest span.  Radius 10:
    10 9 9 9 9 8 8 7 6 4 0.  Restated from the published routine: no image the reference wrote pins it."""
    r = int(radius)
    if r < 0:
        raise ValueError(f"radius {radius} < 0")
    h = [-1] * (r + 1)
    err, dx, dy, plus, minus = 0, r, 0, 1, 2 * r - 1
    while dx >= dy:
        h[dy] = max(h[dy], dx)
        h[dx] = max(h[dx], dy)
        dy += 1
        err += plus
        plus += 2
        if err > 0:
            err -= minus
            dx -= 1
            minus -= 2
    return h
