"""The sparse optical-flow calls of the reference's lucas_kanade.py with cv2's literal signatures on libmavflow's HIP path, as
mavflow.farneback holds cv2.calcOpticalFlowFarneback's: a cv2 argument list passes as it is.

    from mavflow.lucas_kanade import LucasKanade, calcOpticalFlowPyrLK, goodFeaturesToTrack

calcOpticalFlowPyrLK always computes `err`, as cv2 does when it is called from Python, and with it runs cv2's final bounds test: a
point whose last position leaves the bounds ends with status 0.  LucasKanade (detector.LucasKanade, re-exported here under the
reference's module name) still tracks through Context.lk_track, the call without `err`, so its status differs from cv2's Python call
at exactly those points; calcOpticalFlowPyrLK below is the call that follows cv2."""
from __future__ import annotations

import numpy as np

from . import _lib
from .detector import LucasKanade  # noqa: F401  (the reference's class under the reference's module name)

OPTFLOW_USE_INITIAL_FLOW = _lib.OPTFLOW_USE_INITIAL_FLOW
OPTFLOW_LK_GET_MIN_EIGENVALS = _lib.OPTFLOW_LK_GET_MIN_EIGENVALS

_CTX_CACHE_SIZES = 4                 # contexts kept per frame size, least recently used first
_ctx_cache = {}                      # (W, H) -> Context


def _context(W: int, H: int):
    ctx = _ctx_cache.pop((W, H), None)
    if ctx is None or not ctx.alive:
        ctx = _lib.Context(W, H, 1)
    _ctx_cache[(W, H)] = ctx
    while len(_ctx_cache) > _CTX_CACHE_SIZES:
        _ctx_cache.pop(next(iter(_ctx_cache)))
    return ctx


def _gray(img, name: str) -> np.ndarray:
    img = np.asarray(img)
    if img.ndim != 2 or img.dtype != np.uint8:
        raise ValueError(f"{name}: expected a single-channel uint8 image, got {img.dtype} {img.shape}")
    return img


def _points(pts, name: str):
    """cv2's point vectors: (n, 1, 2) or (n, 2) float32 -> ((n, 2) float32, the shape to give back)"""
    pts = np.asarray(pts)
    if pts.dtype != np.float32 or pts.ndim not in (2, 3) or pts.shape[-1] != 2 or (pts.ndim == 3 and pts.shape[1] != 1):
        raise ValueError(f"{name}: expected float32 points of shape (n, 1, 2) or (n, 2), got {pts.dtype} {pts.shape}")
    return pts.reshape(-1, 2), pts.shape


def calcOpticalFlowPyrLK(prevImg, nextImg, prevPts, nextPts, status=None, err=None, winSize=(21, 21), maxLevel=3, criteria=(3, 30, 0.01),
                         flags=0, minEigThreshold=1e-4):
    """cv2.calcOpticalFlowPyrLK's literal signature (8-bit single-channel frames) -> (nextPts, status, err) in cv2's shapes for the
    input's: (n, 1, 2) points give (n, 1, 2) / (n, 1) / (n, 1), (n, 2) points give (n, 2) / (n, 1) / (n, 1).  New arrays: the `nextPts`,
    `status` and `err` arguments are not written.  flags: 0, OPTFLOW_USE_INITIAL_FLOW (4: `nextPts` holds the starting positions),
    OPTFLOW_LK_GET_MIN_EIGENVALS (8: err is the minimum eigenvalue) or both.  criteria: (type, count, epsilon) as cv2.TermCriteria."""
    prev, nxt = _gray(prevImg, "prevImg"), _gray(nextImg, "nextImg")
    if prev.shape != nxt.shape:
        raise ValueError("prevImg and nextImg must be of one size")
    pts, shape = _points(prevPts, "prevPts")
    init = None
    if int(flags) & OPTFLOW_USE_INITIAL_FLOW:
        if nextPts is None:
            raise ValueError("OPTFLOW_USE_INITIAL_FLOW needs the starting positions in `nextPts`")
        init, ishape = _points(nextPts, "nextPts")
        if len(init) != len(pts):
            raise ValueError(f"nextPts holds {len(init)} points, prevPts {len(pts)}")
    H, W = prev.shape
    out, st, e = _context(W, H).lk_track_err(prev, nxt, pts, next_pts=init, flags=int(flags), winSize=tuple(winSize), maxLevel=int(maxLevel),
                                             criteria=tuple(criteria), minEigThreshold=float(minEigThreshold))
    return out.reshape(shape), st.reshape(-1, 1), e.reshape(-1, 1)


def goodFeaturesToTrack(image, maxCorners, qualityLevel, minDistance, mask=None, blockSize=3, useHarrisDetector=False, k=0.04,
                        gradientSize=3):
    """cv2.goodFeaturesToTrack's literal signature (8-bit single-channel image; cv2's own default blockSize of 3) -> (n, 1, 2) float32
    corners, or None when no corner is found, as cv2 returns it.  The Sobel aperture is 3: any other gradientSize is a ValueError.
    maxCorners <= 0 means no limit in cv2; here it is the point buffer's size."""
    if int(gradientSize) != 3:
        raise ValueError(f"gradientSize {gradientSize}: only the 3 x 3 Sobel aperture is built")
    img = _gray(image, "image")
    H, W = img.shape
    mc = int(maxCorners) if int(maxCorners) > 0 else _lib.LK_MAX_POINTS
    corners = _context(W, H).good_features(img, mask=mask, useHarrisDetector=bool(useHarrisDetector), k=float(k), maxCorners=mc,
                                           qualityLevel=float(qualityLevel), minDistance=float(minDistance), blockSize=int(blockSize))
    return corners.reshape(-1, 1, 2) if len(corners) else None
