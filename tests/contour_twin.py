"""numpy restatement of the contour rule (include/rbsensor_mi355x.h, rbs_contour_*): rim, anchor,
class, counts and verdict from per-body depth planes and a frame.  Owners are assess_twin's; the window maximum is taken
by shifted maxima over a -inf-padded image.  binary64 with + - x, comparisons, a float maximum and integer counts: it
takes every decision of the device kernel bit for bit."""
import numpy as np

import assess_twin as tw

NO_RIM, UNDECIDED, PRESENT, ABSENT = range(4)
DEFAULTS = dict(radius=2, min_rim_pixels=16, min_valid_fraction=0.5, min_contour_fraction=0.3, min_flush_fraction=0.5)


def anchors(planes, rows, cols, radius):
    """planes [B, rows*cols] float32 -> (covered [rows, cols] bool, a [B, rows, cols] float32: the maximum of depth(j) over
    the pixels j owned by b in the Chebyshev window of `radius` clipped to the image, -inf where there is none)."""
    planes = np.asarray(planes, dtype=np.float32)
    B = planes.shape[0]
    owner, best = tw.owners(planes)
    owner, best = owner.reshape(rows, cols), best.reshape(rows, cols)
    r = int(radius)
    out = np.full((B, rows, cols), -np.inf, dtype=np.float32)
    for b in range(B):
        pad = np.full((rows + 2 * r, cols + 2 * r), -np.inf, dtype=np.float32)
        pad[r:r + rows, r:r + cols] = np.where(owner == b, best, np.float32(-np.inf))
        wide = np.full((rows + 2 * r, cols), -np.inf, dtype=np.float32)
        for dx in range(2 * r + 1):              # a window maximum is separable and exact: columns, then rows
            wide = np.maximum(wide, pad[:, dx:dx + cols])
        for dy in range(2 * r + 1):
            out[b] = np.maximum(out[b], wide[dy:dy + rows])
    return owner >= 0, out


def counts(planes, frame, rows, cols, model_sigma, sigma_factor, sigmas=3.0, radius=2):
    """-> [B, 5] int32: rim, valid, flush, in_front, beyond."""
    planes = np.asarray(planes, dtype=np.float32)
    B = planes.shape[0]
    y = np.asarray(frame, dtype=np.float32).reshape(rows, cols)
    covered, a = anchors(planes, rows, cols, radius)
    out = np.zeros((B, 5), dtype=np.int32)
    finite = np.isfinite(y)
    for b in range(B):
        rim = ~covered & (a[b] > -np.inf)
        with np.errstate(invalid="ignore", over="ignore"):
            d = a[b].astype(np.float64)
            g = y.astype(np.float64) - d
            tau = np.float64(sigmas) * (np.float64(model_sigma) + np.float64(sigma_factor) * (d * d))
            front = g < -tau
            beyond = g > tau
        val = rim & finite
        out[b] = (rim.sum(), val.sum(), (val & ~front & ~beyond).sum(), (val & front).sum(), (val & beyond).sum())
    return out


def verdict(c, radius=2, min_rim_pixels=16, min_valid_fraction=0.5, min_contour_fraction=0.3, min_flush_fraction=0.5):
    """One record's five counts -> verdict."""
    rim, valid, flush, _front, beyond = (int(v) for v in c[:5])
    if rim < int(min_rim_pixels):
        return NO_RIM
    if valid == 0 or float(valid) < float(min_valid_fraction) * float(rim):
        return UNDECIDED
    if float(beyond) >= float(min_contour_fraction) * float(valid):
        return PRESENT
    if float(flush) >= float(min_flush_fraction) * float(valid):
        return ABSENT
    return UNDECIDED


def contour(planes, frame, rows, cols, model_sigma, sigma_factor, sigmas=3.0, **params):
    """-> (counts [B, 5], verdicts [B])."""
    p = dict(DEFAULTS, **params)
    c = counts(planes, frame, rows, cols, model_sigma, sigma_factor, sigmas, p["radius"])
    return c, np.array([verdict(row, **p) for row in c], dtype=np.int32)
