"""numpy restatement of the pose assessor's rule (include/rbsensor_mi355x.h, rbs_assess_*): owner,
class, counts and verdict from per-body depth planes and a frame.  binary64 with + - x and comparisons and integer counts:
it takes every decision of the device kernels bit for bit."""
import numpy as np

OUT_OF_VIEW, OCCLUDED, SUPPORTED, LOST = range(4)
DEFAULTS = dict(sigmas=3.0, min_support_fraction=0.5, min_visible_fraction=0.25, min_pixels=16)


def owners(planes):
    """planes [B, npx] float32 (+inf: not covered) -> owner [npx] (the nearest body, ties to the lowest; -1: none) and its depth."""
    planes = np.asarray(planes, dtype=np.float32)
    B, npx = planes.shape
    best = np.full(npx, np.inf, dtype=np.float32)
    owner = np.full(npx, -1, dtype=np.int64)
    for b in range(B):
        take = planes[b] < best            # strictly nearer than every lower body: a tie stays with the lowest
        best = np.where(take, planes[b], best)
        owner = np.where(take, b, owner)
    return owner, best


def counts(planes, frame, model_sigma, sigma_factor, sigmas=3.0):
    """-> [B, 5] int32: rendered, valid, support, in_front, behind."""
    planes = np.asarray(planes, dtype=np.float32)
    B = planes.shape[0]
    y = np.asarray(frame, dtype=np.float32).reshape(-1)
    owner, best = owners(planes)
    out = np.zeros((B, 5), dtype=np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        d = best.astype(np.float64)
        r = y.astype(np.float64) - d
        tau = np.float64(sigmas) * (np.float64(model_sigma) + np.float64(sigma_factor) * (d * d))
        finite = np.isfinite(y)
        front = r < -tau
        behind = r > tau
    for b in range(B):
        own = owner == b
        val = own & finite
        out[b] = (own.sum(), val.sum(), (val & ~front & ~behind).sum(), (val & front).sum(), (val & behind).sum())
    return out


def verdict(c, sigmas=3.0, min_support_fraction=0.5, min_visible_fraction=0.25, min_pixels=16):
    """One record's five counts -> verdict."""
    rendered, _valid, support, _front, behind = (int(v) for v in c[:5])
    u = support + behind
    if rendered < int(min_pixels):
        return OUT_OF_VIEW
    if float(u) < float(min_visible_fraction) * float(rendered):
        return OCCLUDED
    if float(support) >= float(min_support_fraction) * float(u):
        return SUPPORTED
    return LOST


def assess(planes, frame, model_sigma, sigma_factor, **params):
    """-> (counts [B, 5], verdicts [B])."""
    p = dict(DEFAULTS, **params)
    c = counts(planes, frame, model_sigma, sigma_factor, p["sigmas"])
    return c, np.array([verdict(row, **p) for row in c], dtype=np.int32)
