"""numpy restatement of the finder's silhouette gate (include/rbsensor_mi355x.h, step 4b and what it changes in steps 5 and
7; rbsensor_find_gate.hip).  The evidence composes assess_twin and contour_twin at B = 1 and adds nothing else; the orders
are find_twin's total order with the class in front."""
import numpy as np

import assess_twin as at
import contour_twin as ct
import find_twin as ft

DEFAULTS = dict(radius=2, min_rim_pixels=16, min_pixels=16, sigmas=3.0, min_support_fraction=0.5, min_visible_fraction=0.25,
                min_valid_fraction=0.5, min_contour_fraction=0.3, min_flush_fraction=0.5)
ASSESS_KEYS = ("sigmas", "min_support_fraction", "min_visible_fraction", "min_pixels")
CONTOUR_KEYS = ("radius", "min_rim_pixels", "min_valid_fraction", "min_contour_fraction", "min_flush_fraction")


def class_of(record, **params):
    """The ten counts -> 0 (the verdicts are SUPPORTED and PRESENT: confirmed) or 1."""
    p = dict(DEFAULTS, **params)
    a = at.verdict(record[:5], **{k: p[k] for k in ASSESS_KEYS})
    c = ct.verdict(record[5:10], **{k: p[k] for k in CONTOUR_KEYS})
    return 0 if a == at.SUPPORTED and c == ct.PRESENT else 1


def evidence(plane, frame, rows, cols, model_sigma, sigma_factor, **params):
    """One pose's depth plane [rows*cols] float32 (+inf: not covered) and the frame -> (record [10] int32, class)."""
    p = dict(DEFAULTS, **params)
    planes = np.asarray(plane, dtype=np.float32).reshape(1, rows * cols)
    rec = np.concatenate([at.counts(planes, frame, model_sigma, sigma_factor, p["sigmas"])[0],
                          ct.counts(planes, frame, rows, cols, model_sigma, sigma_factor, p["sigmas"], p["radius"])[0]]).astype(np.int32)
    return rec, class_of(rec, **p)


def gated_topk(scores, classes, k, index=None):
    """Step 5 with the gate on: the k first of (class ascending, score descending, index ascending), NaN never, as
    (scores [m], indices [m]), m <= k the entries with a number."""
    scores = np.asarray(scores, dtype=np.float64)
    classes = np.asarray(classes)
    index = np.arange(len(scores), dtype=np.int64) if index is None else np.asarray(index, dtype=np.int64)
    out_s, out_i = [], []
    for c in (0, 1):
        pick = np.nonzero((classes == c) & ~np.isnan(scores))[0]
        s, i = ft.topk(scores[pick], index[pick])
        out_s.append(s)
        out_i.append(i)
    return np.concatenate(out_s)[:k], np.concatenate(out_i)[:k]


def result_order(scores, classes):
    """Step 7 with the gate on: survivor positions in the order (a number before NaN, class ascending, score descending,
    survivor index ascending); the NaN scores last in survivor order."""
    scores = np.asarray(scores, dtype=np.float64)
    classes = np.asarray(classes)
    k = np.arange(len(scores))
    nan = np.isnan(scores)
    with np.errstate(invalid="ignore"):
        return np.lexsort((k, -np.where(nan, 0.0, scores), np.where(nan, 0, classes), nan))


def found(scores, classes, order, min_score, require_confirmed):
    """rbs_find_run's `found` from the final order."""
    if len(order) == 0:
        return False
    s, c = scores[order[0]], classes[order[0]]
    ok = bool(s >= min_score)
    return ok and c == 0 if require_confirmed else ok
