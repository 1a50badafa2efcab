"""numpy twin of the object finder's step 1b, the foreground (include/rbsensor_mi355x.h; rbs_findfg_*_kernel in
dbot_ros_amd/csrc/rbsensor_find.hip): the dominant inverse-depth plane of the coarse frame from three-point trials, and the
seeding frame.  Binary64, only + - * / and comparisons, in the header's order: every decision is the device's, bit for bit.
The draws are find_twin.philox's."""
import numpy as np

import find_twin as tw

RECORD = 8          # accepted, a, b, c, count, n_valid, trial, pixels masked
NAN32 = np.float32(np.nan)


def sigma(z, model_sigma, sigma_factor):
    return model_sigma + sigma_factor * (z * z)


def valid(frame, dmin, dmax):
    d = np.asarray(frame, dtype=np.float32).ravel().astype(np.float64)
    with np.errstate(invalid="ignore"):
        return (d >= dmin) & (d <= dmax)


def trial_pixels(seed, t, npx):
    """The three coarse pixels of trial t: words 0..2 of Philox4x32-10 (key seed, counter words (t, 0, 0, 0xFFFFFFFF))."""
    w = tw.philox(seed, 0xFFFFFFFF << 32, t)
    return [(int(w[k]) * npx) >> 32 for k in range(3)]


def plane_through(px, frame, cols, dmin, dmax):
    """(a, b, c, void) of the plane through the pixels px = (i0, i1, i2) of the coarse frame (flat float32)."""
    f = np.asarray(frame, dtype=np.float32).ravel()
    u = [np.float64(i % cols) for i in px]
    v = [np.float64(i // cols) for i in px]
    d = [np.float64(f[i]) for i in px]
    ok = all(bool(x >= dmin) and bool(x <= dmax) for x in d)
    D = (u[1] - u[0]) * (v[2] - v[0]) - (u[2] - u[0]) * (v[1] - v[0])
    if not ok or D == 0.0:
        return 0.0, 0.0, 0.0, 1.0
    one = np.float64(1.0)
    q0, q1, q2 = one / d[0], one / d[1], one / d[2]
    a = ((q1 - q0) * (v[2] - v[0]) - (q2 - q0) * (v[1] - v[0])) / D
    b = ((u[1] - u[0]) * (q2 - q0) - (u[2] - u[0]) * (q1 - q0)) / D
    c = (q0 - a * u[0]) - b * v[0]
    return float(a), float(b), float(c), 0.0


def trials(frame, rows, cols, dmin, dmax, seed, n_trials):
    """-> planes [n_trials][4] = (a, b, c, void); a void trial is (0, 0, 0, 1)."""
    out = np.zeros((n_trials, 4))
    with np.errstate(all="ignore"):
        for t in range(n_trials):
            out[t] = plane_through(trial_pixels(seed, t, rows * cols), frame, cols, dmin, dmax)
    return out


def _w(a, b, c, rows, cols):
    p = np.arange(rows * cols)
    u, v = (p % cols).astype(np.float64), (p // cols).astype(np.float64)
    return (a * u + b * v) + c


def counts(frame, rows, cols, dmin, dmax, model_sigma, sigma_factor, planes, ransac_sigmas):
    """-> int32 [len(planes) + 1]: every trial's inliers (-1: void), then the valid pixels."""
    d = np.asarray(frame, dtype=np.float32).ravel().astype(np.float64)
    ok = valid(frame, dmin, dmax)
    out = np.zeros(len(planes) + 1, dtype=np.int32)
    out[-1] = int(ok.sum())
    with np.errstate(all="ignore"):
        for t, (a, b, c, void) in enumerate(np.asarray(planes, dtype=np.float64).reshape(-1, 4)):
            if void != 0.0:
                out[t] = -1
                continue
            w = _w(a, b, c, rows, cols)
            z = 1.0 / w
            out[t] = int((ok & (w > 0.0) & (np.abs(d - z) <= ransac_sigmas * sigma(z, model_sigma, sigma_factor))).sum())
    return out


def best(planes, cnt, min_inlier_fraction):
    """-> record [8]: accepted, a, b, c, count, n_valid, trial, 0 (the highest count, ties to the lowest trial)."""
    planes = np.asarray(planes, dtype=np.float64).reshape(-1, 4)
    cnt = np.asarray(cnt)
    T = len(planes)
    t = int(np.argmax(cnt[:T]))                     # (argmax: the first of equal maxima)
    c, n_valid = int(cnt[t]), int(cnt[T])
    accepted = c >= 3 and np.float64(c) >= np.float64(min_inlier_fraction) * np.float64(n_valid)
    return np.array([1.0 if accepted else 0.0, planes[t, 0], planes[t, 1], planes[t, 2], c, n_valid, t, 0.0])


def mask(frame, rows, cols, model_sigma, sigma_factor, rec, mask_sigmas):
    """-> the seeding frame, flat float32: kept pixels keep their bits, the others are NaN."""
    f = np.asarray(frame, dtype=np.float32).ravel()
    if rec[0] == 0.0:
        return f.copy()
    with np.errstate(all="ignore"):
        w = _w(rec[1], rec[2], rec[3], rows, cols)
        z = 1.0 / w
        keep = (w <= 0.0) | (z - f.astype(np.float64) > mask_sigmas * sigma(z, model_sigma, sigma_factor))
    return np.where(keep, f, NAN32).astype(np.float32)


def foreground(frame, rows, cols, dmin, dmax, model_sigma, sigma_factor, seed, plane_trials=256, ransac_sigmas=2.0, mask_sigmas=5.0,
               min_inlier_fraction=0.2):
    """Steps 1-4 on a coarse frame -> (record [8] with the pixels masked filled in, the seeding frame [rows, cols])."""
    planes = trials(frame, rows, cols, dmin, dmax, seed, plane_trials)
    cnt = counts(frame, rows, cols, dmin, dmax, model_sigma, sigma_factor, planes, ransac_sigmas)
    rec = best(planes, cnt, min_inlier_fraction)
    out = mask(frame, rows, cols, model_sigma, sigma_factor, rec, mask_sigmas)
    rec[7] = rec[5] - int(valid(out, dmin, dmax).sum())
    return rec, out.reshape(rows, cols)


# the six scenes of the accuracy bar (tests/test_gpu_finder.py): mesh, scene seed - 100
SCENES = [("m1", 1), ("m1", 2), ("m2", 1), ("m2", 2), ("m3", 1), ("m3", 2)]


def scene_labels(object_depth, rows, cols):
    """Labels of a synth.make_frame scene from its noise-free frame: 0 plane, 1 object, 2 occluder, [rows, cols]."""
    from dbot_ros_amd import synth
    d = np.asarray(object_depth, dtype=np.float64).reshape(rows, cols)
    d = np.where(np.isfinite(d), d, np.inf)
    clean = synth.make_frame(d, rows, cols, None, noise=False, nan_frac=0).reshape(rows, cols)
    bare = synth.make_frame(d, rows, cols, None, noise=False, nan_frac=0, occluder=False).reshape(rows, cols)
    lab = np.zeros((rows, cols), dtype=np.int8)
    lab[np.isfinite(d)] = 1
    lab[clean != bare] = 2
    return lab


def check_caps(rec, seed_frame, coarse, labels, dmin, dmax):
    """The issue's caps on one scene: a plane is accepted, <= 0.1 % of the plane-labelled valid coarse pixels stay, >= 95 % of
    the object-labelled ones do.  Returns the two fractions."""
    ok = valid(coarse, dmin, dmax).reshape(coarse.shape)
    kept = valid(seed_frame, dmin, dmax).reshape(coarse.shape)
    assert not np.any(kept & ~ok)
    plane, obj = ok & (labels == 0), ok & (labels == 1)
    assert plane.sum() > 1000 and obj.sum() > 20, (plane.sum(), obj.sum())
    kp, ko = (kept & plane).sum() / plane.sum(), (kept & obj).sum() / obj.sum()
    assert rec[0] == 1.0, rec
    assert kp <= 0.001 and ko >= 0.95, (kp, ko, rec)
    return kp, ko
