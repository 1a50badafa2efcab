"""Arguments of the per-pixel likelihood's math checks, shared by tests/test_math_cpu.py (the host build of
dbot_ros_amd/csrc/rbs_math.h) and tests/test_gpu_pixel_math.py (the same functions on the device): both look at
the same values.  Test infrastructure."""
import numpy as np

# the two model parameter sets of the pixel-by-pixel checks (defaults; a heavier tail with a narrower Gaussian)
PARAM_SETS = [{}, {"tail_weight": 0.05, "model_sigma": 0.001, "sigma_factor": 0.003}]

EXP_TAIL = [-745.0, -800.0, -1e6, -np.inf]          # gradual underflow and the clamp
LOG_ODD = [0.0, np.inf, np.nan, -1.0, 1e-40]        # not a positive normal float


def exp_args():
    rng = np.random.default_rng(0)
    return -np.concatenate([rng.uniform(0, 40, 300000), rng.uniform(0, 1, 200000), rng.uniform(0, 700, 100000),
                            [0.0, 1e-300, 0.5 * np.log(2), 708.0]])


def erfc_args():
    rng = np.random.default_rng(2)
    return np.concatenate([rng.uniform(0, 6, 400000), rng.uniform(0, 0.5, 100000), rng.uniform(6, 1e3, 1000),
                           np.arange(0, 49) / 8.0, np.arange(1, 49) / 8.0 - 1e-12, [np.inf, 1e300]])


def log_args():
    rng = np.random.default_rng(4)
    return np.concatenate([rng.uniform(1e-3, 1e4, 400000), np.exp(rng.uniform(-87, 88, 300000)), rng.uniform(0.9, 1.1, 100000),
                           [1.0, 2.0, 0.5, np.float32(1.0) + np.finfo(np.float32).eps, 1.1754944e-38, 3.4028235e38]]).astype(np.float32)


def pixels(n, seed):
    """(observation, rendered depth, prior) triples as the raster kernel meets them: the object seen
    (|r - o| of a few sigma), occluders in front (o << r), the background behind (o >> r), priors
    over the whole unit interval."""
    rng = np.random.default_rng(seed)
    r = rng.uniform(0.3, 3.0, n)
    sigma = 0.003 + 0.0014247 * r * r
    kind = rng.integers(0, 4, n)
    o = np.where(kind <= 1, r + sigma * rng.normal(0, 1.5, n),
                 np.where(kind == 2, r - rng.uniform(0.01, 0.29, n), r + rng.uniform(0.01, 3.0, n)))
    prior = np.where(rng.random(n) < 0.5, rng.uniform(0.0, 1.0, n), np.float32(0.1))
    return o.astype(np.float32), r.astype(np.float32), prior.astype(np.float32)


def check_pixel_terms(ll, post, ref_ll, ref_post):
    """The bars of the F64 pixel term against the oracle's (libm) term, pixel by pixel: identical except where a
    float rounding of a, b or a quotient flips (<= 2e-5 of pixels, each then within 2 float ulps of the ratio);
    the posterior identical except <= 2e-5 of pixels at 1 float ulp; sums over 5 000 pixels within 1e-11."""
    assert np.all(np.isfinite(ll)) and np.all(np.isfinite(ref_ll))
    same = ll == ref_ll
    d = np.abs(ll - ref_ll)
    # where the argument of the log (a float) is the same, the logs agree to their rounding; a flipped
    # float rounding moves the term by a float ulp or two of the ratio
    assert d[same].size and np.all(d <= 2.6e-7), d.max()
    close = d <= 2.5e-16 + 2 * np.spacing(np.abs(ref_ll))
    assert (~close).mean() <= 2e-5, (~close).mean()
    pd = np.abs(post.view(np.int32).astype(np.int64) - ref_post.view(np.int32).astype(np.int64))
    assert pd.max() <= 1 and (pd != 0).mean() <= 2e-5, (pd.max(), (pd != 0).mean())
    # a particle's sum over 5 000 such pixels: the north-star tolerance with six orders to spare
    s, sr = ll.reshape(-1, 5000).sum(1), ref_ll.reshape(-1, 5000).sum(1)
    assert (np.abs(s - sr) / np.maximum(1.0, np.abs(sr))).max() <= 1e-11
