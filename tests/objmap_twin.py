"""What the object map's tests share (tests/test_object_map_cpu.py, tests/test_gpu_object_map.py): the bars, populations,
planted planes.  The rules themselves are restated in dbot_ros_amd.tracker.object_map_of (np.longdouble) and segment_of.

The bars.  u = 2^-53 is binary64's unit roundoff; n members, L <= n live poses, G <= 32 parts, B <= 8 bodies.  A sum of K
same-sign terms taken in ANY order has a relative error of at most (K - 1) u / (1 - (K - 1) u) (Higham, Accuracy and
Stability of Numerical Algorithms, eq. 4.4 with all terms of one sign): every term passes through at most K - 1 additions.
Every quantity below is such a sum -- the weights are positive, the depths are positive.

  e_i    exp of the device library, a couple of ulps: relative error <= 4 u.  It perturbs numerator and denominator alike.
  W_k    at most n terms e_i.            S      n terms, 1 024 lanes then a tree: at most n + 16 additions on any path.
  c_b    at most L terms W_k, per part, then G partials: a term passes through at most n (inside W_k) + L + G additions.
  a      B terms c_b.                    s1, s2 like c_b with one product (u) -- two for s2 -- in front of each term.

cover = c_b / S:  numerator (n + L + G) u, denominator (n + 16) u, the quotient u, the exps 8 u -- at most (3 n + 64) u
    relative to a value <= 1:                 |cover_dev - T| <= 1/2 spacing32(T) + (2 n + 64) 2^-52.
depth = s1 / a:   numerator (n + L + G + 1) u, denominator (n + L + G + B) u, quotient u, exps 8 u -- at most (4 n + 96) u:
                                              |depth_dev - T| <= 1/2 spacing32(T) + (2 n + 64) 2^-52 |T|.
var = max(0, s2 / a - mu mu):  m2 = s2 / a and mu mu each carry a relative error of at most eps = (2 n + 64) 2^-52 (m2 as
    depth, with one more product; mu mu twice mu's error and one product, (8 n + 193) u <= 2 eps); the difference is taken
    of two numbers of size m2 >= mu mu, so their ABSOLUTE errors add -- the cancellation term, proportional to the squared
    depth and not to the variance -- and the subtraction adds u |var|:
                                              |var_dev - T| <= 1/2 spacing32(T) + 3 eps m2 + 2^-52 T,
    T and m2 the twin's own values.  max(0, .) moves a value towards T >= 0, never away.  The twin works in np.longdouble
    (64-bit significand here): its own cancellation error is 2^-11 of the term above.
None of these numbers is measured from the device."""
import numpy as np

from occmap_twin import spacing32_below, weight_patterns

LD = np.longdouble
SIZES = [1, 2, 63, 64, 65, 300]


def eps(n):
    return LD(2 * n + 64) * LD(2.0) ** -52


def bar_cover(t, n):
    return LD(0.5) * spacing32_below(t) + eps(n)


def bar_depth(t, n):
    t = np.asarray(t, dtype=LD)
    return LD(0.5) * spacing32_below(t) + eps(n) * np.abs(t)


def bar_var(t, m2, n):
    t = np.asarray(t, dtype=LD)
    return LD(0.5) * spacing32_below(t) + LD(3) * eps(n) * np.asarray(m2, dtype=LD) + LD(2.0) ** -52 * t


def second_moment(depth, var):
    """m2 = var + depth^2 of the twin's longdouble values (0 where there is no surface)."""
    d = np.where(np.isfinite(depth), depth, LD(0))
    return var + d * d


def check(dev, twin, n, note=None, what=""):
    """dev = (cover, depth, var) float32 from the device; twin = object_map_of's tuple.  The bars at every pixel; uncovered
    pixels exact; note[what + '/cover' ...] keeps the worst share of a bar seen."""
    cover, depth, var = (np.asarray(x, dtype=np.float32) for x in dev)
    tc, td, tv, a, _ = twin
    B = tc.shape[0]
    cover = cover.reshape(B, -1)
    depth, var = depth.ravel(), var.ravel()
    none = ~(a > 0)
    assert (cover[:, none].view(np.uint32) == 0).all(), what                      # +0.0 bit for bit
    assert (depth[none].view(np.uint32) == np.float32(np.inf).view(np.uint32)).all(), what
    assert (var[none].view(np.uint32) == 0).all(), what
    assert np.isfinite(depth[~none]).all() and (var >= 0).all(), what
    assert (cover[tc == 0].view(np.uint32) == 0).all(), what                      # exactly 0 where no plane of the body owns the pixel
    shares = {}
    shares["cover"] = float((np.abs(cover.astype(LD) - tc) / bar_cover(tc, n)).max())
    on = ~none
    if on.any():
        shares["depth"] = float((np.abs(depth[on].astype(LD) - td[on]) / bar_depth(td[on], n)).max())
        m2 = second_moment(td[on], tv[on])
        shares["var"] = float((np.abs(var[on].astype(LD) - tv[on]) / bar_var(tv[on], m2, n)).max())
    for k, v in shares.items():
        if note is not None:
            note[what + "/" + k] = max(note.get(what + "/" + k, 0.0), v)
        assert v <= 1.0, (what, k, n, v)
    return shares


def member_patterns(n, m, rng):
    """Pose indices [n] into m poses: the identity needs m == n."""
    i = np.arange(n)
    out = {"one_pose": np.full(n, min(3, m - 1)), "sorted_repeats": np.sort(rng.integers(0, m, n)), "permutation": rng.permutation(n) % m}
    if m == n:
        out["identity"] = None
    return out


def populations(m_of, seed=0):
    """(name, n, m, members int32 [n] or None, log-weights [n] or None) over every size, member pattern and weight pattern;
    m_of(n): the number of poses a population of n members draws on."""
    rng = np.random.default_rng(seed)
    out = []
    for n in SIZES:
        m = m_of(n)
        for mn, idx in member_patterns(n, m, rng).items():
            for wn, lw in weight_patterns(n, rng).items():
                out.append((f"n{n}-{mn}-{wn}", n, m, None if idx is None else idx.astype(np.int32), lw))
    return out


def planted(rows=6, cols=8):
    """Three poses of two bodies on a 6 x 8 frame, worked out by hand in tests/test_object_map_cpu.py:
    pose 0: body 0 at 1.0 over columns 0..3, body 1 at 0.5 over columns 2..5 -- but its rectangle ends at column 5, so its
            value at column 5 is not read; rows 1..3 both.
    pose 1: the two bodies TIE at 2.0 over columns 2..3 of row 2 (body 0 keeps them); body 1's rectangle is EMPTY otherwise.
    pose 2: the same surfaces as pose 0 -- its member has log-weight -inf."""
    P = np.full((3, 2, rows, cols), np.inf, dtype=np.float32)
    R = np.zeros((3, 2, 4), dtype=np.int64)
    P[0, 0, 1:4, 0:4] = 1.0
    R[0, 0] = (0, 1, 4, 4)
    P[0, 1, 1:4, 2:6] = 0.5
    R[0, 1] = (2, 1, 5, 4)
    P[1, 0, 2, 2:4] = 2.0
    R[1, 0] = (2, 2, 4, 3)
    P[1, 1, 2, 2:4] = 2.0
    R[1, 1] = (2, 2, 4, 3)
    P[2], R[2] = P[0], R[0]
    return P, R
