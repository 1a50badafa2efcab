"""What the posterior modes' tests share: the rule by brute force in np.longdouble (row-blocked to bound memory), the planted
populations with their asserted decision margins, the derived bars and the comparison.  Test infrastructure.

Bars (u = 2^-53; the reference in np.longdouble).  Notation: P = max |p| / h_t over the population, c4 = 4 / h_r^2,
E = max |lw_i - m| over the log-weights whose e_i counts (e_i >= 2^-960, the rule's cut: E <= 666), n particles.
  d2     absolute error A u inside the support (d2 < 1), A = T + R + 2:
           T = 7 P + 9     a scaled coordinate fl(p / h_t) carries u |a|; a difference u (|a| + |b| + |dx|) <= u (2 P + 1.01); the
                           three squares and their sum 2 sqrt(3) (2 P + 1.01) |dx| u + 5 u |dx|^2 with |dx| <= 1.01
           R = c4 (8 Q + 10) + 1.01,  Q = 16     a quaternion component is off by at most Q u absolute (|r| 2.5 u relative, so the
                           half angle -- up to pi for a rotation vector beyond pi -- 8 u absolute; sin, cos, the division by |r| and
                           the product the rest); q_i . q_j then (4 Q + 4) u, its square (8 Q + 9) u, 1 - c^2 one more, times c4
  rho    (n + c) u sum_j e_j [d2_ij < 1 + A u] / S  at a seed,  c = A + 2 E + 8 + 64:
           a pair term e_j max(0, 1 - d2) is Lipschitz 1 in d2, so A u from d2, (E + 2) u from e_j = exp(lw_j - m) (the subtraction's
           rounding u |lw_j - m| becomes a relative error of e_j; the exponential's last bits), three roundings for 1 - d2, the
           product and the final division; n u for the recursive sum of the terms; S carries (E + 2) u from its terms and at most
           64 u from its own summation -- it is summed by trees in both implementations (block_sum's shuffle tree, four waves
           and n / 256 <= 33 partials on the device up to 8 200 particles; pairwise in numpy)
  pos    4 n u sum e |p| / sum e over the core
  mass   8 n u relative (mass and core_mass)
  rot    (10 (n + Q + E + 3) + 16) u per component, radians: a component of the aligned quaternion sum is off by
           (n + Q + E + 3) u W, W = the core's sum of e; the sum's norm is at least 0.86 W (h_r <= 1 keeps every aligned member
           within 30 degrees of the seed), so the unit quaternion is off by delta = (n + Q + E + 3) u / 0.86 per component; the angle
           2 atan2(|v|, w) moves by at most 4 delta, the axis times the angle by as much again; 16 u for the normalisation,
           atan2 and the scaling
  seeds, n_modes exact.  Memberships are decided by the same comparisons; they enter through mass and core_mass.

Margins.  Integers are decided by floating comparisons, so planted() asserts in np.longdouble that every decision has a relative
margin of at least 1e-6 -- six orders above the bars: seed against runner-up among the candidates (a candidate whose pose is
bit for bit the seed's has bit for bit its rho in any implementation that computes a row from the row's own pose, and the rule
breaks that tie by index: such copies are no runner-up); d2 against separation^2 in every suppression; d2 against 1 in the
core test; nearest seed against second nearest in the assignment.  A draw that misses a margin is drawn again with the next
seed: no case is left out."""
import functools

import numpy as np

from dbot_ros_amd.tracker import MODES_E_MIN, ModesParams

U = 2.0 ** -53
LD = np.longdouble
MARGIN = 1e-6
Q_ERR = 16.0
COARSE_FROM, COARSE_TOL = 2048, 1e-10
PATTERNS = ("tight", "two", "many", "identical", "one_alive", "beyond_pi", "flip")
BODIES_123 = "bodies_123"          # three bodies with 1, 2 and 3 clusters


def _quat(r):
    angle = np.sqrt((r * r).sum(-1))
    half = angle / 2
    safe = np.where(angle > 0, angle, LD(1))
    k = np.where(angle > 0, np.sin(half) / safe, LD(0.5))
    return np.concatenate([np.cos(half)[:, None], r * k[:, None]], axis=1)


def _d2(pa, qa, pb, qb, c4):
    d = pa - pb
    c = (qa * qb).sum(-1)
    return (d * d).sum(-1) + c4 * (1 - c * c)


def _d2_rows(pb, qb, p, q, c4):
    """Rows pb, qb [a, .] against the population [n, .] -> [a, n], two-dimensional temporaries only."""
    d = np.zeros((len(pb), len(p)), dtype=LD)
    for k in range(3):
        t = pb[:, k, None] - p[None, :, k]
        d += t * t
    c = np.zeros_like(d)
    for k in range(4):
        c += qb[:, k, None] * q[None, :, k]
    c *= c
    np.subtract(1, c, out=c)
    c *= c4
    d += c
    return d


def reference(x, lw, params, block=256):
    """The rule by brute force in np.longdouble.  x [n, parts, >= 6].  -> list per body of dict(seeds, rho_seed, support, mass,
    core_mass, pos, rot, abs_pos, margin, n_core), plus the population's constants under key None of the returned dict."""
    x = np.asarray(x, dtype=np.float64)
    n, parts = x.shape[0], x.shape[1]
    lwl = np.asarray(lw, dtype=LD)
    # (the rule: e_i below 2^-960 counts as 0 -- the particle is no candidate and no member)
    with np.errstate(under="ignore"):
        alive64 = np.exp(np.asarray(lw, dtype=np.float64) - np.max(lw)) >= MODES_E_MIN
    e = np.where(alive64, np.exp(lwl - lwl.max()), LD(0))
    S = e.sum()
    h_t, c4, sep2 = LD(params.h_t), 4 / (LD(params.h_r) * LD(params.h_r)), LD(params.separation) * LD(params.separation)
    E = float(np.abs(np.asarray(lw, dtype=np.float64)[alive64] - np.max(lw)).max())
    Pmax = float(np.abs(x[:, :, 0:3]).max() / params.h_t)
    A = (7 * Pmax + 9) + (float(c4) * (8 * Q_ERR + 10) + 1.01) + 2
    out = {None: dict(n=n, E=E, A=A, c=A + 2 * E + 8 + 64)}
    bodies = []
    for b in range(parts):
        p, q = x[:, b, 0:3].astype(LD) / h_t, _quat(x[:, b, 3:6].astype(LD))
        def rho_rows(rows):
            out = np.empty(len(rows), dtype=LD)
            for lo in range(0, len(rows), block):
                r = rows[lo:lo + block]
                k = _d2_rows(p[r], q[r], p, q, c4)
                np.subtract(1, k, out=k)
                np.maximum(k, 0, out=k)
                out[lo:lo + block] = (k @ e) / S
            return out

        # Above COARSE_FROM particles the pair pass is taken in binary64 first (its error is below COARSE_TOL absolutely: the rho
        # bar with support <= 1), and np.longdouble only for the rows within 2 COARSE_TOL of a round's maximum -- every other row
        # enters the margin with its binary64 value plus COARSE_TOL, an upper bound.
        exact = n <= COARSE_FROM
        if exact:
            rho, slack = rho_rows(np.arange(n)), LD(0)
        else:
            assert (n + out[None]["c"]) * U < COARSE_TOL
            p64, q64, e64 = p.astype(np.float64), q.astype(np.float64), e.astype(np.float64)
            rho = np.empty(n, dtype=LD)
            for lo in range(0, n, 512):
                d = np.zeros((len(p64[lo:lo + 512]), n))
                for k in range(3):
                    t = p64[lo:lo + 512, k, None] - p64[None, :, k]
                    d += t * t
                c = q64[lo:lo + 512] @ q64.T
                rho[lo:lo + 512] = (np.maximum(1.0 - (d + float(c4) * (1.0 - c * c)), 0.0) @ e64) / float(S)
            slack = LD(COARSE_TOL)
            known = np.zeros(n, dtype=bool)
        margin = np.inf
        cand = e > 0
        seeds = []
        while len(seeds) < params.k_max and cand.any():
            if not exact:
                top = np.where(cand, rho + np.where(known, 0, slack), -1).max()
                rows = np.nonzero(cand & ~known & (rho + slack >= top - 2 * slack))[0]
                rho[rows] = rho_rows(rows)
                known[rows] = True
            bound = rho if exact else rho + np.where(known, 0, slack)
            s = int(np.argmax(np.where(cand & (True if exact else known), rho, -1)))
            other = cand & ~np.all(x[:, b, 0:6] == x[s, b, 0:6], axis=1)
            if other.any():
                margin = min(margin, float((rho[s] - bound[other].max()) / rho[s]))
            ds = _d2(p, q, p[s][None], q[s][None], c4)
            margin = min(margin, float((np.abs(ds[e > 0] - sep2) / sep2).min()))
            seeds.append(s)
            cand &= ~(ds < sep2)
        D = np.stack([_d2(p, q, p[s][None], q[s][None], c4) for s in seeds], axis=1)
        near = np.argmin(D, axis=1)
        alive = np.asarray(e > 0)
        if len(seeds) > 1:
            two = np.sort(D[alive], axis=1)[:, :2]
            margin = min(margin, float(((two[:, 1] - two[:, 0]) / two[:, 1]).min()))
        dmin = D[np.arange(n), near]
        margin = min(margin, float(np.abs(dmin[alive] - 1).min()))
        support = [((D[:, k] < 1 + A * U) * e).sum() / S for k in range(len(seeds))]      # (d2 is symmetric: the seed's row)
        rec = dict(seeds=seeds, rho_seed=[rho[s] for s in seeds], support=support, mass=[], core_mass=[], pos=[], rot=[],
                   abs_pos=[], n_core=[], margin=margin)
        for k, s in enumerate(seeds):
            member = (near == k) & alive
            core = member & (dmin < 1)
            ec = e[core]
            sign = np.where((q[core] * q[s][None]).sum(-1) < 0, LD(-1), LD(1))
            qm = ((ec * sign)[:, None] * q[core]).sum(0) / ec.sum()
            qm = qm / np.sqrt((qm * qm).sum())
            if qm[0] < 0:
                qm = -qm
            vn = np.sqrt((qm[1:] * qm[1:]).sum())
            rec["rot"].append(qm[1:] * (2 * np.arctan2(vn, qm[0]) / vn) if vn > 0 else np.zeros(3, dtype=LD))
            rec["pos"].append((ec[:, None] * p[core]).sum(0) / ec.sum() * h_t)
            rec["abs_pos"].append((ec[:, None] * np.abs(p[core])).sum(0) / ec.sum() * h_t)
            rec["mass"].append(e[member].sum() / S)
            rec["core_mass"].append(ec.sum() / S)
            rec["n_core"].append(int(core.sum()))
        bodies.append(rec)
    out["bodies"] = bodies
    return out


def check(modes, ref, note=None):
    """A tracker.Modes against reference(): integers exact, values within the bars above."""
    head = ref[None]
    n, E, c = head["n"], head["E"], head["c"]
    assert len(modes.bodies) == len(ref["bodies"])
    for b, (got, want) in enumerate(zip(modes.bodies, ref["bodies"])):
        assert [m.seed for m in got] == want["seeds"], (b, [m.seed for m in got], want["seeds"], want["margin"])
        rot_bar = (10 * (n + Q_ERR + E + 3) + 16) * U
        for k, m in enumerate(got):
            figures = dict(
                rho=(abs(LD(m.density) - want["rho_seed"][k]), (n + c) * U * want["support"][k]),
                mass=(abs(LD(m.mass) - want["mass"][k]) / want["mass"][k], 8 * n * U),
                core_mass=(abs(LD(m.core_mass) - want["core_mass"][k]) / want["core_mass"][k], 8 * n * U),
                pos=(np.abs(m.delta[0:3].astype(LD) - want["pos"][k]), 4 * n * U * want["abs_pos"][k]),
                rot=(np.abs(m.delta[3:6].astype(LD) - want["rot"][k]), rot_bar))
            for name, (err, bar) in figures.items():
                err, bar = np.asarray(err, dtype=np.float64), np.asarray(bar, dtype=np.float64)
                if note is not None:
                    with np.errstate(divide="ignore", invalid="ignore"):
                        note[name] = max(note.get(name, 0.0), float(np.max(np.where(bar > 0, err / bar, np.where(err > 0, np.inf, 0.0)))))
                assert np.all(err <= bar), (name, b, k, err.tolist(), bar.tolist())
        assert abs(sum(m.mass for m in got) - float(sum(want["mass"]))) <= 8 * n * U * len(got)


def _cluster(rng, count, centre_p, centre_r, params, tight=1.0):
    """count members around a centre: positions 0.2 h_t, rotations 0.15 h_r apart (a typical pair inside one bandwidth, some not);
    the rotation noise multiplies the centre's rotation from the left."""
    from dbot_ros_amd import pose
    from dbot_ros_amd.tracker import _rotvecs
    p = centre_p + tight * 0.2 * params.h_t * rng.standard_normal((count, 3))
    noise = tight * 0.15 * params.h_r * rng.standard_normal((count, 3))
    R = pose.rotvec_to_matrix(noise) @ pose.rotvec_to_matrix(np.asarray(centre_r, dtype=np.float64))
    return np.concatenate([p, _rotvecs(R)], axis=1)


def _body(pattern, n, params, rng):
    """-> (deltas [n, 6], forced log-weights or None)."""
    h = params.h_t
    if pattern == "tight":
        return _cluster(rng, n, [0.01, -0.02, 0.005], [0.02, 0.01, -0.03], params), None
    if pattern in ("two", "three", "many"):
        k = {"two": 2, "three": 3, "many": params.k_max + 2}[pattern]
        k = min(k, n)
        share = np.array([0.7, 0.3]) if k == 2 else np.linspace(2.0, 1.0, k) / np.linspace(2.0, 1.0, k).sum()
        counts = np.maximum(1, np.floor(share * n).astype(int))
        counts[0] += n - counts.sum()
        # centres 10 h apart in translation, each with a rotation of its own
        parts = [_cluster(rng, c, [10 * h * j, -0.03 * j, 0.01], [0.05 * j, -0.02, 0.03 * j], params) for j, c in enumerate(counts)]
        return np.concatenate(parts)[_interleave(counts)], None
    if pattern == "identical":
        return np.repeat(_cluster(rng, 1, [0.013, 0.002, -0.007], [0.1, -0.05, 0.02], params), n, axis=0), None
    if pattern == "one_alive":
        lw = np.full(n, -np.inf)
        lw[n // 2] = -3.25
        return _cluster(rng, n, [0.0, 0.0, 0.0], [0.0, 0.0, 0.0], params, tight=3.0), lw
    if pattern == "beyond_pi":
        x = _cluster(rng, n, [-0.01, 0.0, 0.02], [0.5, -0.3, 0.4], params)
        ang = np.linalg.norm(x[1::2, 3:6], axis=1)
        x[1::2, 3:6] *= (1.0 - 2.0 * np.pi / ang)[:, None]           # the same rotation, its vector beyond pi
        return x, None
    if pattern == "flip":
        x = _cluster(rng, n, [0.0, 0.01, 0.0], [0.0, 0.0, 0.0], params)
        x[1::2] = _cluster(rng, len(x[1::2]), [0.0, 0.01, 0.0], [np.pi, 0.0, 0.0], params)
        return x, None
    raise ValueError(pattern)


def _interleave(counts):
    """A fixed permutation that spreads the clusters' members over the index range (chunks and tiles see every cluster)."""
    n = int(np.sum(counts))
    return np.random.default_rng(n).permutation(n)


@functools.lru_cache(maxsize=None)
def planted(pattern, n, parts, min_margin=MARGIN):
    """-> (deltas [n, parts, 6], log-weights [n], params, reference), every decision's margin asserted.  Cached: computed once,
    shared by the tests that need it, never modified (the arrays are read-only)."""
    params = ModesParams()
    names = ("tight", "two", "three")[:parts] if pattern == BODIES_123 else (pattern,) * parts
    for attempt in range(32):
        rng = np.random.default_rng([n, parts, attempt, (PATTERNS + (BODIES_123,)).index(pattern)])
        lw = 0.5 * rng.standard_normal(n) - 40.0
        x = np.empty((n, parts, 6))
        for b, name in enumerate(names):
            x[:, b], forced = _body(name, n, params, rng)
            if forced is not None:
                lw = forced
        ref = reference(x, lw, params)
        if min(body["margin"] for body in ref["bodies"]) >= min_margin:
            x.setflags(write=False)
            lw.setflags(write=False)
            return x, lw, params, ref
    raise AssertionError(f"no draw of {pattern} n={n} parts={parts} keeps every decision {min_margin:g} clear of its threshold")


def faint(n, lw_faint):
    """One body, two clusters ten bandwidths apart; the second's log-weights lie lw_faint below the first's -- either side of the
    rule's cut at 2^-960 (ln: -665.4).  -> (deltas [n, 1, 6], log-weights [n], params, reference), margins asserted."""
    params = ModesParams()
    rng = np.random.default_rng([n, 4242])
    x = np.empty((n, 1, 6))
    x[:, 0] = _body("two", n, params, rng)[0]
    far = x[:, 0, 0] > 5 * params.h_t
    lw = 0.5 * rng.standard_normal(n) - 3.0
    lw[far] += lw_faint
    ref = reference(x, lw, params)
    assert ref["bodies"][0]["margin"] >= MARGIN and 0 < far.sum() < n
    assert abs(lw_faint + 960 * np.log(2.0)) > 10.0        # (every member clearly on one side of the cut)
    return x, lw, params, ref


def assert_pattern(pattern, n, modes):
    """What a planted pattern is there to show, on a Modes of it (the twin's or the device's)."""
    bodies = modes.bodies
    if pattern == "tight" and n >= 63:
        assert all(b[0].mass > 0.9 for b in bodies)
    if pattern == "identical":                      # one mode with density 1 (to its bar: mt.check) and mass 1
        assert all(len(b) == 1 and b[0].seed == 0 and abs(b[0].mass - 1.0) <= 8 * n * U and abs(b[0].core_mass - 1.0) <= 8 * n * U
                   and abs(b[0].density - 1.0) < 1e-9 for b in bodies)
    if pattern == "one_alive":
        assert all(len(b) == 1 and b[0].seed == n // 2 and abs(b[0].mass - 1.0) <= 8 * n * U and abs(b[0].density - 1.0) < 1e-9 for b in bodies)
    if pattern == "two" and n >= 63:                # mode 0 is the heavy one
        assert all(len(b) >= 2 and b[0].mass > 0.6 > 0.4 > b[1].mass for b in bodies), [[m.mass for m in b] for b in bodies]
    if pattern == "many" and n >= 63:               # k_max + 2 clusters: truncated, and the masses still sum to 1
        assert all(len(b) == 4 and abs(sum(m.mass for m in b) - 1.0) <= 32 * n * U for b in bodies)
    if pattern == "beyond_pi" and n >= 63:          # one mode, whatever the vector's branch
        assert all(b[0].mass > 0.9 and np.linalg.norm(b[0].delta[3:6] - [0.5, -0.3, 0.4]) < 0.05 for b in bodies)
    if pattern == "flip" and n >= 63:               # the same position, two rotations: two modes
        assert all(len(b) >= 2 and b[0].mass + b[1].mass > 0.9 and min(b[0].mass, b[1].mass) > 0.3 for b in bodies)
        assert all(abs(abs(np.linalg.norm(b[0].delta[3:6]) - np.linalg.norm(b[1].delta[3:6])) - np.pi) < 0.1 for b in bodies)
    if pattern == BODIES_123 and n >= 63:
        assert [sum(m.mass > 0.1 for m in b) for b in bodies] == [1, 2, 3]


def pack(modes):
    """A Modes as arrays: (n_modes [parts], table [parts, 8, 10]: seed, density, mass, core_mass, delta -- NaN where unused)."""
    t = np.full((len(modes.bodies), 8, 10), np.nan)
    for b, body in enumerate(modes.bodies):
        for k, m in enumerate(body):
            t[b, k] = np.r_[m.seed, m.density, m.mass, m.core_mass, m.delta]
    return np.array([len(body) for body in modes.bodies]), t


def unpack(n_modes, table, frame=0):
    from dbot_ros_amd.tracker import Mode, Modes
    return Modes(bodies=[[Mode(seed=int(r[0]), density=float(r[1]), mass=float(r[2]), core_mass=float(r[3]), delta=r[4:10].copy())
                          for r in table[b, :int(n_modes[b])]] for b in range(len(n_modes))], frame=int(frame))


def same_bits(a, b):
    """Two Modes, bit for bit."""
    (na, ta), (nb, tb) = pack(a), pack(b)
    return np.array_equal(na, nb) and ta.tobytes() == tb.tobytes() and a.frame == b.frame
