"""What the posterior report's tests share: the brute-force reference in np.longdouble, the derived bars, planted
populations, and the ctypes wrapper of rbs_test_posterior (the hooks build's probe of csrc/rbsensor_posterior.hip).
Test infrastructure.

Bars (u = 2^-53, the reference in np.longdouble):
  cov    |cov - ref|[a][b] <= 4 n u sqrt(ref[a][a] ref[b][b]) + (4 n u)^2 max|x_a| max|x_b|
         Cauchy-Schwarz: the sum of the terms' magnitudes is at most sqrt(V_aa V_bb) S; recursive summation loses at most n u
         of that; the 4 covers the exponential's last bits and the three roundings per term; the second term is the mean's
         own rounding, which enters squared.
  mean   4 n u sum e_i |x_i[c]| / S
  ess    relative 8 n u
  integers exact;  cov's smallest eigenvalue >= - the first bar's largest entry (smallest_eigenvalue_at_least: a factorisation
  in np.longdouble, no eigenvalue solver's error to allow for)."""
import ctypes as C

import numpy as np

from dbot_ros_amd import pose
from dbot_ros_amd.tracker import BODY, Posterior

U = 2.0 ** -53
KINDS = ("uniform", "spread", "dominant", "neg_inf", "identical", "velocity")


def reference(x, lw, idx):
    """The rule by brute force in np.longdouble -> dict(mean, cov, ess, survivors, abs_mean)."""
    xl = np.asarray(x, dtype=np.longdouble).reshape(len(lw), -1)
    lwl = np.asarray(lw, dtype=np.longdouble)
    e = np.exp(lwl - lwl.max())
    S = e.sum()
    mean = (e[:, None] * xl).sum(axis=0) / S
    d = xl - mean
    cov = (e[:, None] * d).T @ d / S
    return dict(mean=mean, cov=cov, ess=S * S / (e * e).sum(), survivors=len(set(np.asarray(idx).tolist())),
                abs_mean=(e[:, None] * np.abs(xl)).sum(axis=0) / S)


def bars(ref, x):
    """-> (cov bar [D, D], mean bar [D], relative ess bar) for a population of n = len(x)."""
    x = np.asarray(x, dtype=np.float64).reshape(len(x), -1)
    n = x.shape[0]
    sd = np.sqrt(np.maximum(np.diag(ref["cov"]).astype(np.float64), 0.0))
    xmax = np.abs(x).max(axis=0)
    return (4 * n * U * np.outer(sd, sd) + (4 * n * U) ** 2 * np.outer(xmax, xmax), 4 * n * U * ref["abs_mean"].astype(np.float64),
            8 * n * U)


def smallest_eigenvalue_at_least(A, lo):
    """True when the symmetric matrix A has no eigenvalue below lo: A - lo I is factored L D L^T in np.longdouble without
    pivoting, and is positive semidefinite exactly when no pivot is negative (a zero pivot needs a zero column under it).
    No eigenvalue solver and no allowance for one: the factorisation's own rounding, D 2^-64 ||A||, is three orders below
    the bars this is used with."""
    M = np.array(A, dtype=np.longdouble)
    M[np.diag_indices_from(M)] -= np.longdouble(lo)
    for k in range(M.shape[0]):
        d = M[k, k]
        if d < 0:
            return False
        if d == 0:
            if np.any(M[k + 1:, k] != 0):
                return False
            continue
        c = M[k + 1:, k].copy()
        M[k + 1:, k + 1:] -= np.outer(c, c) / d
    return True


def check(rep, x, lw, idx, note=None):
    """A Posterior against the brute-force reference of (x, lw, idx), every bar above.  Returns the reference."""
    ref = reference(x, lw, idx)
    cov_bar, mean_bar, ess_bar = bars(ref, x)
    dc = np.abs(rep.cov.astype(np.longdouble) - ref["cov"]).astype(np.float64)
    dm = np.abs(rep.mean.astype(np.longdouble) - ref["mean"]).astype(np.float64)
    de = float(abs(np.longdouble(rep.ess) - ref["ess"]) / ref["ess"])
    if note is not None:
        with np.errstate(divide="ignore", invalid="ignore"):
            note["cov"] = max(note.get("cov", 0.0), float(np.nanmax(np.where(cov_bar > 0, dc / cov_bar, 0.0))))
            note["mean"] = max(note.get("mean", 0.0), float(np.nanmax(np.where(mean_bar > 0, dm / mean_bar, 0.0))))
        note["ess"] = max(note.get("ess", 0.0), de / ess_bar)
    assert np.all(dc <= cov_bar), ("cov", float((dc - cov_bar).max()), np.unravel_index(np.argmax(dc - cov_bar), dc.shape))
    assert np.all(dm <= mean_bar), ("mean", float((dm - mean_bar).max()))
    assert de <= ess_bar, ("ess", de, ess_bar)
    assert np.array_equal(rep.cov, rep.cov.T), "cov is not symmetric bit for bit"
    assert smallest_eigenvalue_at_least(rep.cov, -cov_bar.max()), ("cov's smallest eigenvalue", float(np.linalg.eigvalsh(rep.cov).min()),
                                                                    -float(cov_bar.max()))
    assert rep.survivors == ref["survivors"] and rep.n == len(lw)
    return ref


def population(kind, n, parts, seed=0):
    """Planted (x [n, parts * 12], lw [n], idx [n]).  Bodies after the first are correlated with the first (cross-body
    blocks).  Kinds: uniform weights; spread (Gaussian log-weights); one dominant weight (ess -> 1); a tenth (at least one)
    at -inf; all particles identical; velocities whose mean is 1 000 times their spread."""
    rng = np.random.default_rng([n, parts, seed, KINDS.index(kind)])
    scale = np.repeat([0.01, 0.05, 0.002, 0.02], 3)
    x = np.empty((n, parts * BODY))
    x[:, :BODY] = rng.standard_normal((n, BODY)) * scale
    for b in range(1, parts):
        x[:, BODY * b:BODY * (b + 1)] = (0.5 - 0.8 * (b - 1)) * x[:, :BODY] + 0.5 * rng.standard_normal((n, BODY)) * scale
    lw = np.zeros(n)
    if kind in ("spread", "neg_inf", "velocity"):
        lw = 3.0 * rng.standard_normal(n) - 700.0
    if kind == "dominant":
        lw = np.full(n, -50.0) + rng.standard_normal(n)
        lw[n // 2] = 0.0
    if kind == "neg_inf" and n > 1:
        lw[rng.permutation(n)[:max(1, n // 10)]] = -np.inf
    if kind == "identical":
        x[:] = x[0]
        lw = rng.standard_normal(n)
    if kind == "velocity":
        for b in range(parts):
            x[:, BODY * b + 6:BODY * b + 12] = np.repeat([2.0, 20.0], 3) * (1.0 + 1e-3 * rng.standard_normal((n, 6)))
    idx = rng.integers(0, n, n).astype(np.int32)
    return x, lw, idx


def planted_mean(parts, seed=0):
    """[parts * 12 + parts * 9]: mean rows and the transposed mean rotations, as mean_kernel leaves them for recentre_body."""
    rng = np.random.default_rng([parts, seed, 77])
    mu = rng.standard_normal((parts, BODY)) * np.repeat([0.004, 0.03, 0.002, 0.02], 3)
    RmT = np.stack([pose.rotvec_to_matrix(mu[b, 3:6]).T for b in range(parts)])
    return np.concatenate([mu.ravel(), RmT.ravel()])


def recentred(x, mean, parts):
    """recentre_body in numpy: t -= t_mean, R(delta) <- R(delta) R(mean)^T."""
    from dbot_ros_amd.tracker import _rotvecs
    x = np.array(x, dtype=np.float64)
    p = x.reshape(len(x), parts, BODY)
    mu = mean[:parts * BODY].reshape(parts, BODY)
    RmT = mean[parts * BODY:].reshape(parts, 3, 3)
    for b in range(parts):
        p[:, b, 0:3] -= mu[b, 0:3]
        p[:, b, 3:6] = _rotvecs(pose.rotvec_to_matrix(p[:, b, 3:6]) @ RmT[b])
    return x


class PosteriorProbe:
    """rbs_test_posterior of the hooks build."""

    def __init__(self, path):
        self.lib = C.CDLL(path)
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        self.lib.rbs_test_posterior.restype = C.c_int32
        self.lib.rbs_test_posterior.argtypes = [C.c_int32, C.c_int32, dp, dp, ip, dp, C.c_int32, C.c_int32, C.c_uint64, dp, ip]

    def run(self, x, lw, idx, mean=None, recentred=True, resampled=False, frame=0):
        """-> (Posterior, True when the kernels left particles, log-weights and slot map as they were)."""
        n, D = x.shape
        parts = D // BODY
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        xs, lws, ids = (np.array(a, order="C") for a in (x, lw, idx.astype(np.int32)))
        mean = np.ascontiguousarray(np.zeros(D + parts * 9) if mean is None else mean)
        out, out_i = np.empty(1 + D + D * D), np.empty(4, dtype=np.int32)
        rc = self.lib.rbs_test_posterior(n, parts, xs.ctypes.data_as(dp), lws.ctypes.data_as(dp), ids.ctypes.data_as(ip), mean.ctypes.data_as(dp),
                                         1 if recentred else 0, 1 if resampled else 0, frame, out.ctypes.data_as(dp), out_i.ctypes.data_as(ip))
        assert rc == 0, rc
        untouched = (xs.tobytes() == np.ascontiguousarray(x).tobytes() and lws.tobytes() == np.ascontiguousarray(lw).tobytes()
                     and np.array_equal(ids, idx))
        return Posterior(mean=out[1:1 + D].copy(), cov=out[1 + D:].reshape(D, D).copy(), ess=float(out[0]), survivors=int(out_i[1]),
                         resampled=bool(out_i[2]), n=int(out_i[0]), frame=int(out_i[3])), untouched


def same_bits(a, b):
    """Two Posteriors, bit for bit."""
    return (a.mean.tobytes() == b.mean.tobytes() and a.cov.tobytes() == b.cov.tobytes() and np.float64(a.ess).tobytes() == np.float64(b.ess).tobytes()
            and (a.survivors, a.resampled, a.n, a.frame) == (b.survivors, b.resampled, b.n, b.frame))
