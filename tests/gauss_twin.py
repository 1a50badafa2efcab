"""CPU twin of the robust Gaussian tracker in numpy: the oracle of record for
rbs_gauss_* (dbot_ros_amd/gaussian.py).  Sigma poses are rendered through a caller-supplied depth
function -- the CPU oracle's orc_render in the tests (oracle_binding.Oracle.render_depth), whose depths
the device reproduces bit for bit.  States are in model coordinates (the default pose z of the
centred meshes), as they cross the C-ABI."""
import numpy as np

from dbot_ros_amd.pose import matrix_to_rotvec, pack_Rt, rotvec_to_matrix

BODY = 12


class Params:
    """rbs_gauss_params; the defaults are R:config/gaussian_tracker.yaml's."""

    def __init__(self, linear_sigma=(0.002,) * 3, angular_sigma=(0.01,) * 3, velocity_factor=0.8, ut_alpha=1.0,
                 fg_noise_std=0.001, bg_depth=-3.0, bg_noise_std=100.0, tail_weight=0.1, uniform_tail_min=-5000.0,
                 uniform_tail_max=5000.0):
        self.linear_sigma, self.angular_sigma = np.array(linear_sigma, float), np.array(angular_sigma, float)
        self.velocity_factor, self.ut_alpha = float(velocity_factor), float(ut_alpha)
        self.fg_noise_std, self.bg_depth, self.bg_noise_std = float(fg_noise_std), float(bg_depth), float(bg_noise_std)
        self.tail_weight = float(tail_weight)
        self.uniform_tail_min, self.uniform_tail_max = float(uniform_tail_min), float(uniform_tail_max)

    @classmethod
    def from_builder(cls, p):
        """From dbot_ros_amd.gaussian.GaussianTrackerBuilder.Parameters."""
        t, o = p.object_transition, p.observation
        return cls((t.linear_sigma_x, t.linear_sigma_y, t.linear_sigma_z), (t.angular_sigma_x, t.angular_sigma_y, t.angular_sigma_z),
                   t.velocity_factor, p.ut_alpha, o.fg_noise_std, o.bg_depth, o.bg_noise_std, o.tail_weight,
                   o.uniform_tail_min, o.uniform_tail_max)


class GaussTwin:
    def __init__(self, params, parts, render=None):
        """render: absolute poses [parts, 12] (R|t) -> float32 depth [rows*cols], +inf uncovered."""
        self.p, self.B, self.render = params, int(parts), render
        self.D, self.NP = BODY * self.B, 6 * self.B
        self.nd = 1 + 2 * self.NP
        a2 = params.ut_alpha ** 2
        self.c = a2 * self.D
        self.sqrtc = np.sqrt(self.c)
        self.wm0 = 1.0 - 1.0 / a2
        self.wc0 = self.wm0 + 1.0 - a2 + 2.0
        self.w = 1.0 / (2.0 * self.c)
        # state index -> pose-first index
        self.perm = np.array([6 * b + d if d < 6 else self.NP + 6 * b + d - 6 for b in range(self.B) for d in range(BODY)])
        self.z = np.zeros(self.D)
        self.mu = np.zeros(self.D)
        self.cov = np.zeros((self.D, self.D))

    # ---- pieces --------------------------------------------------------------------------------------------
    def initialize(self, z, cov0=None):
        self.z = np.array(z, dtype=np.float64).copy()
        self.mu = np.zeros(self.D)
        if cov0 is None:
            s = np.concatenate([self.p.linear_sigma, self.p.angular_sigma] * 2)
            cov0 = np.diag(np.tile(s * s, self.B))
        self.cov = 0.5 * (np.asarray(cov0, float) + np.asarray(cov0, float).T)

    def transition(self):
        """A and Q of the predict step (state order)."""
        D, vf = self.D, self.p.velocity_factor
        A, Q = np.zeros((D, D)), np.zeros((D, D))
        s2 = np.concatenate([self.p.linear_sigma, self.p.angular_sigma]) ** 2
        for b in range(self.B):
            for d in range(6):
                ip, iv = BODY * b + d, BODY * b + d + 6
                A[ip, ip], A[ip, iv], A[iv, iv] = 1.0, vf, vf
                Q[ip, ip] = Q[ip, iv] = Q[iv, ip] = Q[iv, iv] = s2[d]
        return A, Q

    def predict(self, mu, cov):
        A, Q = self.transition()
        S = A @ cov @ A.T + Q
        return A @ mu, 0.5 * (S + S.T)

    def to_pf(self, v, M=None):
        out = np.empty(self.D)
        out[self.perm] = v
        if M is None:
            return out
        Mp = np.empty((self.D, self.D))
        Mp[np.ix_(self.perm, self.perm)] = M
        return out, Mp

    def from_pf(self, v, M):
        return v[self.perm], M[np.ix_(self.perm, self.perm)]

    def sigma_deltas(self, mpf, L):
        """Pose parts [nd, NP] of the distinct sigma points: centre, then +/- sqrt(c) L[:, j] for the pose columns."""
        X = np.repeat(mpf[None, :self.NP], self.nd, axis=0)
        for j in range(self.NP):
            X[1 + 2 * j] += self.sqrtc * L[:self.NP, j]
            X[2 + 2 * j] -= self.sqrtc * L[:self.NP, j]
        return X

    def absolute_poses(self, z, X):
        """Pose deltas [n, NP] (pose-first) around z -> absolute poses [n, parts, 12]."""
        d = X.reshape(-1, self.B, 6)
        zz = z.reshape(self.B, BODY)
        R = rotvec_to_matrix(d[..., 3:6]) @ rotvec_to_matrix(zz[:, 3:6])[None]
        return pack_Rt(R, d[..., 0:3] + zz[None, :, 0:3])

    def pixel_terms(self, depths, y):
        """depths [nd, npx] (+inf uncovered), y [npx] -> per pixel (pi, h [NP, npx], residual, valid)."""
        p = self.p
        fg2, bg2 = p.fg_noise_std ** 2, p.bg_noise_std ** 2
        y = np.asarray(y, dtype=np.float64)
        cov = np.isfinite(depths)
        m = np.where(cov, depths.astype(np.float64), p.bg_depth)
        s = np.where(cov, fg2, bg2)
        extra = 2.0 * self.NP
        yhat = self.wm0 * m[0] + self.w * (m[1:].sum(0) + extra * m[0])
        d0 = m[0] - yhat
        P = self.wc0 * d0 * d0 + self.w * (((m[1:] - yhat) ** 2).sum(0) + extra * d0 * d0) + (self.wm0 * s[0] + self.w * (s[1:].sum(0) + extra * s[0]))
        P = np.maximum(P, fg2)
        h = (m[1::2] - m[2::2]) / (2.0 * self.sqrtc)
        R = np.maximum(P - (h * h).sum(0), fg2)
        valid = np.isfinite(y)
        res = np.where(valid, y - yhat, 0.0)
        b = np.ones_like(P)
        if p.tail_weight > 0.0:
            log_tail = np.log(p.tail_weight / (p.uniform_tail_max - p.uniform_tail_min)) - np.log(1.0 - p.tail_weight)
            inside = valid & (y >= p.uniform_tail_min) & (y <= p.uniform_tail_max)
            with np.errstate(over="ignore"):
                lg = -0.5 * np.log(2.0 * np.pi * P) - 0.5 * res * res / P
                b = np.where(inside, 1.0 / (1.0 + np.exp(log_tail - lg)), 1.0)
        pi = np.where(valid, b / R, 0.0)
        return pi, h, res, valid

    def whitened_update(self, mpf, L, depths, y):
        """-> (mu+ pf, Sigma+ pf, Lambda, eta) from the sigma points' depths."""
        pi, h, res, _ = self.pixel_terms(depths, y)
        Lam = np.eye(self.NP) + (h * pi) @ h.T
        eta = (h * pi) @ res
        zeta = np.linalg.solve(Lam, eta)
        G = np.eye(self.D)
        G[:self.NP, :self.NP] = np.linalg.inv(Lam)
        mup = mpf + L[:, :self.NP] @ zeta
        Sp = L @ G @ L.T
        return mup, 0.5 * (Sp + Sp.T), Lam, eta

    def recentre(self, z, mu):
        z, mu = z.copy().reshape(self.B, BODY), mu.copy().reshape(self.B, BODY)
        for b in range(self.B):
            Rm = rotvec_to_matrix(mu[b, 3:6])
            z[b, 0:3] += mu[b, 0:3]
            z[b, 3:6] = matrix_to_rotvec(Rm @ rotvec_to_matrix(z[b, 3:6]))
            z[b, 6:12] = mu[b, 6:12]
            mu[b, 0:6] = 0.0
        return z.ravel(), mu.ravel()

    # ---- one frame -----------------------------------------------------------------------------------------
    def step(self, z, mu_m, S_m, y, poses=None):
        """From a prior (z, predicted mean, predicted covariance): -> (z+, mu+, Sigma+, sigma poses).
        poses: render these sigma poses instead of the twin's own (teacher forcing on the device's bits)."""
        mpf, Spf = self.to_pf(mu_m, S_m)
        L = np.linalg.cholesky(Spf)
        own = self.absolute_poses(z, self.sigma_deltas(mpf, L))
        use = own if poses is None else poses
        depths = np.stack([self.render(q) for q in use])
        mup, Spp, _, _ = self.whitened_update(mpf, L, depths, y)
        mu, S = self.from_pf(mup, Spp)
        z2, mu2 = self.recentre(z, mu)
        return z2, mu2, S, own

    def track(self, y):
        mu_m, S_m = self.predict(self.mu, self.cov)
        self.z, self.mu, self.cov, _ = self.step(self.z, mu_m, S_m, y)
        return self.z.copy()


def truth_state(truth_Rt):
    """synth.truth_pose rows [parts, 12] (R|t of the centred meshes) -> model-frame state, zero velocities."""
    Rt = np.asarray(truth_Rt).reshape(-1, 12)
    s = np.zeros((Rt.shape[0], BODY))
    for b in range(Rt.shape[0]):
        s[b, 0:3] = Rt[b, 9:12]
        s[b, 3:6] = matrix_to_rotvec(Rt[b, :9].reshape(3, 3))
    return s.ravel()
