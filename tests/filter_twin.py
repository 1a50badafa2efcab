"""A plain reference of the particle filter's device code (dbot_ros_amd/csrc/rbsensor_tracker.hip), one function per
stage, written from the operation and not from the kernels' loop structure: no chunks, no waves, no scans.

  philox4x32_10 / philox_words   the Philox4x32-10 block function (Salmon et al., SC'11; Random123), in Python integers
                                 and, for many counters at once, in numpy uint64 (held to the integer one by the tests)
  u01, device_normals,           the tracker's use of it: counter layout, 53-bit uniforms, Box-Muller
  device_uniforms
  transition                     vel' = vf vel + sigma o n, pose' = pose + vel' for the bodies 0..b (IEEE double, op by op)
  weight_update                  log_w += ll_new - ll (IEEE double, op by op)
  weights_kl_cdf                 softmax, KL(w || uniform) and the running sum, in np.longdouble
  parents_of                     clip(searchsorted(cdf, u, side="right"), 0, n - 1)
  weighted_mean                  math.fsum over extended-precision products
  fold_mean, recentre,           the default-pose update and the re-centring through dbot_ros_amd.pose
  recentred_rotations
  TwinTracker                    the stages chained into the tracker's frame, over any sensor object (the oracle in CPU tests)

Test infrastructure: numpy only, no device."""
import math

import numpy as np

from dbot_ros_amd import pose

BODY = 12
MASK32, MASK64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57        # the two multipliers
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85        # the key schedule's Weyl increments
UNIFORM_KEY_XOR = 0x5BD1E995                           # the resampling stream's key: seed ^ this
TWO_PI = 6.283185307179586

assert np.finfo(np.longdouble).nmant >= 63, "the reference sums need an extended-precision long double"


# ---------------------------------------------------------------- Philox4x32-10
def philox4x32_10(seed, ctr_hi, ctr_lo):
    """Counter (c0, c1, c2, c3) = (ctr_lo low, ctr_lo high, ctr_hi low, ctr_hi high), key (k0, k1) = (seed low, seed high)
    -> the four output words, after ten rounds."""
    k0, k1 = seed & MASK32, (seed >> 32) & MASK32
    c0, c1, c2, c3 = ctr_lo & MASK32, (ctr_lo >> 32) & MASK32, ctr_hi & MASK32, (ctr_hi >> 32) & MASK32
    for _ in range(10):
        p0, p1 = PHILOX_M0 * c0, PHILOX_M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK32, (p0 >> 32) ^ c3 ^ k1, p0 & MASK32
        k0, k1 = (k0 + PHILOX_W0) & MASK32, (k1 + PHILOX_W1) & MASK32
    return c0, c1, c2, c3


def philox_words(seed, ctr_hi, ctr_lo):
    """The same for an array of ctr_lo (uint64) under one seed and one ctr_hi: four uint64 arrays of 32-bit words."""
    lo = np.asarray(ctr_lo, dtype=np.uint64)
    m32 = np.uint64(MASK32)
    s32 = np.uint64(32)
    k0, k1 = seed & MASK32, (seed >> 32) & MASK32
    c0, c1 = lo & m32, lo >> s32
    c2 = np.full(lo.shape, ctr_hi & MASK32, dtype=np.uint64)
    c3 = np.full(lo.shape, (ctr_hi >> 32) & MASK32, dtype=np.uint64)
    for _ in range(10):
        p0, p1 = np.uint64(PHILOX_M0) * c0, np.uint64(PHILOX_M1) * c2     # 32 x 32 bits: no overflow of 64
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ np.uint64(k0), p1 & m32, (p0 >> s32) ^ c3 ^ np.uint64(k1), p0 & m32
        k0, k1 = (k0 + PHILOX_W0) & MASK32, (k1 + PHILOX_W1) & MASK32
    return c0, c1, c2, c3


def u01(hi, lo):
    """The top 53 of the 64 bits hi:lo as a double in [0, 1)."""
    bits = ((np.asarray(hi, dtype=np.uint64) << np.uint64(32)) | np.asarray(lo, dtype=np.uint64)) >> np.uint64(11)
    return bits.astype(np.float64) * 2.0 ** -53


def stream_counter(frame, b):
    """ctr_hi of both streams: the frame number above the sampling block's eight bits (64-bit wrap-around)."""
    return ((frame << 8) | b) & MASK64


def device_normals(seed, frame, b, n):
    """[n][6] standard normals of sampling block b: pair `pr` of particle i from counter (frame << 8 | b, i << 2 | pr),
    Box-Muller on u1 = 1 - u01(words 0, 1) in (0, 1], u2 = u01(words 2, 3)."""
    i = np.arange(n, dtype=np.uint64)
    out = np.empty((n, 6))
    for pr in range(3):
        w = philox_words(seed, stream_counter(frame, b), (i << np.uint64(2)) | np.uint64(pr))
        u1, u2 = 1.0 - u01(w[0], w[1]), u01(w[2], w[3])
        rad = np.sqrt(-2.0 * np.log(u1))
        out[:, 2 * pr] = rad * np.cos(TWO_PI * u2)
        out[:, 2 * pr + 1] = rad * np.sin(TWO_PI * u2)
    return out


def device_uniforms(seed, frame, b, n):
    """[n] resampling uniforms of sampling block b: key seed ^ 0x5bd1e995, counter (frame << 8 | b, j), words 0 and 1."""
    w = philox_words(seed ^ UNIFORM_KEY_XOR, stream_counter(frame, b), np.arange(n, dtype=np.uint64))
    return u01(w[0], w[1])


# ---------------------------------------------------------------- the stages
def transition(part_old, noise, normals_b, b, sigma, vf):
    """Sampling block b restarts from the OLD particles [n][parts*12] and moves the bodies 0..b, body b with this block's
    normals [n][6], the bodies before it with the noise [n][parts][6] they were moved with before.  -> (new particles,
    noise with block b's row filled in).  Every component is a product, a product and a sum, then one more sum."""
    sigma = np.asarray(sigma, dtype=np.float64)
    noise = noise.copy()
    noise[:, b] = normals_b
    new = part_old.copy()
    for bb in range(b + 1):
        s = new[:, BODY * bb: BODY * bb + BODY]
        s[:, 6:12] = vf * s[:, 6:12] + sigma * noise[:, bb]
        s[:, 0:6] = s[:, 0:6] + s[:, 6:12]
    return new, noise


def weight_update(logw, ll, ll_new):
    """-> (log_w + (ll_new - ll), ll_new)."""
    return logw + (ll_new - ll), ll_new.copy()


def weights_kl_cdf(logw):
    """Normalised weights, KL(w || uniform) = log n + sum w log w and the running sum of the weights, in long double."""
    lw = np.asarray(logw, dtype=np.longdouble)
    e = np.exp(lw - lw.max())
    w = e / e.sum()
    pos = w > 0
    kl = np.log(np.longdouble(w.size)) + (w[pos] * np.log(w[pos])).sum()
    return w, kl, np.cumsum(w)


def parents_of(cdf, u):
    """Multinomial resampling: child j descends from the first particle whose cdf exceeds u_j (the last one if none does)."""
    return np.clip(np.searchsorted(cdf, u, side="right"), 0, len(cdf) - 1).astype(np.int32)


def weighted_mean(w, particles):
    """sum_i w_i particle_i per component: the products in long double, each split into two doubles, math.fsum over all."""
    w = np.asarray(w, dtype=np.longdouble)
    out = np.empty(particles.shape[1])
    for c in range(particles.shape[1]):
        t = w * particles[:, c].astype(np.longdouble)
        hi = t.astype(np.float64)
        out[c] = math.fsum(np.concatenate([hi, (t - hi).astype(np.float64)]).tolist())
    return out


def mean_magnitude(w, particles):
    """sum_i |w_i particle_i| per component: what the error of a computed mean scales with."""
    return np.asarray((np.asarray(w, dtype=np.longdouble)[:, None] * np.abs(particles).astype(np.longdouble)).sum(axis=0), dtype=np.float64)


def fold_mean(deflt, mean, parts):
    """The mean delta folded into the default pose: t += t_mean, R <- R(mean) R(default), velocities <- the mean's.
    -> (new default [parts*12], its rotations as matrices [parts][3][3])."""
    z = np.array(deflt, dtype=np.float64).reshape(parts, BODY).copy()
    mu = np.asarray(mean, dtype=np.float64).reshape(parts, BODY)
    R = np.empty((parts, 3, 3))
    for b in range(parts):
        R[b] = pose.rotvec_to_matrix(mu[b, 3:6]) @ pose.rotvec_to_matrix(z[b, 3:6])
        z[b, 0:3] = z[b, 0:3] + mu[b, 0:3]
        z[b, 3:6] = pose.matrix_to_rotvec(R[b])
        z[b, 6:12] = mu[b, 6:12]
    return z.ravel(), R


def recentred_rotations(particles, mean, parts):
    """The re-centred particles' rotations as matrices, R(delta_i) R(mean)^T: [n][parts][3][3]."""
    p = particles.reshape(-1, parts, BODY)
    mu = np.asarray(mean, dtype=np.float64).reshape(parts, BODY)
    RmT = np.swapaxes(pose.rotvec_to_matrix(mu[:, 3:6]), -1, -2)
    return pose.rotvec_to_matrix(p[..., 3:6]) @ RmT[None]


def recentre(particles, mean, parts):
    """delta_i (-) mean: t -= t_mean, R(delta_i) <- R(delta_i) R(mean)^T; velocities stay."""
    out = particles.copy()
    p = out.reshape(-1, parts, BODY)
    mu = np.asarray(mean, dtype=np.float64).reshape(parts, BODY)
    R = recentred_rotations(particles, mean, parts)
    p[..., 0:3] = p[..., 0:3] - mu[None, :, 0:3]
    for i in range(p.shape[0]):
        for b in range(parts):
            p[i, b, 3:6] = pose.matrix_to_rotvec(R[i, b])
    return out


# ---------------------------------------------------------------- the stages chained into the tracker's frame
class TwinTracker:
    """The tracker's frame out of the stages above, over a sensor with set_observation /
    loglikes_poses / reset; model-coordinate states.  Randomness: given arrays, or the device's streams from `seed`."""

    def __init__(self, sensor, n, parts, sigma6, velocity_factor, max_kl, seed=0):
        self.sensor, self.n, self.parts = sensor, n, parts
        self.sigma, self.vf, self.max_kl, self.seed = np.asarray(sigma6, dtype=np.float64), velocity_factor, max_kl, seed
        self.initialize(np.zeros(parts * BODY))

    def initialize(self, default_state):
        self.default = np.array(default_state, dtype=np.float64)
        self.default.reshape(self.parts, BODY)[:, 6:12] = 0.0
        self.particles = np.zeros((self.n, self.parts * BODY))
        self.log_weights, self.loglikes = np.zeros(self.n), np.zeros(self.n)
        self.indices = np.zeros(self.n, dtype=np.int32)
        self.n_resamplings, self.frame, self.decisions = 0, 0, []
        self.sensor.reset()

    def track(self, image, normals=None, uniforms=None):
        n, parts = self.n, self.parts
        self.sensor.set_observation(image)
        old, noise = self.particles, np.zeros((n, parts, 6))
        for b in range(parts):
            nz = normals[b] if normals is not None else device_normals(self.seed, self.frame, b, n)
            new, noise = transition(old, noise, nz, b, self.sigma, self.vf)
            last = b == parts - 1
            idx = self.indices.copy()
            ll_new = self.sensor.loglikes_poses(pose.compose_with_default(new, self.default, parts), idx, update=last)
            if last:
                self.indices = idx
            self.log_weights, self.loglikes = weight_update(self.log_weights, self.loglikes, ll_new)
            _w, kl, cdf = weights_kl_cdf(self.log_weights)
            resample = bool(kl > self.max_kl)
            self.decisions.append(resample)
            if resample:
                u = uniforms[b] if uniforms is not None else device_uniforms(self.seed, self.frame, b, n)
                par = parents_of(cdf, u)
                old, new, noise = old[par], new[par], noise[par]
                self.loglikes, self.indices = self.loglikes[par], self.indices[par]
                self.log_weights = np.zeros(n)
                self.n_resamplings += 1
        w, _kl, _cdf = weights_kl_cdf(self.log_weights)
        mean = weighted_mean(w, new)
        self.default, _R = fold_mean(self.default, mean, parts)
        self.particles = recentre(new, mean, parts)
        self.frame += 1
        return self.default.copy()
