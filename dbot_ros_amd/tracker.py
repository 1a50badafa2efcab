"""Host-side mirror of the callers either side of the hot path ("next" rows):
the object state transition, the Rao-Blackwellised coordinate particle filter loop and the
tracker that the reference node builds and drives

    ObjectTransitionBuilder<State>::Parameters   R:source/dbot_ros/tracker/particle_tracker_node.cpp:138-159
    ParticleTrackerBuilder<Tracker>::Parameters  R:...particle_tracker_node.cpp:208-218
    tracker->initialize(initial_poses)           R:...particle_tracker_node.cpp:252
    tracker_->track(image) -> State              R:source/dbot_ros/object_tracker_ros.hpp:49

restated from SURVEY.md Appendix A.1/A.6 (recalled upstream behaviour; the dbot sources are not
available, so this part is unpinned like the oracle).  The sensor is anything with
set_observation / loglikes_poses / reset (the product's RbSensor, or the oracle in CPU tests).
Randomness comes from a caller-supplied numpy Generator (fl's mt19937 streams cannot be
reproduced without fl).
"""
from dataclasses import dataclass

import numpy as np

from . import filter as flt
from .pose import matrix_to_rotvec, pack_Rt, rotvec_to_matrix

BODY = 12


@dataclass
class Posterior:
    """What a particle tracker knows about its own estimate after a frame (include/rbsensor_mi355x.h, "Posterior report").
    mean [D], cov [D, D]: weighted moments of the re-centred particle deltas, D = 12 per body (position, rotation vector,
    linear and angular velocity), MODEL coordinates: translations add in the camera frame, rotations multiply from the left.
    ess: effective sample size; survivors: distinct occlusion slots among the particles; resampled: the frame's last
    sampling block resampled; n: particles; frame: frames tracked since initialize."""
    mean: np.ndarray
    cov: np.ndarray
    ess: float
    survivors: int
    resampled: bool
    n: int
    frame: int = 0


def posterior_of(particles, log_weights, indices, resampled=False, frame=0):
    """The rule of the posterior report in numpy -- the restatement the device kernels (csrc/rbsensor_posterior.hip) are
    tested against.  particles [n, D] re-centred deltas, log_weights [n] (-inf: no contribution), indices [n].
    Two passes: the mean, then central moments; the upper triangle mirrored."""
    x = np.asarray(particles, dtype=np.float64)
    x = x.reshape(x.shape[0], -1)
    lw = np.asarray(log_weights, dtype=np.float64)
    e = np.exp(lw - lw.max())
    S = e.sum()
    mean = (e[:, None] * x).sum(axis=0) / S
    d = x - mean
    full = (e[:, None] * d).T @ d / S
    cov = np.triu(full) + np.triu(full, 1).T
    return Posterior(mean=mean, cov=cov, ess=float(S * S / (e * e).sum()), survivors=int(np.unique(np.asarray(indices)).size),
                     resampled=bool(resampled), n=int(x.shape[0]), frame=int(frame))


MODES_MAX = 8
MODES_E_MIN = 2.0 ** -960     # e_i below it counts as 0 (include/rbsensor_mi355x.h, "Posterior modes")


@dataclass
class ModesParams:
    """Parameters of the posterior modes (include/rbsensor_mi355x.h, "Posterior modes").  The defaults are starting values,
    UNMEASURED: a few transition sigmas wide, not tuned on data."""
    h_t: float = 0.02          # translation bandwidth, metres (> 0)
    h_r: float = 0.2           # rotation bandwidth, radians (0 < h_r <= 1)
    separation: float = 2.0    # suppression radius in bandwidths (>= 1)
    k_max: int = 4             # most modes returned per body (1 .. 8)

    def check(self):
        if not (self.h_t > 0 and np.isfinite(self.h_t)):
            raise ValueError("modes: h_t must be positive")
        if not 0 < self.h_r <= 1:
            raise ValueError("modes: h_r must lie in (0, 1]")
        if not (self.separation >= 1 and np.isfinite(self.separation)):
            raise ValueError("modes: separation must be at least 1")
        if not (1 <= int(self.k_max) <= MODES_MAX and int(self.k_max) == self.k_max):
            raise ValueError("modes: k_max outside 1..8")
        return self

    @classmethod
    def from_rosparam(cls, tree):
        """The optional key particle_filter/modes: true (the defaults), or a mapping of any of the four parameters; None
        where the key is absent or false -- the reference's YAML files parse unchanged, the report off."""
        v = tree.get("particle_filter", {}).get("modes", None)
        if v is None or v is False:
            return None
        if v is True:
            return cls()
        unknown = set(v) - {"h_t", "h_r", "separation", "k_max"}
        if unknown:
            raise ValueError(f"particle_filter/modes: unknown keys {sorted(unknown)}")
        return cls(h_t=float(v.get("h_t", cls.h_t)), h_r=float(v.get("h_r", cls.h_r)), separation=float(v.get("separation", cls.separation)),
                   k_max=int(v.get("k_max", cls.k_max))).check()


@dataclass
class Mode:
    """One mode of one body: seed (particle index), density (rho at the seed), mass (share of the belief assigned to the mode),
    core_mass (... within one bandwidth of the seed), delta [6] (the core's mean position and rotation-vector delta, re-centred
    MODEL coordinates), pose [6] (the published position and rotation vector of that body were this mode the estimate: the
    delta composed with the frame's state as the tracker publishes it; None where no state is known)."""
    seed: int
    density: float
    mass: float
    core_mass: float
    delta: np.ndarray
    pose: np.ndarray = None


@dataclass
class Modes:
    """bodies: per body the list of its Modes in selection order; frame: frames tracked since initialize (0: stateless)."""
    bodies: list
    frame: int = 0


def _quaternions(r):
    """[n, 3] rotation vectors -> [n, 4] unit quaternions (w, x, y, z); (1, 0, 0, 0) at r = 0 (pose.rotvec_to_matrix's form)."""
    angle = np.sqrt(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2])
    half = 0.5 * angle
    small = angle < 1e-9
    k = np.where(small, 0.5 - angle * angle / 48.0, np.sin(half) / np.where(small, 1.0, angle))
    return np.concatenate([np.cos(half)[:, None], r * k[:, None]], axis=1)


def modes_of(particles, log_weights, params=None, frame=0, block=512):
    """The rule of the posterior modes in numpy -- the restatement the device kernels (csrc/rbsensor_modes.hip) are tested
    against.  particles [n, parts, >= 6] or [n, parts * 12] (or [n, parts * 6]) re-centred deltas, log_weights [n] (-inf: no
    contribution).  The pair pass is row-blocked (block rows at a time) to bound memory."""
    P = (params or ModesParams()).check()
    lw = np.asarray(log_weights, dtype=np.float64).ravel()
    n = lw.size
    x = np.asarray(particles, dtype=np.float64)
    if x.ndim == 2:
        w = BODY if x.shape[1] % BODY == 0 else 6
        x = x.reshape(n, x.shape[1] // w, w)
    with np.errstate(under="ignore"):
        e = np.exp(lw - lw.max())
    e = np.where(e < MODES_E_MIN, 0.0, e)
    S = e.sum()
    c4, sep2 = 4.0 / (P.h_r * P.h_r), P.separation * P.separation

    def d2(pa, qa, pb, qb):          # [a, 1, .] against [1, b, .] -> [a, b]
        d = pa - pb
        c = (qa * qb).sum(-1)
        return (d * d).sum(-1) + c4 * (1.0 - c * c)

    bodies = []
    for b in range(x.shape[1]):
        p, q = x[:, b, 0:3] / P.h_t, _quaternions(x[:, b, 3:6])
        rho = np.empty(n)
        # (two-dimensional temporaries, d2's operations component by component, and no matrix product: every row goes through the
        #  same sequence of operations, so particles with the same pose get the same rho bit for bit and tie by index)
        for lo in range(0, n, block):
            pb, qb = p[lo:lo + block], q[lo:lo + block]
            d, c = np.zeros((len(pb), n)), np.zeros((len(pb), n))
            for k in range(3):
                t = pb[:, k, None] - p[None, :, k]
                d += t * t
            for k in range(4):
                c += qb[:, k, None] * q[None, :, k]
            k = 1.0 - (d + c4 * (1.0 - c * c))
            rho[lo:lo + block] = (np.maximum(k, 0.0) * e[None]).sum(1) / S
        cand = e > 0
        seeds = []
        while len(seeds) < P.k_max and cand.any():
            s = int(np.argmax(np.where(cand, rho, -1.0)))       # (argmax: the lowest index on a tie)
            seeds.append(s)
            cand &= ~(d2(p, q, p[s][None], q[s][None]) < sep2)
        D = np.stack([d2(p, q, p[s][None], q[s][None]) for s in seeds], axis=1)
        near = np.argmin(D, axis=1)                             # (argmin: the earlier mode on a tie)
        out = []
        for k, s in enumerate(seeds):
            member = (near == k) & (e > 0)
            core = member & (D[:, k] < 1.0)
            ec = e[core]
            sign = np.where((q[core] * q[s][None]).sum(-1) < 0.0, -1.0, 1.0)
            qm = ((ec * sign)[:, None] * q[core]).sum(0) / ec.sum()    # (of order 1 whatever the weights' scale: no underflow below)
            qm = qm / np.sqrt((qm * qm).sum())
            if qm[0] < 0.0:
                qm = -qm
            vn = np.sqrt((qm[1:] * qm[1:]).sum())
            rot = qm[1:] * (2.0 * np.arctan2(vn, qm[0]) / vn) if vn > 0.0 else np.zeros(3)
            pos = (ec[:, None] * p[core]).sum(0) / ec.sum() * P.h_t
            out.append(Mode(seed=s, density=float(rho[s]), mass=float(e[member].sum() / S), core_mass=float(ec.sum() / S),
                            delta=np.concatenate([pos, rot])))
        bodies.append(out)
    return Modes(bodies=bodies, frame=int(frame))


@dataclass
class OcclusionMap:
    """What a particle tracker believes is occluded after a frame (include/rbsensor_mi355x.h, "Occlusion map"): plane
    [rows, cols] float32, the weighted mean of the particles' occlusion planes; frame: frames tracked since initialize."""
    plane: np.ndarray
    frame: int = 0


@dataclass
class ObjectMap:
    """Where a particle tracker sees the object after a frame (include/rbsensor_mi355x.h, "Object map"): cover
    [n_bodies, rows, cols] float32, the probability per body that it is what the camera sees at the pixel; depth
    [rows, cols], the posterior mean of the rendered depth (+inf: no surface); var [rows, cols], its variance; frame:
    frames tracked since initialize."""
    cover: np.ndarray
    depth: np.ndarray
    var: np.ndarray
    frame: int = 0


@dataclass
class Segmentation:
    """A depth frame segmented against an ObjectMap (rbs_object_segment): labels [rows, cols] int32, the body or -1;
    counts [n_bodies]; pixel [c] the labelled pixels in ascending index; xyz [c, 3] their points in camera coordinates."""
    labels: np.ndarray
    counts: np.ndarray
    pixel: np.ndarray
    xyz: np.ndarray


@dataclass
class BodyOcclusion:
    """One body's share of an occlusion map at a pose: pixels the body owns, those of them above the threshold, and the
    mean of the map over them (nan when the body owns no pixel)."""
    rendered: int
    occluded: int
    mean: float


def occlusion_map_of(planes_by_slot, log_weights, indices):
    """The rule of the occlusion map in numpy -- the restatement the device kernels (csrc/rbsensor_occmap.hip) are tested
    against, in np.longdouble (binary64 where the platform has nothing wider).  planes_by_slot: {slot: plane} or an array
    [slots, npx] of the planes rbs_get_occlusion hands out; log_weights [n] (None: uniform; -inf: no contribution);
    indices [n].  Returns M [npx] as longdouble, not rounded to float."""
    idx = np.asarray(indices).astype(np.int64).ravel()
    LD = np.longdouble
    if log_weights is None:
        e = np.ones(idx.size, dtype=LD)
    else:
        lw = np.asarray(log_weights, dtype=np.float64).ravel()
        e = np.exp((lw - lw.max()).astype(LD))
    S = e.sum()
    acc = None
    for s in np.unique(idx):
        W = e[idx == s].sum()
        if not W > 0:
            continue
        term = W * np.asarray(planes_by_slot[int(s)], dtype=np.float32).ravel().astype(LD)
        acc = term if acc is None else acc + term
    return acc / S


def object_map_of(planes, rects, members, log_weights):
    """The rule of the object map in numpy -- the restatement the device kernels (csrc/rbsensor_objmap.hip) are tested
    against, in np.longdouble.  planes [m, B, rows, cols] float32: body b of pose k alone (+inf: no surface), valid inside
    rects [m, B, 4] (x0, y0, x1, y1); members [n] pose indices (None: the identity); log_weights [n] (None: uniform; -inf: no
    contribution).  Returns (cover [B, npx], depth [npx], var [npx], a [npx], S) as longdouble, not rounded to float;
    depth = +inf and var = 0 where a = 0."""
    LD = np.longdouble
    P = np.asarray(planes, dtype=np.float32)
    if P.ndim != 4:
        raise ValueError("object_map_of: planes must be [m, B, rows, cols]")
    m, B, rows, cols = P.shape
    npx = rows * cols
    idx = np.arange(m) if members is None else np.asarray(members).astype(np.int64).ravel()
    if log_weights is None:
        e = np.ones(idx.size, dtype=LD)
    else:
        lw = np.asarray(log_weights, dtype=np.float64).ravel()
        e = np.exp((lw - lw.max()).astype(LD))
    S = e.sum()
    R = np.asarray(rects).reshape(m, B, -1)
    yy, xx = np.mgrid[0:rows, 0:cols]
    c = np.zeros((B, rows, cols), dtype=LD)
    s1 = np.zeros((rows, cols), dtype=LD)
    s2 = np.zeros((rows, cols), dtype=LD)
    for k in np.unique(idx):
        W = e[idx == k].sum()
        if not W > 0:
            continue
        best = np.full((rows, cols), np.inf, dtype=np.float32)
        owner = np.full((rows, cols), -1, dtype=np.int64)
        for b in range(B):   # ascending, strictly nearer: a tie stays with the lowest body
            x0, y0, x1, y1 = (int(v) for v in R[k, b, :4])
            inside = (xx >= x0) & (xx < x1) & (yy >= y0) & (yy < y1)
            nearer = inside & (P[k, b] < best)
            best = np.where(nearer, P[k, b], best)
            owner = np.where(nearer, b, owner)
        d = np.where(owner >= 0, best, np.float32(0)).astype(LD)
        for b in range(B):
            c[b] += np.where(owner == b, W, LD(0))
        s1 += np.where(owner >= 0, W * d, LD(0))
        s2 += np.where(owner >= 0, W * (d * d), LD(0))
    a = c.sum(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        mu = np.where(a > 0, s1 / np.where(a > 0, a, 1), LD(np.inf))
        var = np.where(a > 0, np.maximum(s2 / np.where(a > 0, a, 1) - np.where(a > 0, mu, 0) ** 2, 0), LD(0))
    return (c / S).reshape(B, npx), mu.reshape(npx), var.reshape(npx), a.reshape(npx), S


def segment_of(cover, depth, var, y, K, model_sigma, sigma_factor, min_cover=0.5, sigmas=3.0, depth_sigmas=3.0):
    """The segmentation rule in numpy (binary64, exactly the device's operations): cover [B, rows, cols], depth, var and the
    observation y [rows, cols] float32; K the 3 x 3 camera matrix.  Returns (labels int32 [rows*cols], counts [B],
    pixel int32 [c], xyz float32 [c, 3])."""
    cov = np.asarray(cover, dtype=np.float32)
    B, rows, cols = cov.shape
    D = np.asarray(depth, dtype=np.float32).reshape(rows, cols).astype(np.float64)
    v = np.asarray(var, dtype=np.float32).reshape(rows, cols).astype(np.float64)
    yf = np.asarray(y, dtype=np.float32).reshape(rows, cols)
    best = np.argmax(cov, axis=0)          # (the first maximum: a tie stays with the lowest body)
    top = np.take_along_axis(cov, best[None], 0)[0].astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        tau = float(sigmas) * (float(model_sigma) + float(sigma_factor) * (D * D))
        ex = np.maximum(0.0, np.abs(yf.astype(np.float64) - D) - tau)
        ok = (top >= float(min_cover)) & np.isfinite(yf) & np.isfinite(D) & (ex * ex <= (float(depth_sigmas) * float(depth_sigmas)) * v)
    labels = np.where(ok, best, -1).astype(np.int32).ravel()
    counts = np.array([(labels == b).sum() for b in range(B)], dtype=np.int32)
    pixel = np.nonzero(labels >= 0)[0].astype(np.int32)
    K = np.asarray(K, dtype=np.float64).reshape(3, 3)
    z = yf.ravel()[pixel]
    x, yy = (pixel % cols).astype(np.float64), (pixel // cols).astype(np.float64)
    X = ((x - K[0, 2]) / K[0, 0] * z.astype(np.float64)).astype(np.float32)
    Y = ((yy - K[1, 2]) / K[1, 1] * z.astype(np.float64)).astype(np.float32)
    return labels, counts, pixel, np.stack([X, Y, z], axis=-1).astype(np.float32).reshape(-1, 3)


def object_frame_jacobian(R, c):
    """d(published pose) / d(model pose), 6 x 6, to first order.  With center_object_frame the published position is
    p = t - R c (R: the body's absolute rotation, c: its centring offset); a model perturbation (dt, dtheta) -- dtheta
    from the left, R' = R(dtheta) R -- moves it by dp = dt + [R c]x dtheta and turns the published rotation by dtheta."""
    v = np.asarray(R, dtype=np.float64) @ np.asarray(c, dtype=np.float64)
    J = np.eye(6)
    J[0:3, 3:6] = np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])
    return J


class ObjectTransitionBuilder:
    @dataclass
    class Parameters:
        linear_sigma_x: float = 0.0025
        linear_sigma_y: float = 0.0025
        linear_sigma_z: float = 0.0025
        angular_sigma_x: float = 0.02
        angular_sigma_y: float = 0.02
        angular_sigma_z: float = 0.02
        velocity_factor: float = 0.8
        part_count: int = 1

        @classmethod
        def from_rosparam(cls, tree, part_count):
            t = tree["particle_filter"]["object_transition"]
            return cls(*(float(t[k]) for k in ("linear_sigma_x", "linear_sigma_y", "linear_sigma_z",
                                               "angular_sigma_x", "angular_sigma_y", "angular_sigma_z",
                                               "velocity_factor")), part_count=part_count)

    def __init__(self, params):
        self.params = params

    def build(self):
        return ObjectTransition(self.params)


class ObjectTransition:
    """Random walk on the velocities (R:config/particle_tracker.yaml:51-63): per body and per
    frame, with 6 standard normals n = (n_lin, n_ang):
        vel'  = velocity_factor * vel + sigma o n
        pose' = pose + vel'."""

    def __init__(self, p):
        self.vf = p.velocity_factor
        self.sigma = np.array([p.linear_sigma_x, p.linear_sigma_y, p.linear_sigma_z,
                               p.angular_sigma_x, p.angular_sigma_y, p.angular_sigma_z])
        self.part_count = p.part_count

    def apply(self, states, noise, body):
        """states [n, parts*12] (not modified), noise [n, 6] for `body` -> new states."""
        out = states.copy()
        s = out[:, BODY * body: BODY * body + BODY]
        s[:, 6:12] = self.vf * s[:, 6:12] + self.sigma * noise
        s[:, 0:6] = s[:, 0:6] + s[:, 6:12]
        return out


class ParticleTrackerBuilder:
    @dataclass
    class Parameters:
        evaluation_count: int = 2000
        moving_average_update_rate: float = 1.0
        max_kl_divergence: float = 2.0
        center_object_frame: bool = True

        @classmethod
        def from_rosparam(cls, tree, evaluation_count):
            pf = tree["particle_filter"]
            return cls(int(evaluation_count), float(pf["moving_average_update_rate"]),
                       float(pf["max_kl_divergence"]), bool(pf["center_object_frame"]))

    def __init__(self, transition_builder, sensor_builder, object_model, params):
        self.transition_builder, self.sensor_builder = transition_builder, sensor_builder
        self.object_model, self.params = object_model, params

    def build(self, rng=None):
        return ParticleTracker(self.transition_builder.build(), self.sensor_builder.build(),
                               self.object_model, self.params, rng)


class ParticleTracker:
    """dbot::ParticleTracker mirror: one sampling block per object, particle count =
    evaluation_count / #blocks."""

    def __init__(self, transition, sensor, object_model, params, rng=None):
        self.transition, self.sensor, self.params = transition, sensor, params
        self.parts = object_model.count_parts
        self.centers = np.array(object_model.centers)  # mesh re-centring offsets (center_object_frame)
        self.n = max(1, params.evaluation_count // self.parts)
        self.rng = rng if rng is not None else np.random.default_rng(0)
        self.default = np.zeros(self.parts * BODY)       # integrated pose the deltas live around
        self.particles = np.zeros((self.n, self.parts * BODY))
        self.log_weights = np.zeros(self.n)
        self.loglikes = np.zeros(self.n)
        self.indices = np.zeros(self.n, dtype=np.int32)
        self.moving_average = None
        self.n_resamplings = 0
        self._resampled, self._frames = False, 0

    # -- State <-> model coordinates ---------------------------------------------------------
    def _to_model(self, state):
        """Camera-frame pose of the ORIGINAL mesh frame -> pose of the centred mesh frame."""
        s = np.array(state, dtype=np.float64).reshape(self.parts, BODY).copy()
        if self.params.center_object_frame:
            for b in range(self.parts):
                s[b, 0:3] += rotvec_to_matrix(s[b, 3:6]) @ self.centers[b]
        return s.ravel()

    def _from_model(self, state):
        s = np.array(state, dtype=np.float64).reshape(self.parts, BODY).copy()
        if self.params.center_object_frame:
            for b in range(self.parts):
                s[b, 0:3] -= rotvec_to_matrix(s[b, 3:6]) @ self.centers[b]
        return s.ravel()

    # -- Tracker interface -------------------------------------------------------------------
    def initialize(self, initial_states):
        """initial_states: list of State vectors (parts*12); the first is used as the default
        pose, particles start as zero deltas (R:...particle_tracker_node.cpp:242-252)."""
        self.default = self._to_model(initial_states[0])
        self.default.reshape(self.parts, BODY)[:, 6:12] = 0.0
        self.particles[:] = 0.0
        self.log_weights[:] = 0.0
        self.loglikes[:] = 0.0
        self.indices[:] = 0
        self.moving_average = None
        self._resampled, self._frames = False, 0
        self.sensor.reset()

    def absolute_poses(self, particles):
        d = particles.reshape(-1, self.parts, BODY)
        z = self.default.reshape(self.parts, BODY)
        R = rotvec_to_matrix(d[..., 3:6]) @ rotvec_to_matrix(z[:, 3:6])[None]
        return pack_Rt(R, d[..., 0:3] + z[None, :, 0:3])

    def draw_randomness(self):
        """Per frame: standard normals [parts, n, 6] and uniforms [parts, n], drawn
        unconditionally so host and device trackers consume identical streams."""
        return (self.rng.standard_normal((self.parts, self.n, 6)), self.rng.random((self.parts, self.n)))

    def track(self, image, normals=None, uniforms=None):
        """One depth frame -> estimated State (camera-frame poses + velocities per object)."""
        if normals is None or uniforms is None:
            normals, uniforms = self.draw_randomness()
        self.sensor.set_observation(image)
        old = self.particles
        noises = np.zeros((self.n, self.parts, 6))
        new = old
        for b in range(self.parts):
            noises[:, b] = normals[b]
            # every block restarts from the SAME old particles; noise accumulates over blocks
            new = old
            for bb in range(b + 1):
                new = self.transition.apply(new, noises[:, bb], bb)
            last = b == self.parts - 1
            idx = self.indices.copy()
            new_ll = self.sensor.loglikes_poses(self.absolute_poses(new), idx, update=last)
            if last:
                self.indices = idx
            self.log_weights += new_ll - self.loglikes
            self.loglikes = new_ll
            w = flt.normalized_weights(self.log_weights)
            self._resampled = bool(flt.kl_to_uniform(w) > self.params.max_kl_divergence)
            if self._resampled:
                parents = flt.multinomial_resample(w, uniforms[b])
                self.n_resamplings += 1
                self.indices = self.indices[parents].copy()
                old, new, noises = old[parents], new[parents], noises[parents]
                self.loglikes = self.loglikes[parents]
                self.log_weights = np.zeros(self.n)
        self.particles = new
        # fold the weighted mean delta into the default pose and re-centre the particles
        w = flt.normalized_weights(self.log_weights)
        mean = flt.weighted_mean(w, self.particles).reshape(self.parts, BODY)
        z = self.default.reshape(self.parts, BODY)
        p = self.particles.reshape(self.n, self.parts, BODY)
        for b in range(self.parts):
            Rm = rotvec_to_matrix(mean[b, 3:6])
            z[b, 0:3] += mean[b, 0:3]
            z[b, 3:6] = matrix_to_rotvec(Rm @ rotvec_to_matrix(z[b, 3:6]))
            z[b, 6:12] = mean[b, 6:12]
            p[:, b, 0:3] -= mean[b, 0:3]
            Rd = rotvec_to_matrix(p[:, b, 3:6]) @ Rm.T
            p[:, b, 3:6] = _rotvecs(Rd)
        self._frames += 1
        est = self._from_model(self.default)
        rate = self.params.moving_average_update_rate
        self.moving_average = est if self.moving_average is None else rate * est + (1 - rate) * self.moving_average
        return self.moving_average.copy()

    # -- the spread of the last estimate -------------------------------------------------------
    def posterior(self):
        """Posterior of the population the last frame left behind (posterior_of on this tracker's own arrays)."""
        if self._frames == 0:
            raise ValueError("posterior: no frame has been tracked since initialize")
        return posterior_of(self.particles, self.log_weights, self.indices, self._resampled, self._frames)

    def modes(self, params=None):
        """The modes of the population the last frame left behind (modes_of on this tracker's own arrays), each with its
        published pose."""
        if self._frames == 0:
            raise ValueError("modes: no frame has been tracked since initialize")
        return self._with_poses(modes_of(self.particles, self.log_weights, params, self._frames), self.default)

    def _with_poses(self, modes, default):
        """Fill Mode.pose: the mode's delta composed with the MODEL state `default` (translations add, rotations multiply from
        the left) and converted to the published frame as _from_model does."""
        z = np.asarray(default, dtype=np.float64).reshape(self.parts, BODY)
        for b, body in enumerate(modes.bodies):
            for m in body:
                s = z.copy()
                s[b, 0:3] += m.delta[0:3]
                s[b, 3:6] = matrix_to_rotvec(rotvec_to_matrix(m.delta[3:6]) @ rotvec_to_matrix(z[b, 3:6]))
                m.pose = self._from_model(s.ravel()).reshape(self.parts, BODY)[b, 0:6].copy()
        return modes

    def pose_covariance(self, posterior):
        """[parts, 6, 6]: per body the covariance of the PUBLISHED pose (position, rotation; camera frame, left
        perturbation) -- J C J^T with object_frame_jacobian when center_object_frame moves the published position to
        t - R c, the model block itself otherwise.  R is taken from the last estimate (self.default)."""
        z = self.default.reshape(self.parts, BODY)
        out = np.empty((self.parts, 6, 6))
        for b in range(self.parts):
            C = posterior.cov[BODY * b:BODY * b + 6, BODY * b:BODY * b + 6]
            if self.params.center_object_frame:
                J = object_frame_jacobian(rotvec_to_matrix(z[b, 3:6]), self.centers[b])
                C = J @ C @ J.T
            out[b] = C
        return out

    # -- what the filter believes is occluded ---------------------------------------------------
    def occlusion_map(self):
        """OcclusionMap of the population the last frame left behind: sensor.occlusion_mean with this tracker's own
        weights and slot map."""
        if self._frames == 0:
            raise ValueError("occlusion_map: no frame has been tracked since initialize")
        plane = self.sensor.occlusion_mean(self.indices, self.log_weights)
        return OcclusionMap(plane=plane.reshape(self.sensor.rows, self.sensor.cols), frame=self._frames)

    def occlusion_of_estimate(self, threshold=0.5):
        """Per body a BodyOcclusion: the last frame's occlusion map summarised over the pixels each body owns at the
        published estimate (sensor.occlusion_bodies; center_object_frame undone as assess() undoes it)."""
        from .assess import state_poses
        if self.moving_average is None:
            raise ValueError("occlusion_of_estimate: no frame tracked yet")
        rec = self.sensor.occlusion_bodies(self.occlusion_map().plane, state_poses(self, self.moving_average), threshold)[0]
        return [BodyOcclusion(rendered=int(r), occluded=int(o), mean=float(q) / 2.0 ** 32 / int(r) if r else float("nan"))
                for r, o, q in rec]

    # -- where the filter sees the object ---------------------------------------------------------
    def poses(self):
        """[n, parts, 12]: the absolute pose of every member of the population the last frame left behind."""
        if self._frames == 0:
            raise ValueError("poses: no frame has been tracked since initialize")
        return self.absolute_poses(self.particles)

    def object_map(self):
        """ObjectMap of the population the last frame left behind: sensor.object_map over poses() with this tracker's own
        weights."""
        cover, depth, var = self.sensor.object_map(self.poses(), None, self.log_weights)
        r, c = self.sensor.rows, self.sensor.cols
        return ObjectMap(cover=cover.reshape(-1, r, c), depth=depth.reshape(r, c), var=var.reshape(r, c), frame=self._frames)

    def segment(self, params=None, object_map=None):
        """Segmentation of the sensor's current observation against `object_map` (None: self.object_map())
        (sensor.object_segment; params: a dict with any of min_cover, sigmas, depth_sigmas).  The observation is the frame
        handed over last: with frames in flight that is a later frame than the map's, so segment frame by frame."""
        m = self.object_map() if object_map is None else object_map
        labels, counts, pixel, xyz, _ = self.sensor.object_segment((m.cover, m.depth, m.var), params)
        return Segmentation(labels=labels.reshape(self.sensor.rows, self.sensor.cols), counts=counts, pixel=pixel, xyz=xyz)

    # -- the last estimate judged against its frame (dbot_ros_amd/assess.py) -------------------
    _in_flight = 0   # frames submitted and not yet collected (the device trackers' submit / result)

    def assess(self, frame=None, assessor=None):
        """The last estimate judged against `frame` (None: the sensor's current observation) -> assess.Assessment of one
        pose.  assessor: a PoseAssessor over the same sensor (None: one with the default parameters, kept).  With frames
        in flight (submit / result) the frame must be given: ValueError otherwise."""
        from . import assess as _assess
        if assessor is None:
            assessor = getattr(self, "_assessor", None)
            if assessor is None:
                assessor = self._assessor = _assess.PoseAssessor(self.sensor)
        return _assess.assess_last_estimate(self, assessor, frame, self._in_flight > 0)

    def refine(self, frame=None, refiner=None):
        """The last estimate refined against `frame` (None: the sensor's current observation) -> (State,
        refine.Refinement of one pose).  refiner: a PoseRefiner over the same sensor (None: one with the default
        parameters, kept).  The filter is not touched: the next frame's estimate is what it would have been.  With
        frames in flight the frame must be given: ValueError otherwise."""
        from . import refine as _refine
        if refiner is None:
            refiner = getattr(self, "_refiner", None)
            if refiner is None:
                refiner = self._refiner = _refine.PoseRefiner(self.sensor)
        return _refine.refine_last_estimate(self, refiner, frame, self._in_flight > 0)


def modes_params_c(params):
    """A ModesParams as the C-ABI's rbs_modes_params (unchecked: the library refuses what is out of range)."""
    from . import _capi
    c = _capi.RbsModesParams()
    c.h_t, c.h_r, c.separation, c.k_max, c.reserved = float(params.h_t), float(params.h_r), float(params.separation), int(params.k_max), 0
    return c


def modes_from_c(rec, frame=0):
    """An array of rbs_body_modes -> Modes (poses unfilled)."""
    return Modes(bodies=[[Mode(seed=int(m.seed), density=float(m.density), mass=float(m.mass), core_mass=float(m.core_mass),
                               delta=np.array(m.delta[:], dtype=np.float64)) for m in body.mode[:body.n_modes]] for body in rec],
                 frame=int(frame))


def _rotvecs(R):
    """Vectorised matrix -> rotation vector (atan2 form; particle deltas are far from pi)."""
    s = 0.5 * np.stack([R[:, 2, 1] - R[:, 1, 2], R[:, 0, 2] - R[:, 2, 0], R[:, 1, 0] - R[:, 0, 1]], -1)
    sn = np.linalg.norm(s, axis=-1)
    cs = 0.5 * (np.trace(R, axis1=1, axis2=2) - 1.0)
    ang = np.arctan2(sn, cs)
    k = np.where(sn > 1e-8, ang / np.where(sn > 1e-8, sn, 1.0), 1.0)
    out = s * k[:, None]
    flip = (sn <= 1e-8) & (cs <= 0.0)      # angle ~ pi: axis from the symmetric part (pose.matrix_to_rotvec)
    for i in np.nonzero(flip)[0]:
        out[i] = matrix_to_rotvec(R[i])
    return out


class DeviceParticleTracker(ParticleTracker):
    """Same interface, but the transition, filter step and mean run on the sensor's device
    (rbs_tracker_* in librbsensor_mi355x.so): one host synchronisation per frame.  With
    device_rng=True the normals/uniforms are drawn on the device (Philox), otherwise they come
    from this object's numpy Generator exactly as in the host tracker."""

    def __init__(self, transition, sensor, object_model, params, rng=None, device_rng=False, seed=0, posterior=False,
                 occlusion_map=False, object_map=False, modes=None):
        import ctypes as C
        from . import _capi
        super().__init__(transition, sensor, object_model, params, rng)
        self._C, self._capi = C, _capi
        self._lib = _capi.load()
        self.device_rng, self.seed = device_rng, seed
        tp = _capi.RbsTrackerParams()
        tp.linear_sigma = (C.c_double * 3)(*transition.sigma[:3])
        tp.angular_sigma = (C.c_double * 3)(*transition.sigma[3:])
        tp.velocity_factor = transition.vf
        tp.max_kl_divergence = params.max_kl_divergence
        tp.n_particles = self.n
        self._t = C.c_void_p()
        rc = self._lib.rbs_tracker_create(sensor._h, C.byref(tp), C.byref(self._t))
        if rc != 0:
            sensor._check(rc)
        sensor._register_dependent(self)   # the C tracker borrows the sensor handle
        if posterior:
            self.set_posterior(True)
        if occlusion_map:
            self.set_occlusion_map(True)
        if object_map:
            self.set_object_map(True)
        if modes is not None and modes is not False:
            self.set_modes(ModesParams() if modes is True else modes)

    def set_posterior(self, enable):
        """Switch the device's posterior report on or off (rbs_tracker_set_posterior; refused with frames in flight)."""
        self.sensor._check(self._lib.rbs_tracker_set_posterior(self._t, 1 if enable else 0))

    def posterior(self):
        """The report of the frame most recently handed out by track() / result() (rbs_tracker_posterior), reduced on
        the device; needs posterior=True (or set_posterior(True)) -- an RbSensorError otherwise."""
        C = self._C
        D = self.parts * BODY
        info = self._capi.RbsTrackerPosteriorInfo()
        mean, cov = np.empty(D), np.empty((D, D))
        dp = C.POINTER(C.c_double)
        self.sensor._check(self._lib.rbs_tracker_posterior(self._t, C.byref(info), mean.ctypes.data_as(dp), cov.ctypes.data_as(dp)))
        return Posterior(mean=mean, cov=cov, ess=float(info.ess), survivors=int(info.survivors), resampled=bool(info.resampled),
                         n=int(info.n), frame=int(info.frame))

    def posterior_ms(self):
        """Device time of the last report's kernels in milliseconds (rbs_tracker_posterior_ms)."""
        ms = self._C.c_float()
        self.sensor._check(self._lib.rbs_tracker_posterior_ms(self._t, self._C.byref(ms)))
        return float(ms.value)

    def set_modes(self, params):
        """Switch the device's posterior modes on with `params` (a ModesParams; True: the defaults) or off (None / False)
        (rbs_tracker_set_modes; refused with frames in flight)."""
        if params is None or params is False:
            self.sensor._check(self._lib.rbs_tracker_set_modes(self._t, None))
            return
        self.sensor._check(self._lib.rbs_tracker_set_modes(self._t, self._C.byref(modes_params_c(ModesParams() if params is True else params))))

    def modes(self):
        """The Modes of the frame most recently handed out by track() / result() (rbs_tracker_modes), found on the device;
        needs modes=... (or set_modes()) -- an RbSensorError otherwise.  Each Mode carries its published pose: the delta
        composed with that frame's state."""
        C = self._C
        frame = C.c_int32()
        rec = (self._capi.RbsBodyModes * self.parts)()
        self.sensor._check(self._lib.rbs_tracker_modes(self._t, C.byref(frame), rec))
        return self._with_poses(modes_from_c(rec, int(frame.value)), self.default)

    def modes_ms(self):
        """Device time of the last modes report's kernels in milliseconds (rbs_tracker_modes_ms)."""
        ms = self._C.c_float()
        self.sensor._check(self._lib.rbs_tracker_modes_ms(self._t, self._C.byref(ms)))
        return float(ms.value)

    def set_occlusion_map(self, enable):
        """Switch the device's occlusion map on or off (rbs_tracker_set_occlusion_map; refused with frames in flight)."""
        self.sensor._check(self._lib.rbs_tracker_set_occlusion_map(self._t, 1 if enable else 0))

    def occlusion_map(self):
        """The map of the frame most recently handed out by track() / result() (rbs_tracker_occlusion_map), reduced on
        the device; needs occlusion_map=True (or set_occlusion_map(True)) -- an RbSensorError otherwise."""
        C = self._C
        frame = C.c_int32()
        plane = np.empty((self.sensor.rows, self.sensor.cols), dtype=np.float32)
        self.sensor._check(self._lib.rbs_tracker_occlusion_map(self._t, C.byref(frame), plane.ctypes.data_as(C.POINTER(C.c_float))))
        return OcclusionMap(plane=plane, frame=int(frame.value))

    def occlusion_map_ms(self):
        """Device time of the last map's kernels in milliseconds (rbs_tracker_occlusion_map_ms)."""
        ms = self._C.c_float()
        self.sensor._check(self._lib.rbs_tracker_occlusion_map_ms(self._t, self._C.byref(ms)))
        return float(ms.value)

    def set_object_map(self, enable):
        """Switch the device's object map on or off (rbs_tracker_set_object_map; refused with frames in flight)."""
        self.sensor._check(self._lib.rbs_tracker_set_object_map(self._t, 1 if enable else 0))

    def object_map(self):
        """The ObjectMap of the frame most recently handed out by track() / result() (rbs_tracker_object_map), reduced on
        the device; needs object_map=True (or set_object_map(True)) -- an RbSensorError otherwise."""
        C = self._C
        r, c = self.sensor.rows, self.sensor.cols
        frame = C.c_int32()
        cover = np.empty((self.parts, r, c), dtype=np.float32)
        depth, var = np.empty((r, c), dtype=np.float32), np.empty((r, c), dtype=np.float32)
        fp = C.POINTER(C.c_float)
        self.sensor._check(self._lib.rbs_tracker_object_map(self._t, C.byref(frame), cover.ctypes.data_as(fp), depth.ctypes.data_as(fp),
                                                            var.ctypes.data_as(fp)))
        return ObjectMap(cover=cover, depth=depth, var=var, frame=int(frame.value))

    def object_map_ms(self):
        """Device time of the last object map's kernels in milliseconds (rbs_tracker_object_map_ms)."""
        ms = self._C.c_float()
        self.sensor._check(self._lib.rbs_tracker_object_map_ms(self._t, self._C.byref(ms)))
        return float(ms.value)

    def poses(self):
        """[n, parts, 12]: the absolute pose of every member of the population get_state() returns (rbs_tracker_poses;
        refused with frames in flight)."""
        out = np.empty((self.n, self.parts, 12))
        self.sensor._check(self._lib.rbs_tracker_poses(self._t, out.ctypes.data_as(self._C.POINTER(self._C.c_double))))
        return out

    def close(self):
        if getattr(self, "_t", None) is not None and self._t.value:
            self._lib.rbs_tracker_destroy(self._t)
            self._t = self._C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def initialize(self, initial_states):
        self.default = self._to_model(initial_states[0])
        self.default.reshape(self.parts, BODY)[:, 6:12] = 0.0
        d = np.ascontiguousarray(self.default, dtype=np.float64)
        self.sensor._check(self._lib.rbs_tracker_initialize(self._t, d.ctypes.data_as(self._C.POINTER(self._C.c_double))))
        self.moving_average = None
        self.n_resamplings = 0
        self._in_flight = 0   # (rbs_tracker_initialize drops frames still in flight)

    def _frame_args(self, image, normals, uniforms):
        C = self._C
        dp, fp = C.POINTER(C.c_double), C.POINTER(C.c_float)
        if not self.device_rng and (normals is None or uniforms is None):
            normals, uniforms = self.draw_randomness()
        # a float64 image (what dbot's tracker receives) goes in as it is: rbs_tracker_track_f64 / _submit_f64 convert while staging
        f64 = isinstance(image, np.ndarray) and image.dtype == np.float64
        img = np.ascontiguousarray(image, dtype=np.float64 if f64 else np.float32).ravel()
        nptr = uptr = None
        if normals is not None:
            normals = np.ascontiguousarray(normals, dtype=np.float64)
            nptr = normals.ctypes.data_as(dp)
        if uniforms is not None:
            uniforms = np.ascontiguousarray(uniforms, dtype=np.float64)
            uptr = uniforms.ctypes.data_as(dp)
        self._f64 = f64
        return (img, normals, uniforms), (img.ctypes.data_as(dp if f64 else fp), nptr, uptr, C.c_uint64(self.seed))

    def _estimate(self, out, nres):
        self.default = out
        self.n_resamplings = int(nres.value)
        est = self._from_model(self.default)
        rate = self.params.moving_average_update_rate
        self.moving_average = est if self.moving_average is None else rate * est + (1 - rate) * self.moving_average
        return self.moving_average.copy()

    def track(self, image, normals=None, uniforms=None):
        C = self._C
        _keep, args = self._frame_args(image, normals, uniforms)
        out = np.empty(self.parts * BODY)
        nres = C.c_int32()
        fn = self._lib.rbs_tracker_track_f64 if self._f64 else self._lib.rbs_tracker_track
        self.sensor._check(fn(self._t, *args, out.ctypes.data_as(C.POINTER(C.c_double)), C.byref(nres)))
        return self._estimate(out, nres)

    def submit(self, image, normals=None, uniforms=None):
        """Enqueue one frame (rbs_tracker_submit) and return at once; at most two frames may be in
        flight.  result() hands out the estimates in submission order."""
        _keep, args = self._frame_args(image, normals, uniforms)
        self.sensor._check((self._lib.rbs_tracker_submit_f64 if self._f64 else self._lib.rbs_tracker_submit)(self._t, *args))
        self._in_flight += 1

    def result(self):
        """The moving-average estimate of the oldest submitted frame (rbs_tracker_result)."""
        C = self._C
        out = np.empty(self.parts * BODY)
        nres = C.c_int32()
        self.sensor._check(self._lib.rbs_tracker_result(self._t, out.ctypes.data_as(C.POINTER(C.c_double)), C.byref(nres)))
        self._in_flight = max(0, self._in_flight - 1)
        return self._estimate(out, nres)

    def get_state(self):
        """(particle deltas [n, parts*12], log-weights [n], occlusion slot map [n]) from the device."""
        C = self._C
        p = np.empty((self.n, self.parts * BODY))
        w = np.empty(self.n)
        i = np.empty(self.n, dtype=np.int32)
        self.sensor._check(self._lib.rbs_tracker_get(self._t, p.ctypes.data_as(C.POINTER(C.c_double)),
                                                     w.ctypes.data_as(C.POINTER(C.c_double)),
                                                     i.ctypes.data_as(C.POINTER(C.c_int32))))
        return p, w, i
