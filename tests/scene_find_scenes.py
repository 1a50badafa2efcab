"""The scenes of the scene finder's tests (tests/test_scene_find_cpu.py, tests/test_gpu_scene_find.py): bodies placed apart,
frames from synth.make_frame over the CPU oracle's render, and the whole scene find in the numpy twin with the oracle's
scores -- the expectation of the GPU tests' outcome assertions, computed without a device."""
import types

import numpy as np

import oracle_binding as ob
import scenarios as sc
import scene_find_twin as st
from dbot_ros_amd import CameraData, ObjectModel, synth
from dbot_ros_amd.pose import quat_to_matrix

SMALL = dict(max_seeds=48, n_rotations=128, n_candidates=256, n_survivors=8, rounds=3, children=16, batch=4096)
TINY = dict(max_seeds=16, n_rotations=32, n_candidates=64, n_survivors=4, rounds=2, children=8, batch=1024)


def truth_poses(names, cols, rows, K, seed, z=None, spread=0.56):
    """[B][12]: body b's centre on the image's middle row at column (0.5 + (b - (B-1)/2) spread / max(B-1, 1)... ) cols,
    depths 0.6 .. 0.9, a random rotation each."""
    rng = np.random.default_rng(seed)
    B = len(names)
    out = np.zeros((B, 12))
    for b in range(B):
        q = rng.normal(size=4)
        q /= np.linalg.norm(q)
        zb = float(rng.uniform(0.65, 0.85)) if z is None else float(np.atleast_1d(z)[b % np.size(z)])
        frac = 0.5 if B == 1 else 0.5 + spread * (b / (B - 1) - 0.5)
        u, v = frac * cols, (0.5 + 0.06 * ((b % 2) - 0.5)) * rows
        out[b, :9] = np.asarray(quat_to_matrix(q)).ravel()
        out[b, 9:] = [(u - K[0, 2]) / K[0, 0] * zb, (v - K[1, 2]) / K[1, 1] * zb, zb]
    return out


class Scene:
    """names, resolution -> object model, camera, sensor parameters, the truth and a frame of it."""

    def __init__(self, names, cols, rows, seed, z=None, spread=0.56, **frame_kw):
        self.names, self.cols, self.rows, self.B = tuple(names), cols, rows, len(names)
        self.om, self.cam, self.P = sc.make_scene(self.names, cols, rows, max_particles=1)
        self.K = np.asarray(self.cam.camera_matrix, dtype=np.float64)
        self.truth = truth_poses(self.names, cols, rows, self.K, seed, z, spread)
        self.ms, self.sf = self.P.kinect.model_sigma, self.P.kinect.sigma_factor
        self._part = {}
        depth = self.oracle().render_depth(self.truth)
        self.depth = np.where(np.isfinite(depth), depth, np.inf).astype(np.float32)
        self.frame = synth.make_frame(self.depth, rows, cols, np.random.default_rng(seed + 1000), **frame_kw)
        self.e = [st.mean_vertex_distance(v) for v in self.om.vertices]

    def oracle(self, max_particles=1, cam=None):
        return ob.Oracle(self.om, cam or self.cam, self.P, max_particles=max_particles, mode=ob.EAGER)

    def part_model(self, b):
        """The one-body model made of part b (vertices as the sensor holds them: already centred)."""
        return ObjectModel([self.om.vertices[b]], [self.om.triangles[b]], center=False)

    def part_oracle(self, b, max_particles, cam=None):
        return ob.Oracle(self.part_model(b), cam or self.cam, self.P, max_particles=max_particles, mode=ob.EAGER)

    def plane(self, b, pose):
        """Body b rendered alone by the oracle: [npx] float32, +inf where it covers nothing."""
        if b not in self._part:
            self._part[b] = self.part_oracle(b, 1)
        d = self._part[b].render_depth(np.asarray(pose, dtype=np.float64).reshape(12))
        return np.where(np.isfinite(d), d, np.inf).astype(np.float32)

    def planes(self, poses):
        return np.stack([self.plane(b, poses[b]) for b in range(self.B)])


def _scores(oracle, frame, poses, threads):
    poses = np.ascontiguousarray(poses, dtype=np.float64)
    n = len(poses)
    oracle.reset()
    oracle.set_observation(np.asarray(frame, dtype=np.float64))
    return oracle.loglikes_poses(poses, np.zeros(n, dtype=np.int32), update=False, threads=threads)


def twin_scene_find(scene, search_mask=None, given=None, find=SMALL, seed=0, foreground=None, refinement=None, threads=None, **scene_params):
    """The whole scene find of scene.frame in the twin, every score the eager oracle's."""
    threads = threads or sc.usable_threads()
    p = types.SimpleNamespace(coarse_downsampling=0, seed_stride=4, min_depth=0.2, max_depth=3.0, depth_offset=-1.0, nms_translation=0.02,
                              nms_angle=np.radians(30.0), sigma_translation=0.01, sigma_angle=np.radians(10.0), decay=0.6, seed=seed,
                              min_score=-np.inf)
    for k, v in find.items():
        setattr(p, k, v)
    B = scene.B
    search_mask = (1 << B) - 1 if search_mask is None else search_mask
    cap = max(p.max_seeds * p.n_rotations, p.n_survivors * p.children, scene_params.get("polish_children", 64))

    def find_of(b, resid):
        full = scene.part_oracle(b, cap)

        def coarse_score(coarse, cr, cc, Kc, poses):
            o = scene.part_oracle(b, cap, CameraData(Kc, cr, cc))
            return _scores(o, coarse.ravel(), poses, threads)

        poses, scores, found = st.find_body(resid, scene.rows, scene.cols, scene.K, scene.om.vertices[b], p, scene.ms, scene.sf, coarse_score,
                                            lambda q: _scores(full, resid, q, threads), foreground, refinement)
        if len(poses) == 0:
            return None, np.nan, False
        return poses[0], scores[0], found

    joint = scene.oracle(cap)
    return st.scene_find(scene.frame, scene.rows, scene.cols, scene.e, search_mask, given, scene.plane, find_of,
                         lambda q: _scores(joint, scene.frame, q.reshape(len(q), -1), threads), scene.ms, scene.sf, seed, **scene_params)


# ---------------------------------------------------------------- explain-away on identical meshes
FOREGROUND = dict(plane_trials=256, ransac_sigmas=2.0, mask_sigmas=5.0, min_inlier_fraction=0.2)
# the distance of each found body to the copy it lands on, in the twin run on the CPU (tests/test_scene_find_cpu.py)
EXPLAIN_AWAY_TWIN_DISTANCES = (0.00496539, 0.0014898)


def explain_away_scene():
    """Two copies of m1 at 160 x 120, 33 cm apart at 0.50 and 0.55 m, in front of the wall, no occluding slab; the find with
    step 1b on (the wall is the frame's dominant plane).  -> (scene, twin_scene_find's keywords)."""
    return Scene(("m1", "m1"), 160, 120, 1, z=(0.5, 0.55), occluder=False), dict(find=SMALL, seed=0, foreground=FOREGROUND)


def distances_to_copies(poses, truth):
    """[B][B]: |t_b - truth t_c|."""
    return np.linalg.norm(np.asarray(poses)[:, None, 9:] - np.asarray(truth)[None, :, 9:], axis=2)
