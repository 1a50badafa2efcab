"""Object finder: the object's initial pose from one depth frame, searched on the sensor's device
(rbs_find_* in librbsensor_mi355x.so; the search: include/rbsensor_mi355x.h and DESIGN.md Appendix F).

The reference starts a tracker from the pose an external FindObject service returns when a request
has auto_detect set (R:source/dbot_ros/tracker/object_tracker_controller_service_node.cpp:143-167);
ObjectFinder.find is that search.  Poses cross the C-ABI in the sensor's (centred) mesh frame; this
class undoes center_object_frame, so its states go straight into tracker.initialize([states[0]]).
"""
import ctypes as C
import math
from collections import namedtuple
from dataclasses import dataclass, fields
from typing import Optional

import numpy as np

from . import _capi
from .pose import matrix_to_rotvec
from .sensor import RbSensorError


@dataclass
class FindResult:
    found: bool
    states: np.ndarray    # [K, 12] tracker states (position, rotation vector, zero velocities), caller's mesh frame
    poses: np.ndarray     # [K, 12] R row-major | t of the sensor's (centred) mesh frame
    scores: np.ndarray    # [K] log-likelihoods at the sensor's resolution
    assessment: Optional[object] = None   # find(assess=PoseAssessor): the assess.Assessment of the K poses against the frame
    confirmed: Optional[int] = None       # ... and the first pose whose verdict is SUPPORTED (-1: none)
    classes: Optional[np.ndarray] = None  # the gate on: [K] int32, 0 = the pose is confirmed (SUPPORTED and PRESENT); None: the stage off
    refined: Optional[np.ndarray] = None  # find(refine=PoseRefiner): [K', 12] the first K' = min(K, 64) poses refined against the frame
    refined_states: Optional[np.ndarray] = None   # ... as tracker states [K', 12], like `states`
    refinement: Optional[object] = None   # ... and the refine.Refinement of those poses


# the dominant plane of the last find (step 1b): 1 / z = a u + b v + c over the coarse pixels (u, v)
Plane = namedtuple("Plane", "accepted a b c count n_valid trial masked")


class ObjectFinder:
    """ObjectFinder(sensor, object_model, params, foreground=None, refinement=None, gate=None).find(frame=None) -> FindResult."""

    @dataclass
    class Foreground:
        """Step 1b (rbs_find_foreground): seeds only from what stands in front of the frame's dominant depth plane."""
        enabled: bool = True
        plane_trials: int = 256
        ransac_sigmas: float = 2.0
        mask_sigmas: float = 5.0
        min_inlier_fraction: float = 0.2

        @classmethod
        def from_mapping(cls, m):
            g = cls()
            names = [f.name for f in fields(cls)]
            for k, v in dict(m or {}).items():
                if k not in names:
                    raise ValueError(f"object_finder/foreground/{k}: unknown key (one of {sorted(names)})")
                cur = getattr(g, k)
                setattr(g, k, bool(v) if isinstance(cur, bool) else int(v) if isinstance(cur, int) else float(v))
            return g

        def c_params(self):
            g = _capi.RbsFindForeground()
            for f in fields(self):
                setattr(g, f.name, int(getattr(self, f.name)) if f.name in ("enabled", "plane_trials") else getattr(self, f.name))
            return g

    @dataclass
    class Refinement:
        """Step 6b (rbs_find_refinement): every survivor's 6 x 6 search covariance adapts to its round's best children."""
        enabled: bool = True
        elite: int = 8
        mix: float = 0.5
        shrink: float = 1.0
        jitter: float = 1e-10

        @classmethod
        def from_mapping(cls, m):
            g = cls()
            names = [f.name for f in fields(cls)]
            for k, v in dict(m or {}).items():
                if k not in names:
                    raise ValueError(f"object_finder/refinement/{k}: unknown key (one of {sorted(names)})")
                cur = getattr(g, k)
                setattr(g, k, bool(v) if isinstance(cur, bool) else int(v) if isinstance(cur, int) else float(v))
            return g

        def c_params(self):
            g = _capi.RbsFindRefinement()
            for f in fields(self):
                setattr(g, f.name, int(getattr(self, f.name)) if f.name in ("enabled", "elite") else getattr(self, f.name))
            return g

    @dataclass
    class Gate:
        """The silhouette gate (rbs_find_gate; steps 4b, 5 and 7): every hypothesis' assess and contour evidence, the
        confirmed ones first.  The fields besides the two switches are rbs_assess_params' and rbs_contour_params'."""
        enabled: bool = True
        require_confirmed: bool = False
        radius: int = 2
        min_rim_pixels: int = 16
        min_pixels: int = 16
        sigmas: float = 3.0
        min_support_fraction: float = 0.5
        min_visible_fraction: float = 0.25
        min_valid_fraction: float = 0.5
        min_contour_fraction: float = 0.3
        min_flush_fraction: float = 0.5

        @classmethod
        def from_mapping(cls, m):
            g = cls()
            names = [f.name for f in fields(cls)]
            for k, v in dict(m or {}).items():
                if k not in names:
                    raise ValueError(f"object_finder/gate/{k}: unknown key (one of {sorted(names)})")
                cur = getattr(g, k)
                setattr(g, k, bool(v) if isinstance(cur, bool) else int(v) if isinstance(cur, int) else float(v))
            return g

        def c_params(self):
            g = _capi.RbsFindGate()
            whole = ("enabled", "require_confirmed", "radius", "min_rim_pixels", "min_pixels")
            for f in fields(self):
                setattr(g, f.name, int(getattr(self, f.name)) if f.name in whole else getattr(self, f.name))
            return g

    @dataclass
    class Parameters:
        coarse_downsampling: int = 0          # 0: the largest of {1, 2, 4} leaving >= 160 columns
        seed_stride: int = 4
        min_depth: float = 0.2
        max_depth: float = 3.0
        depth_offset: float = -1.0            # < 0: mean vertex distance from the mesh's centre
        max_seeds: int = 1024
        n_rotations: int = 1024
        n_candidates: int = 512
        nms_translation: float = 0.02
        nms_angle: float = math.radians(30.0)
        n_survivors: int = 32
        rounds: int = 8
        children: int = 64
        sigma_translation: float = 0.01
        sigma_angle: float = math.radians(10.0)
        decay: float = 0.6
        batch: int = 65536
        seed: int = 0
        min_score: float = -math.inf
        foreground: Optional["ObjectFinder.Foreground"] = None   # step 1b; None: off
        # step 6b, an ObjectFinder.Refinement; None: off (step 6's fixed schedule).  A plain attribute, not a dataclass field:
        # the fields besides `foreground` are rbs_find_params' own, one to one.
        refinement = None
        # the gate, an ObjectFinder.Gate; None: off.  A plain attribute as well
        gate = None
        # the optional `scene:` mapping, a SceneFinder.Parameters (several objects: node.build_scene_finder); None: its defaults
        scene = None
        # the optional `refine:` key (node.py: the poses a replay starts from are refined by node.build_pose_refiner's PoseRefiner);
        # a plain attribute as well: the finder itself never reads it -- find(refine=...) is the switch
        refine = False

        @classmethod
        def from_rosparam(cls, tree):
            """From the optional `object_finder:` mapping of the merged rosparam tree; every key is
            optional (angles in degrees: nms_angle_deg, sigma_angle_deg; foreground / refinement / gate: mappings of
            Foreground's / Refinement's / Gate's fields; scene: a mapping of SceneFinder.Parameters' fields)."""
            m = dict((tree or {}).get("object_finder") or {})
            p = cls()
            if "foreground" in m:
                p.foreground = ObjectFinder.Foreground.from_mapping(m.pop("foreground"))
            if "refinement" in m:
                p.refinement = ObjectFinder.Refinement.from_mapping(m.pop("refinement"))
            if "gate" in m:
                p.gate = ObjectFinder.Gate.from_mapping(m.pop("gate"))
            if "scene" in m:
                p.scene = SceneFinder.Parameters.from_mapping(m.pop("scene"))
            if "refine" in m:
                p.refine = bool(m.pop("refine"))
            for k in ("nms_angle", "sigma_angle"):
                if k + "_deg" in m:
                    m[k] = math.radians(float(m.pop(k + "_deg")))
            names = {f.name: f.type for f in fields(cls)}
            for k, v in m.items():
                if k not in names:
                    raise ValueError(f"object_finder/{k}: unknown key (one of {sorted(names)})")
                setattr(p, k, int(v) if isinstance(getattr(p, k), int) else float(v))
            return p

        def c_params(self):
            p = _capi.RbsFindParams()
            for f in fields(self):
                if f.name != "foreground":
                    setattr(p, f.name, getattr(self, f.name))
            return p

    def __init__(self, sensor, object_model, params=None, foreground=None, refinement=None, gate=None):
        self._lib = _capi.load()
        self.sensor = sensor
        self.params = params or ObjectFinder.Parameters()
        self.centers = np.array(object_model.centers)
        self._f = C.c_void_p()
        cp = self.params.c_params()
        rc = self._lib.rbs_find_create(sensor._h, C.byref(cp), C.byref(self._f))
        if rc != 0:
            self._f = C.c_void_p()
            sensor._check(rc)
        sensor._register_dependent(self)   # the finder borrows the sensor handle
        self.foreground = None
        foreground = self.params.foreground if foreground is None else foreground
        self.refinement = None
        refinement = self.params.refinement if refinement is None else refinement
        self.gate = None
        gate = self.params.gate if gate is None else gate
        try:
            if foreground is not None:
                self.set_foreground(foreground)
            if refinement is not None:
                self.set_refinement(refinement)
            if gate is not None:
                self.set_gate(gate)
        except Exception:
            self.close()
            raise

    def close(self):
        if getattr(self, "_f", None) is not None and self._f.value:
            self._lib.rbs_find_destroy(self._f)
            self._f = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc):
        if rc != 0:
            raise RbSensorError(rc, self._lib.rbs_find_last_error(self._f).decode())

    def _states_of(self, poses):
        states = np.zeros((len(poses), 12))
        c = self.centers[0]
        for i in range(len(poses)):
            R = poses[i, :9].reshape(3, 3)
            states[i, 0:3] = poses[i, 9:12] - R @ c
            states[i, 3:6] = matrix_to_rotvec(R)
        return states

    def find(self, frame=None, k=None, assess=None, refine=None):
        """frame: rows*cols depth (metres, NaN = no reading) at the sensor's resolution, or None for
        the sensor's current observation.  Returns up to k (default n_survivors) poses, best first.
        assess: a PoseAssessor over the same sensor -- the returned poses are judged against the same frame
        (FindResult.assessment) and `confirmed` names the first one that is SUPPORTED (with the assessor's contour rule
        on: the first of Assessment.confirmed_mask()); `found` is unchanged.
        refine: a PoseRefiner over the same sensor -- the returned poses are refined against the same frame
        (FindResult.refined, refined_states, refinement) and `assess` judges the refined ones; poses, states and scores
        stay the finder's own."""
        k = int(self.params.n_survivors if k is None else k)
        poses = np.zeros((max(k, 1), 12))
        scores = np.zeros(max(k, 1))
        n, found = C.c_int32(), C.c_int32()
        dp = C.POINTER(C.c_double)
        img = None
        if frame is not None:
            img = np.ascontiguousarray(frame, dtype=np.float32).ravel()
            if img.size != self.sensor.rows * self.sensor.cols:
                raise ValueError(f"frame has {img.size} pixels, the sensor {self.sensor.rows * self.sensor.cols}")
        self._check(self._lib.rbs_find_run(self._f, img.ctypes.data_as(C.POINTER(C.c_float)) if img is not None else None, k,
                                           poses.ctypes.data_as(dp), scores.ctypes.data_as(dp), C.byref(n), C.byref(found)))
        K = int(n.value)
        poses, scores = poses[:K].copy(), scores[:K].copy()
        res = FindResult(bool(found.value), self._states_of(poses), poses, scores)
        if self.gate is not None:
            res.classes = self.evidence(_capi.RBS_FIND_RESULT)[1][:K]
        judged = poses
        if refine is not None and K > 0:
            refined, res.refinement = refine.refine(poses[:min(K, 64)], img)
            res.refined = judged = refined.reshape(-1, 12)
            res.refined_states = self._states_of(res.refined)
        if assess is not None:
            from .assess import SUPPORTED
            res.confirmed = -1
            if K > 0:
                res.assessment = assess.assess(judged[:min(K, 64)], img)
                hits = np.nonzero(res.assessment.verdicts[:, 0] == SUPPORTED)[0]
                if res.assessment.contour_verdicts is not None:   # the assessor's contour rule is on: the silhouette must be PRESENT too
                    hits = np.nonzero(res.assessment.confirmed_mask())[0]
                res.confirmed = int(hits[0]) if hits.size else -1
        return res

    def stage(self, stage, round=0):
        """One stage's exact outputs of the last find: (poses, scores, indices, info); see rbs_find_get_stage."""
        if isinstance(stage, str):
            stage = {"seeds": 0, "coarse": 1, "candidates": 2, "survivors": 3, "children": 4, "result": 5}[stage]
        n = C.c_int64()
        info = np.zeros(6)
        dp, lp = C.POINTER(C.c_double), C.POINTER(C.c_int64)
        self._check(self._lib.rbs_find_get_stage(self._f, stage, round, None, None, None, C.byref(n), info.ctypes.data_as(dp)))
        m = int(n.value)
        width = 4 if stage == _capi.RBS_FIND_SEEDS else 12
        poses = np.zeros((m, width))
        scores = np.zeros(m)
        idx = np.zeros(m, dtype=np.int64)
        self._check(self._lib.rbs_find_get_stage(self._f, stage, round, poses.ctypes.data_as(dp), scores.ctypes.data_as(dp),
                                                 idx.ctypes.data_as(lp), C.byref(n), None))
        return poses, scores, idx, info

    def set_foreground(self, foreground=None):
        """Step 1b for the finds from the next one on; None (or enabled = False): off.  Bad values raise, and the
        previous setting stays."""
        if foreground is None or not foreground.enabled:
            self._check(self._lib.rbs_find_set_foreground(self._f, None))
            self.foreground = None
            return
        g = foreground.c_params()
        self._check(self._lib.rbs_find_set_foreground(self._f, C.byref(g)))
        self.foreground = foreground

    def set_refinement(self, refinement=None):
        """Step 6b for the finds from the next one on; None (or enabled = False): off, step 6's fixed schedule.  Bad values
        raise, and the previous setting stays."""
        if refinement is None or not refinement.enabled:
            self._check(self._lib.rbs_find_set_refinement(self._f, None))
            self.refinement = None
            return
        g = refinement.c_params()
        self._check(self._lib.rbs_find_set_refinement(self._f, C.byref(g)))
        self.refinement = refinement

    def set_gate(self, gate=None):
        """The gate for the finds from the next one on; None (or enabled = False): off.  Bad values raise, and the previous
        setting stays."""
        if gate is None or not gate.enabled:
            self._check(self._lib.rbs_find_set_gate(self._f, None))
            self.gate = None
            return
        g = gate.c_params()
        self._check(self._lib.rbs_find_set_gate(self._f, C.byref(g)))
        self.gate = gate

    def evidence(self, stage):
        """The last find's evidence of `stage` ("coarse", "candidates", "survivors" or "result"), in that stage's order:
        (records [n, 10] int32 = rendered, valid, support, in_front, behind, rim, valid, flush, in_front, beyond;
        classes [n] int32).  The gate only."""
        if isinstance(stage, str):
            stage = {"coarse": 1, "candidates": 2, "survivors": 3, "result": 5}[stage]
        n = C.c_int64()
        ip = C.POINTER(C.c_int32)
        self._check(self._lib.rbs_find_get_evidence(self._f, stage, None, None, C.byref(n)))
        rec = np.zeros((int(n.value), 10), dtype=np.int32)
        cls = np.zeros(int(n.value), dtype=np.int32)
        self._check(self._lib.rbs_find_get_evidence(self._f, stage, rec.ctypes.data_as(ip), cls.ctypes.data_as(ip), C.byref(n)))
        return rec, cls

    def gate_ms(self):
        """Device ms of the last find's evidence kernel: step 4b, step 7."""
        out = (C.c_float * 2)()
        self._check(self._lib.rbs_find_gate_ms(self._f, out))
        return list(out)

    def covariance(self, round):
        """The last find's covariances entering `round` [survivors, 6, 6] (round = rounds: the final ones); step 6b only."""
        n = C.c_int64()
        self._check(self._lib.rbs_find_get_covariance(self._f, round, None, C.byref(n)))
        out = np.zeros((int(n.value), 6, 6))
        self._check(self._lib.rbs_find_get_covariance(self._f, round, out.ctypes.data_as(C.POINTER(C.c_double)), C.byref(n)))
        return out

    def perturbations(self, round):
        """The perturbations d of round `round`'s children [survivors * children, 6]; step 6b only."""
        n = C.c_int64()
        self._check(self._lib.rbs_find_get_perturbations(self._f, round, None, C.byref(n)))
        out = np.zeros((int(n.value), 6))
        self._check(self._lib.rbs_find_get_perturbations(self._f, round, out.ctypes.data_as(C.POINTER(C.c_double)), C.byref(n)))
        return out

    def plane(self):
        """The last find's dominant plane (rbs_find_get_plane); the stage off: all zeros."""
        out = np.zeros(8)
        self._check(self._lib.rbs_find_get_plane(self._f, out.ctypes.data_as(C.POINTER(C.c_double))))
        return Plane(bool(out[0]), float(out[1]), float(out[2]), float(out[3]), int(out[4]), int(out[5]), int(out[6]), int(out[7]))

    def seed_frame(self):
        """The last find's seeding frame [coarse rows, coarse cols] float32 (the stage off: the coarse frame)."""
        n = C.c_int64()
        self._check(self._lib.rbs_find_get_seed_frame(self._f, None, C.byref(n)))
        out = np.zeros(int(n.value), dtype=np.float32)
        self._check(self._lib.rbs_find_get_seed_frame(self._f, out.ctypes.data_as(C.POINTER(C.c_float)), C.byref(n)))
        _, _, _, info = self.stage(_capi.RBS_FIND_SEEDS)
        return out.reshape(int(info[0]), int(info[1]))

    def stage_ms(self):
        """Device ms of the last find: frame + seeds, coarse scoring, selection, refinement, whole find."""
        out = (C.c_float * 5)()
        self._check(self._lib.rbs_find_stage_ms(self._f, out))
        return list(out)


@dataclass
class SceneFindResult:
    found: np.ndarray     # [B] bool: a searched body has a pose that passed min_score (given bodies: True)
    searched: np.ndarray  # [B] bool
    state: np.ndarray     # [B*12] one tracker state of all bodies (caller's mesh frames), for tracker.initialize([state])
    states: np.ndarray    # [B, 12] the same, per body
    poses: np.ndarray     # [B, 12] R row-major | t of the sensor's (centred) mesh frames; NaN: a searched body without a pose
    scores: np.ndarray    # [B] each searched body's score on its residual frame (NaN: given, or no pose)
    joint_score: float    # the B-body log-likelihood of `poses` on the frame (NaN: a body has no pose)
    assessment: Optional[object] = None   # find(assess=PoseAssessor): the assess.Assessment of the B poses against the frame
    confirmed: Optional[np.ndarray] = None   # ... and [B] bool: the body is searched and confirmed (None: no assessor, or a body without a pose)
    refined: Optional[np.ndarray] = None     # find(refine=PoseRefiner): [B, 12] the poses refined against the frame (None: no refiner, or a body without a pose)
    refined_state: Optional[np.ndarray] = None   # ... as one tracker state [B*12], like `state`
    refinement: Optional[object] = None      # ... and the refine.Refinement of that one pose

    @property
    def all_found(self):
        return bool(self.found.all())


class _BodyFinder(ObjectFinder):
    """A scene finder's finder of one body (rbs_find_scene_body_finder), borrowed: the inspection methods of
    ObjectFinder (stage, plane, seed_frame, covariance, perturbations, evidence, stage_ms, gate_ms) read that body's last find."""

    def __init__(self, scene, body):
        self._lib = scene._lib
        self.sensor = scene.sensor
        self.params = scene.params
        self.centers = scene.centers[body:body + 1]
        self._scene = scene          # (keeps the owner alive)
        self._f = C.c_void_p(self._lib.rbs_find_scene_body_finder(scene._f, body))
        if not self._f.value:
            raise ValueError(f"body {body} outside 0..{scene.parts - 1}")
        self.foreground, self.refinement, self.gate = scene.foreground, scene.refinement, scene.gate

    def close(self):
        self._f = C.c_void_p()

    def find(self, *a, **k):
        raise TypeError("a scene finder's body finder is borrowed: run SceneFinder.find")

    set_foreground = set_refinement = set_gate = find


class SceneFinder:
    """SceneFinder(sensor, object_model, params=None, scene=None, foreground=None, refinement=None, gate=None).find(frame, search, given)
    -> SceneFindResult: every body of a model of several from one depth frame (rbs_find_scene_*; the rule:
    include/rbsensor_mi355x.h and DESIGN.md Appendix K).  params: ObjectFinder.Parameters, every body's find."""

    @dataclass
    class Parameters:
        """rbs_find_scene_params.  explain_radius and the polish figures are unmeasured starting values."""
        explain_sigmas: float = 3.0
        explain_radius: int = 2
        polish_sweeps: int = 2
        polish_children: int = 64
        polish_sigma_translation: float = 0.005
        polish_sigma_angle: float = math.radians(5.0)
        polish_decay: float = 0.6

        @classmethod
        def from_mapping(cls, m):
            """From the optional `object_finder/scene:` mapping (the angle in degrees: polish_sigma_angle_deg)."""
            m = dict(m or {})
            g = cls()
            if "polish_sigma_angle_deg" in m:
                m["polish_sigma_angle"] = math.radians(float(m.pop("polish_sigma_angle_deg")))
            names = [f.name for f in fields(cls)]
            for k, v in m.items():
                if k not in names:
                    raise ValueError(f"object_finder/scene/{k}: unknown key (one of {sorted(names + ['polish_sigma_angle_deg'])})")
                setattr(g, k, int(v) if isinstance(getattr(g, k), int) else float(v))
            return g

        def c_params(self):
            p = _capi.RbsFindSceneParams()
            for f in fields(self):
                setattr(p, f.name, getattr(self, f.name))
            p.reserved = 0
            return p

    def __init__(self, sensor, object_model, params=None, scene=None, foreground=None, refinement=None, gate=None):
        self._lib = _capi.load()
        self.sensor = sensor
        self.params = params or ObjectFinder.Parameters()
        self.scene = scene or SceneFinder.Parameters()
        self.centers = np.array(object_model.centers, dtype=np.float64).reshape(-1, 3)
        self.parts = len(self.centers)
        self._f = C.c_void_p()
        cp, sp = self.params.c_params(), self.scene.c_params()
        rc = self._lib.rbs_find_scene_create(sensor._h, C.byref(cp), C.byref(sp), C.byref(self._f))
        if rc != 0:
            self._f = C.c_void_p()
            sensor._check(rc)
        sensor._register_dependent(self)   # the scene finder borrows the sensor handle
        self.foreground = self.refinement = self.gate = None
        foreground = self.params.foreground if foreground is None else foreground
        refinement = self.params.refinement if refinement is None else refinement
        gate = self.params.gate if gate is None else gate
        try:
            if foreground is not None:
                self.set_foreground(foreground)
            if refinement is not None:
                self.set_refinement(refinement)
            if gate is not None:
                self.set_gate(gate)
        except Exception:
            self.close()
            raise

    def close(self):
        if getattr(self, "_f", None) is not None and self._f.value:
            self._lib.rbs_find_scene_destroy(self._f)
            self._f = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc):
        if rc != 0:
            raise RbSensorError(rc, self._lib.rbs_find_scene_last_error(self._f).decode())

    def set_foreground(self, foreground=None):
        """Step 1b of every body's find, as ObjectFinder.set_foreground."""
        on = foreground is not None and foreground.enabled
        g = foreground.c_params() if on else None
        self._check(self._lib.rbs_find_scene_set_foreground(self._f, C.byref(g) if on else None))
        self.foreground = foreground if on else None

    def set_refinement(self, refinement=None):
        """Step 6b of every body's find, as ObjectFinder.set_refinement."""
        on = refinement is not None and refinement.enabled
        g = refinement.c_params() if on else None
        self._check(self._lib.rbs_find_scene_set_refinement(self._f, C.byref(g) if on else None))
        self.refinement = refinement if on else None

    def set_gate(self, gate=None):
        """The gate of every body's find, as ObjectFinder.set_gate.  With require_confirmed a body without a confirmed
        pose is not placed: `found` is False for it."""
        on = gate is not None and gate.enabled
        g = gate.c_params() if on else None
        self._check(self._lib.rbs_find_scene_set_gate(self._f, C.byref(g) if on else None))
        self.gate = gate if on else None

    def mask_of(self, search):
        """None: every body; an int: the mask itself; else the bodies' indices."""
        if search is None:
            return (1 << self.parts) - 1
        if isinstance(search, (int, np.integer)):
            return int(search)
        m = 0
        for b in search:
            if not 0 <= int(b) < 32:
                raise ValueError(f"search: body {b} outside 0..31")
            m |= 1 << int(b)
        return m

    def poses_of_state(self, state):
        """A tracker state [B*12] (caller's mesh frames) -> poses [B, 12] of the sensor's mesh frames."""
        from .pose import pack_Rt, rotvec_to_matrix
        s = np.asarray(state, dtype=np.float64).reshape(self.parts, 12)
        R = rotvec_to_matrix(s[:, 3:6]).reshape(self.parts, 3, 3)
        t = s[:, 0:3] + np.einsum("bij,bj->bi", R, self.centers)
        return pack_Rt(R, t).reshape(self.parts, 12)

    def find(self, frame=None, search=None, given=None, assess=None, given_poses=None, refine=None):
        """frame: rows*cols depth at the sensor's resolution (None: the sensor's current observation).  search: the bodies
        to place (None: all; indices or a bit mask).  The others' poses: given, a tracker state [B*12] in the caller's mesh
        frames (a tracker's estimate), or given_poses [B, 12] in the sensor's mesh frames, which come back bit for bit.
        assess: a PoseAssessor over the same sensor -- the B poses are judged against the same frame and `confirmed` names
        the searched bodies that read SUPPORTED (with the contour rule on: and PRESENT).
        refine: a PoseRefiner over the same sensor -- the B poses are refined together against the same frame
        (SceneFindResult.refined, refined_state, refinement; the bodies not searched are refined with the others inside the
        call, which `refinement` reports, but keep their given poses bit for bit in `refined`) and
        `assess` judges the refined ones; poses, states and scores stay the finder's own."""
        mask = self.mask_of(search)
        B = self.parts
        gp = None
        if given_poses is not None:
            gp = np.ascontiguousarray(given_poses, dtype=np.float64).reshape(B, 12)
        elif given is not None:
            gp = np.ascontiguousarray(self.poses_of_state(given))
        img = None
        if frame is not None:
            img = np.ascontiguousarray(frame, dtype=np.float32).ravel()
            if img.size != self.sensor.rows * self.sensor.cols:
                raise ValueError(f"frame has {img.size} pixels, the sensor {self.sensor.rows * self.sensor.cols}")
        poses = np.zeros((B, 12))
        scores = np.zeros(B)
        found, joint = C.c_uint32(), C.c_double()
        dp = C.POINTER(C.c_double)
        self._check(self._lib.rbs_find_scene_run(self._f, img.ctypes.data_as(C.POINTER(C.c_float)) if img is not None else None,
                                                 C.c_uint32(mask & 0xFFFFFFFF), gp.ctypes.data_as(dp) if gp is not None else None,
                                                 poses.ctypes.data_as(dp), scores.ctypes.data_as(dp), C.byref(found), C.byref(joint)))
        searched = np.array([bool(mask >> b & 1) for b in range(B)])
        fnd = np.array([bool(found.value >> b & 1) for b in range(B)]) | ~searched
        def states_of(poses):
            states = np.full((B, 12), np.nan)
            for b in range(B):
                if np.isfinite(poses[b]).all():
                    R = poses[b, :9].reshape(3, 3)
                    states[b] = 0.0
                    states[b, 0:3] = poses[b, 9:12] - R @ self.centers[b]
                    states[b, 3:6] = matrix_to_rotvec(R)
            return states

        states = states_of(poses)
        res = SceneFindResult(fnd, searched, states.ravel().copy(), states, poses, scores, float(joint.value))
        judged = poses
        if refine is not None and np.isfinite(poses).all():
            refined, res.refinement = refine.refine(poses[None], img)
            res.refined = judged = refined.reshape(B, 12)
            # the refiner moves every body of a pose: inside the call the given bodies are refined too, so the searched bodies'
            # ownership is taken against neighbours that move with them, and `refinement` reports status, counts and rms of
            # every body as it moved there.  Only the searched bodies take their refined pose; the given ones are put back.
            res.refined[~searched] = poses[~searched]
            res.refined_state = states_of(res.refined).ravel().copy()
        if assess is not None and np.isfinite(poses).all():
            from .assess import SUPPORTED
            res.assessment = assess.assess(judged[None], img)
            ok = np.asarray(res.assessment.verdicts).reshape(-1)[:B] == SUPPORTED
            if res.assessment.contour_verdicts is not None:
                from .assess import CONTOUR_PRESENT
                ok &= np.asarray(res.assessment.contour_verdicts).reshape(-1)[:B] == CONTOUR_PRESENT
            res.confirmed = ok & searched
        return res

    def order(self):
        """The last scene find's S1: (the searched bodies in the order taken, e [B])."""
        order = (C.c_int32 * 32)()
        n = C.c_int32()
        e = np.zeros(self.parts)
        self._check(self._lib.rbs_find_scene_get_order(self._f, order, C.byref(n), e.ctypes.data_as(C.POINTER(C.c_double))))
        return [int(order[i]) for i in range(n.value)], e

    def residual(self, body):
        """The residual frame [rows, cols] float32 that searched body `body` was found on."""
        out = np.zeros(self.sensor.rows * self.sensor.cols, dtype=np.float32)
        self._check(self._lib.rbs_find_scene_get_residual(self._f, int(body), out.ctypes.data_as(C.POINTER(C.c_float))))
        return out.reshape(self.sensor.rows, self.sensor.cols)

    def body_finder(self, body):
        """Body `body`'s finder, borrowed, for inspection (ObjectFinder.stage and the like)."""
        return _BodyFinder(self, int(body))

    def polish(self, round):
        """Polish round `round` of the last scene find: (children poses [n, B, 12], joint scores [n], the child taken)."""
        n, best = C.c_int32(), C.c_int32()
        self._check(self._lib.rbs_find_scene_get_polish(self._f, int(round), None, None, C.byref(n), None))
        poses = np.zeros((n.value, self.parts, 12))
        scores = np.zeros(n.value)
        dp = C.POINTER(C.c_double)
        self._check(self._lib.rbs_find_scene_get_polish(self._f, int(round), poses.ctypes.data_as(dp), scores.ctypes.data_as(dp),
                                                        C.byref(n), C.byref(best)))
        return poses, scores, int(best.value)

    def stage_ms(self):
        """ms of the last scene find: (per body [B], render kernel, residual kernel, polish, whole)."""
        per = (C.c_float * max(self.parts, 1))()
        out = (C.c_float * 4)()
        self._check(self._lib.rbs_find_scene_stage_ms(self._f, per, out))
        return list(per)[:self.parts], out[0], out[1], out[2], out[3]
