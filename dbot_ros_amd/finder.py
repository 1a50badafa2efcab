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


# the dominant plane of the last find (step 1b): 1 / z = a u + b v + c over the coarse pixels (u, v)
Plane = namedtuple("Plane", "accepted a b c count n_valid trial masked")


class ObjectFinder:
    """ObjectFinder(sensor, object_model, params, foreground=None, refinement=None).find(frame=None) -> FindResult."""

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

        @classmethod
        def from_rosparam(cls, tree):
            """From the optional `object_finder:` mapping of the merged rosparam tree; every key is
            optional (angles in degrees: nms_angle_deg, sigma_angle_deg; foreground / refinement: mappings of Foreground's /
            Refinement's fields)."""
            m = dict((tree or {}).get("object_finder") or {})
            p = cls()
            if "foreground" in m:
                p.foreground = ObjectFinder.Foreground.from_mapping(m.pop("foreground"))
            if "refinement" in m:
                p.refinement = ObjectFinder.Refinement.from_mapping(m.pop("refinement"))
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

    def __init__(self, sensor, object_model, params=None, foreground=None, refinement=None):
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
        try:
            if foreground is not None:
                self.set_foreground(foreground)
            if refinement is not None:
                self.set_refinement(refinement)
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

    def find(self, frame=None, k=None, assess=None):
        """frame: rows*cols depth (metres, NaN = no reading) at the sensor's resolution, or None for
        the sensor's current observation.  Returns up to k (default n_survivors) poses, best first.
        assess: a PoseAssessor over the same sensor -- the returned poses are judged against the same frame
        (FindResult.assessment) and `confirmed` names the first one that is SUPPORTED (with the assessor's contour rule
        on: the first of Assessment.confirmed_mask()); `found` is unchanged."""
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
        states = np.zeros((K, 12))
        c = self.centers[0]
        for i in range(K):
            R = poses[i, :9].reshape(3, 3)
            states[i, 0:3] = poses[i, 9:12] - R @ c
            states[i, 3:6] = matrix_to_rotvec(R)
        res = FindResult(bool(found.value), states, poses, scores)
        if assess is not None:
            from .assess import SUPPORTED
            res.confirmed = -1
            if K > 0:
                res.assessment = assess.assess(poses[:min(K, 64)], img)
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
