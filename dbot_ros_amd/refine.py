"""Pose refiner: poses moved onto the surface a depth frame shows, on the sensor's device (rbs_refine_* in
librbsensor_mi355x.so; the rule: include/rbsensor_mi355x.h and DESIGN.md Appendix Q).

Projective point-to-plane ICP solved as damped Gauss-Newton on the assess rule's per-body planes: deterministic, a handful
of iterations, all of them enqueued without a host round trip.  Poses cross the C-ABI in the sensor's (centred) mesh
frame, [n, parts, 12] R row-major | t, as for PoseAssessor.assess.  Every default below is an unmeasured starting value.
"""
import ctypes as C
from dataclasses import dataclass, fields

import numpy as np

from . import _capi

MAX_ITERATIONS, CONVERGED, TOO_FEW_PIXELS, DEGENERATE, FROZEN = range(5)
STATUSES = ("MAX_ITERATIONS", "CONVERGED", "TOO_FEW_PIXELS", "DEGENERATE", "FROZEN")
_INT = ("min_pixels", "iters")


@dataclass
class Refinement:
    status: np.ndarray        # [n, parts] int32: MAX_ITERATIONS, CONVERGED, TOO_FEW_PIXELS, DEGENERATE
    iterations: np.ndarray    # [n, parts] int32: iterations evaluated
    counts: np.ndarray        # [n, parts, 2] int32: usable pixels of the first / last evaluated iteration
    rms: np.ndarray           # [n, parts, 2] float64: sqrt(q / count) of those, in sigmas


@dataclass
class Iteration:
    pose: np.ndarray          # [12] the pose that entered the iteration
    sums: np.ndarray          # [28] H upper (21), g (6), q
    delta: np.ndarray         # [6] (omega, v) applied
    count: int
    status: int


class PoseRefiner:
    """PoseRefiner(sensor, params=None).refine(poses, frame=None) -> (poses, Refinement)."""

    @dataclass
    class Parameters:   # unmeasured starting values, every one of them
        gate_sigmas: float = 10.0
        huber_sigmas: float = 3.0
        damping: float = 1e-3
        max_rotation: float = 0.2
        max_translation: float = 0.02
        eps_rotation: float = 1e-3
        eps_translation: float = 1e-4
        min_pixels: int = 16
        iters: int = 10

        @classmethod
        def from_mapping(cls, m):
            p = cls()
            names = [f.name for f in fields(cls)]
            for k, v in dict(m or {}).items():
                if k not in names:
                    raise ValueError(f"pose_refiner/{k}: unknown key (one of {sorted(names)})")
                setattr(p, k, int(v) if k in _INT else float(v))
            return p

        def c_params(self):
            p = _capi.RbsRefineParams()
            for f in fields(self):
                v = getattr(self, f.name)
                setattr(p, f.name, int(v) if f.name in _INT else float(v))
            return p

    def __init__(self, sensor, params=None):
        self._lib = _capi.load()
        self.sensor = sensor
        self.params = params or PoseRefiner.Parameters()

    def refine(self, poses, frame=None):
        """poses: [n, parts, 12] (or anything of n * parts * 12 values); frame: rows*cols depth (metres, NaN = no
        reading), or None for the sensor's current observation."""
        B = self.sensor.n_bodies
        P = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, B, 12)
        n = P.shape[0]
        img = None
        if frame is not None:
            img = np.ascontiguousarray(frame, dtype=np.float32).ravel()
            if img.size != self.sensor.rows * self.sensor.cols:
                raise ValueError(f"frame has {img.size} pixels, the sensor {self.sensor.rows * self.sensor.cols}")
        out = np.empty_like(P)
        rec = (_capi.RbsRefineBody * max(n * B, 1))()
        cp = self.params.c_params()
        fp = img.ctypes.data_as(C.POINTER(C.c_float)) if img is not None else None
        dp = C.POINTER(C.c_double)
        self.sensor._check(self._lib.rbs_refine_poses(self.sensor._h, C.byref(cp), fp, P.ctypes.data_as(dp), n, out.ctypes.data_as(dp), rec))
        r = rec[:n * B]
        return out, Refinement(np.array([x.status for x in r], dtype=np.int32).reshape(n, B),
                               np.array([x.iterations for x in r], dtype=np.int32).reshape(n, B),
                               np.array([(x.count_first, x.count_last) for x in r], dtype=np.int32).reshape(n, B, 2),
                               np.array([(x.rms_first, x.rms_last) for x in r], dtype=np.float64).reshape(n, B, 2))

    def refine_state(self, tracker, state, frame=None):
        """One tracker State refined -> (State, Refinement of a single pose).  The velocities are the given state's."""
        from .assess import state_poses
        from .pose import Rt_to_state
        poses, rec = self.refine(state_poses(tracker, state), frame)
        out = Rt_to_state(tracker, poses[0]).reshape(tracker.parts, 12)
        out[:, 6:12] = np.asarray(state, dtype=np.float64).reshape(tracker.parts, 12)[:, 6:12]
        return out.ravel(), rec

    def history(self, k, b, it):
        """Iteration `it` of body b of the last call's pose k (rbs_refine_get_history)."""
        h = _capi.RbsRefineHistory()
        self.sensor._check(self._lib.rbs_refine_get_history(self.sensor._h, int(k), int(b), int(it), C.byref(h)))
        return Iteration(np.array(h.pose), np.array(h.sums), np.array(h.delta), int(h.count), int(h.status))

    def kernel_ms(self):
        """Device ms of the last call, summed over its iterations: (render, accumulate, solve)."""
        out = (C.c_float * 3)()
        self.sensor._check(self._lib.rbs_refine_kernel_ms(self.sensor._h, out))
        return tuple(float(v) for v in out)


def refine_last_estimate(tracker, refiner, frame=None, in_flight=False):
    """The trackers' refine(): the last estimate refined against `frame` (None: the sensor's current observation) and
    returned as a State; the filter is not touched.  With frames in flight the frame must be given."""
    if tracker.moving_average is None:
        raise ValueError("refine: no frame tracked yet")
    if in_flight and frame is None:
        raise ValueError("refine: frames are in flight (submit / result): pass the estimate's frame")
    return refiner.refine_state(tracker, tracker.moving_average, frame)
