"""Pose assessor: poses judged against one depth frame on the sensor's device (rbs_assess_* in
librbsensor_mi355x.so; the rule: include/rbsensor_mi355x.h and DESIGN.md Appendix J).

The reference puts a person between FindObject and RunObjectTracker
(R:source/dbot_ros/tracker/object_tracker_controller_service_node.cpp:180-195); PoseAssessor.assess is that
judgement as integer pixel counts and a verdict per (pose, body).  Poses cross the C-ABI in the sensor's (centred)
mesh frame, [n, parts, 12] R row-major | t, as for RbSensor.render_depth.
"""
import ctypes as C
from dataclasses import dataclass, fields
from typing import Optional

import numpy as np

from . import _capi
from .pose import pack_Rt, rotvec_to_matrix

OUT_OF_VIEW, OCCLUDED, SUPPORTED, LOST = range(4)
VERDICTS = ("OUT_OF_VIEW", "OCCLUDED", "SUPPORTED", "LOST")
COUNTS = ("rendered", "valid", "support", "in_front", "behind")
# the contour rule (rbs_contour_*): the silhouette, opt-in beside the rule above
CONTOUR_NO_RIM, CONTOUR_UNDECIDED, CONTOUR_PRESENT, CONTOUR_ABSENT = range(4)
CONTOUR_VERDICTS = ("NO_RIM", "UNDECIDED", "PRESENT", "ABSENT")
CONTOUR_COUNTS = ("rim", "valid", "flush", "in_front", "beyond")


@dataclass
class Assessment:
    counts: np.ndarray     # [n, parts, 5] int32: rendered, valid, support, in_front, behind
    verdicts: np.ndarray   # [n, parts] int32: OUT_OF_VIEW, OCCLUDED, SUPPORTED, LOST
    contour_counts: Optional[np.ndarray] = None     # [n, parts, 5] int32: rim, valid, flush, in_front, beyond (None: contour off)
    contour_verdicts: Optional[np.ndarray] = None   # [n, parts] int32: NO_RIM, UNDECIDED, PRESENT, ABSENT (None: contour off)

    def confirmed_mask(self):
        """[n] bool: every body SUPPORTED and -- with the contour rule on -- every body's silhouette PRESENT."""
        ok = (np.asarray(self.verdicts) == SUPPORTED).all(axis=1)
        if self.contour_verdicts is not None:
            ok &= (np.asarray(self.contour_verdicts) == CONTOUR_PRESENT).all(axis=1)
        return ok


def state_poses(tracker, state):
    """A tracker State (parts*12, the caller's mesh frame) -> absolute poses [1, parts, 12] of the sensor's mesh frame,
    through the tracker's own state-to-model rule."""
    s = tracker._to_model(state).reshape(tracker.parts, 12)
    return pack_Rt(rotvec_to_matrix(s[:, 3:6]), s[:, 0:3])[None]


class PoseAssessor:
    """PoseAssessor(sensor, params=None, contour=None).assess(poses, frame=None) -> Assessment.  contour: a
    PoseAssessor.ContourParameters switches the contour rule on (rbs_contour_poses: both rules in one call); None: every
    method makes the calls it makes without it."""

    @dataclass
    class Parameters:
        sigmas: float = 3.0
        min_support_fraction: float = 0.5
        min_visible_fraction: float = 0.25
        min_pixels: int = 16

        @classmethod
        def from_mapping(cls, m):
            p = cls()
            names = [f.name for f in fields(cls)]
            for k, v in dict(m or {}).items():
                if k not in names:
                    raise ValueError(f"supervisor/assess/{k}: unknown key (one of {sorted(names)})")
                setattr(p, k, int(v) if k == "min_pixels" else float(v))
            return p

        def c_params(self):
            p = _capi.RbsAssessParams()
            p.sigmas, p.min_support_fraction = float(self.sigmas), float(self.min_support_fraction)
            p.min_visible_fraction, p.min_pixels, p.reserved = float(self.min_visible_fraction), int(self.min_pixels), 0
            return p

    @dataclass
    class ContourParameters:
        radius: int = 2
        min_rim_pixels: int = 16
        min_valid_fraction: float = 0.5
        min_contour_fraction: float = 0.3
        min_flush_fraction: float = 0.5

        @classmethod
        def from_mapping(cls, m):
            p = cls()
            names = [f.name for f in fields(cls)]
            for k, v in dict(m or {}).items():
                if k not in names:
                    raise ValueError(f"supervisor/contour/{k}: unknown key (one of {sorted(names)})")
                setattr(p, k, int(v) if k in ("radius", "min_rim_pixels") else float(v))
            return p

        def c_params(self):
            p = _capi.RbsContourParams()
            p.radius, p.min_rim_pixels = int(self.radius), int(self.min_rim_pixels)
            p.min_valid_fraction, p.min_contour_fraction = float(self.min_valid_fraction), float(self.min_contour_fraction)
            p.min_flush_fraction = float(self.min_flush_fraction)
            return p

    def __init__(self, sensor, params=None, contour=None):
        self._lib = _capi.load()
        self.sensor = sensor
        self.params = params or PoseAssessor.Parameters()
        self.contour = contour

    def assess(self, poses, frame=None):
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
        out = (_capi.RbsAssessBody * max(n * B, 1))()
        cp = self.params.c_params()
        fp = img.ctypes.data_as(C.POINTER(C.c_float)) if img is not None else None
        if self.contour is None:
            self.sensor._check(self._lib.rbs_assess_poses(self.sensor._h, C.byref(cp), fp, P.ctypes.data_as(C.POINTER(C.c_double)), n, out))
            rec = np.frombuffer(out, dtype=np.int32).reshape(-1, 8)[:n * B].reshape(n, B, 8)
            return Assessment(rec[:, :, :5].copy(), rec[:, :, 5].copy())
        cout = (_capi.RbsContourBody * max(n * B, 1))()
        cc = self.contour.c_params()
        self.sensor._check(self._lib.rbs_contour_poses(self.sensor._h, C.byref(cp), C.byref(cc), fp, P.ctypes.data_as(C.POINTER(C.c_double)),
                                                       n, out, cout))
        rec = np.frombuffer(out, dtype=np.int32).reshape(-1, 8)[:n * B].reshape(n, B, 8)
        crec = np.frombuffer(cout, dtype=np.int32).reshape(-1, 8)[:n * B].reshape(n, B, 8)
        return Assessment(rec[:, :, :5].copy(), rec[:, :, 5].copy(), crec[:, :, :5].copy(), crec[:, :, 5].copy())

    def assess_state(self, tracker, state, frame=None):
        """One tracker State judged: Assessment of a single pose."""
        return self.assess(state_poses(tracker, state), frame)

    def verdict(self, counts):
        """The rule's verdict of one record's five counts (rbs_assess_verdict: host only)."""
        body = _capi.RbsAssessBody(*(int(v) for v in counts[:5]))
        v = C.c_int32()
        cp = self.params.c_params()
        rc = self._lib.rbs_assess_verdict(C.byref(cp), C.byref(body), C.byref(v))
        if rc != 0:
            raise ValueError("rbs_assess_verdict: bad parameters")
        return int(v.value)

    def contour_verdict(self, counts):
        """The contour rule's verdict of one record's five counts (rbs_contour_verdict: host only); the library's defaults
        when the contour rule is off."""
        body = _capi.RbsContourBody(*(int(v) for v in counts[:5]))
        v = C.c_int32()
        cc = (self.contour or PoseAssessor.ContourParameters()).c_params()
        rc = self._lib.rbs_contour_verdict(C.byref(cc), C.byref(body), C.byref(v))
        if rc != 0:
            raise ValueError("rbs_contour_verdict: bad parameters")
        return int(v.value)

    def plane(self, k, b):
        """Depth image [rows*cols] float32 of body b of the last call's pose k, rendered alone (+inf where it covers nothing)."""
        out = np.empty(self.sensor.rows * self.sensor.cols, dtype=np.float32)
        self.sensor._check(self._lib.rbs_assess_get_plane(self.sensor._h, int(k), int(b), out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def kernel_ms(self):
        """Device ms of the last call: (render, count), and with the contour rule on (render, count, contour)."""
        if self.contour is not None:
            out = (C.c_float * 3)()
            self.sensor._check(self._lib.rbs_contour_kernel_ms(self.sensor._h, out))
            return tuple(float(v) for v in out)
        out = (C.c_float * 2)()
        self.sensor._check(self._lib.rbs_assess_kernel_ms(self.sensor._h, out))
        return tuple(float(v) for v in out)


def assess_last_estimate(tracker, assessor, frame=None, in_flight=False):
    """The trackers' assess(): the last estimate judged against `frame` (None: the sensor's current observation).  With
    frames in flight the observation is not the estimate's frame: the frame must be given."""
    if tracker.moving_average is None:
        raise ValueError("assess: no frame tracked yet")
    if in_flight and frame is None:
        raise ValueError("assess: frames are in flight (submit / result): pass the estimate's frame")
    return assessor.assess_state(tracker, tracker.moving_average, frame)
