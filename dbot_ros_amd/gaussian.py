"""Host-side mirror of the reference's second tracker, the robust Gaussian tracker
(R:source/dbot_ros/tracker/gaussian_tracker_node.cpp, R:config/gaussian_tracker.yaml):

    GaussianTrackerBuilder<Tracker>::Parameters   R:...gaussian_tracker_node.cpp:78-116
    tracker->initialize(initial_poses) / track     R:source/dbot_ros/object_tracker_ros.hpp:49

The filter is this project's restatement (upstream's fl / dbot are not
vendored, so parity with upstream is unpinned): an unscented-transform Gaussian filter whose
sigma poses are rendered and reduced on the sensor's device (rbs_gauss_* in
librbsensor_mi355x.so).  track() does the D x D algebra on the host inside the library, one host
synchronisation per frame; submit() / result() run the whole step on the device with up to two
frames in flight.  Like DeviceParticleTracker, states cross the C-ABI in model
coordinates; this class does the center_object_frame conversion and the moving average.
"""
import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import _capi
from .sensor import RbSensorError
from .tracker import BODY, ObjectTransitionBuilder, ParticleTracker


class GaussianTrackerBuilder:
    """dbot::GaussianTrackerBuilder<Tracker> mirror."""

    @dataclass
    class Observation:
        tail_weight: float = 0.1
        bg_depth: float = -3.0
        fg_noise_std: float = 0.001
        bg_noise_std: float = 100.0
        uniform_tail_min: float = -5000.0
        uniform_tail_max: float = 5000.0
        sensors: int = 0                   # pixels (camera_data->pixels(), node :133)

    @dataclass
    class Parameters:
        ut_alpha: float = 1.0
        moving_average_update_rate: float = 1.0
        center_object_frame: bool = True
        observation: "GaussianTrackerBuilder.Observation" = field(default_factory=lambda: GaussianTrackerBuilder.Observation())
        object_transition: ObjectTransitionBuilder.Parameters = field(
            default_factory=lambda: ObjectTransitionBuilder.Parameters(0.002, 0.002, 0.002, 0.01, 0.01, 0.01, 0.8))

        @classmethod
        def from_rosparam(cls, tree, part_count, sensors=0):
            """From the dict loaded from R:config/gaussian_tracker.yaml: the keys the node reads at
            R:source/dbot_ros/tracker/gaussian_tracker_node.cpp:78-116, verbatim."""
            g = tree["gaussian_filter"]
            o, t = g["observation"], g["object_transition"]
            obs = GaussianTrackerBuilder.Observation(
                float(o["tail_weight"]), float(o["bg_depth"]), float(o["fg_noise_std"]), float(o["bg_noise_std"]),
                float(o["uniform_tail_min"]), float(o["uniform_tail_max"]), int(sensors))
            tr = ObjectTransitionBuilder.Parameters(*(float(t[k]) for k in (
                "linear_sigma_x", "linear_sigma_y", "linear_sigma_z",
                "angular_sigma_x", "angular_sigma_y", "angular_sigma_z", "velocity_factor")), part_count=int(part_count))
            return cls(float(g["unscented_transform"]["alpha"]), float(g["moving_average_update_rate"]),
                       bool(g["center_object_frame"]), obs, tr)

        def c_params(self):
            """The rbs_gauss_params the library takes."""
            t, o = self.object_transition, self.observation
            p = _capi.RbsGaussParams()
            p.linear_sigma = (C.c_double * 3)(t.linear_sigma_x, t.linear_sigma_y, t.linear_sigma_z)
            p.angular_sigma = (C.c_double * 3)(t.angular_sigma_x, t.angular_sigma_y, t.angular_sigma_z)
            p.velocity_factor = t.velocity_factor
            p.ut_alpha = self.ut_alpha
            p.fg_noise_std, p.bg_depth, p.bg_noise_std = o.fg_noise_std, o.bg_depth, o.bg_noise_std
            p.tail_weight, p.uniform_tail_min, p.uniform_tail_max = o.tail_weight, o.uniform_tail_min, o.uniform_tail_max
            return p

    def __init__(self, sensor, object_model, params):
        self.sensor, self.object_model, self.params = sensor, object_model, params

    def build(self):
        return GaussianTracker(self.sensor, self.object_model, self.params)


class GaussianTracker:
    """The robust Gaussian tracker on the sensor's device.  The C tracker borrows the sensor's
    handle: close() (or the sensor's own close()) releases it first.  A sensor drives one tracker
    at a time."""

    def __init__(self, sensor, object_model, params):
        self._lib = _capi.load()
        self.sensor, self.params = sensor, params
        self.parts = object_model.count_parts
        self.centers = np.array(object_model.centers)
        self.D = self.parts * BODY
        self.default = np.zeros(self.D)
        self.moving_average = None
        self._cov = None
        self._g = C.c_void_p()
        sensor._check(self._lib.rbs_gauss_create(sensor._h, C.byref(params.c_params()), C.byref(self._g)))
        sensor._register_dependent(self)

    def close(self):
        if getattr(self, "_g", None) is not None and self._g.value:
            self._lib.rbs_gauss_destroy(self._g)
            self._g = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _live(self):
        if not self._g.value:
            raise RbSensorError(_capi.RBS_ERR_INVALID_ARGUMENT, "GaussianTracker is closed")

    # -- State <-> model coordinates: ParticleTracker's rule (it reads parts, centers, params.center_object_frame)
    _to_model = ParticleTracker._to_model
    _from_model = ParticleTracker._from_model
    # -- the last estimate judged against its frame: ParticleTracker's method (it reads moving_average, sensor, _in_flight)
    assess = ParticleTracker.assess
    _in_flight = 0

    # -- Tracker interface -------------------------------------------------------------------
    def initialize(self, initial_states, cov0=None):
        """initial_states: list of State vectors (parts*12); the first is the default pose (velocities
        zeroed), the mean delta starts at 0 and the covariance at cov0 (D x D) or, None, per body
        diag(lin^2, ang^2, lin^2, ang^2) of the transition's sigmas."""
        self._live()
        self.default = self._to_model(initial_states[0])
        self.default.reshape(self.parts, BODY)[:, 6:12] = 0.0
        d = np.ascontiguousarray(self.default, dtype=np.float64)
        c = None if cov0 is None else np.ascontiguousarray(cov0, dtype=np.float64).reshape(self.D, self.D)
        dp = C.POINTER(C.c_double)
        self.sensor._check(self._lib.rbs_gauss_initialize(self._g, d.ctypes.data_as(dp), None if c is None else c.ctypes.data_as(dp)))
        self._cov = None if c is None else c.copy()
        self.moving_average = None
        self._in_flight = 0   # (rbs_gauss_initialize drops frames still in flight)

    def track(self, image):
        """One depth frame (float32 or float64, rows*cols metres, NaN = no reading) -> State.  image=None: the frame
        an earlier sensor.set_observation* call staged."""
        self._live()
        f64 = isinstance(image, np.ndarray) and image.dtype == np.float64
        out = np.empty(self.D)
        cov = np.empty((self.D, self.D))
        dp = C.POINTER(C.c_double)
        if image is None:
            rc = self._lib.rbs_gauss_track(self._g, None, out.ctypes.data_as(dp), cov.ctypes.data_as(dp))
        elif f64:
            img = np.ascontiguousarray(image, dtype=np.float64).ravel()
            rc = self._lib.rbs_gauss_track_f64(self._g, img.ctypes.data_as(dp), out.ctypes.data_as(dp), cov.ctypes.data_as(dp))
        else:
            img = np.ascontiguousarray(image, dtype=np.float32).ravel()
            rc = self._lib.rbs_gauss_track(self._g, img.ctypes.data_as(C.POINTER(C.c_float)), out.ctypes.data_as(dp),
                                           cov.ctypes.data_as(dp))
        self.sensor._check(rc)
        return self._finish(out, cov)

    def submit(self, image=None):
        """Enqueue one frame (rbs_gauss_submit: the whole filter step on the device) and return at once; at most two
        frames may be in flight.  result() hands out the estimates in submission order.  image: as track()."""
        self._live()
        if image is None:
            rc = self._lib.rbs_gauss_submit(self._g, None)
        elif isinstance(image, np.ndarray) and image.dtype == np.float64:
            img = np.ascontiguousarray(image, dtype=np.float64).ravel()
            rc = self._lib.rbs_gauss_submit_f64(self._g, img.ctypes.data_as(C.POINTER(C.c_double)))
        else:
            img = np.ascontiguousarray(image, dtype=np.float32).ravel()
            rc = self._lib.rbs_gauss_submit(self._g, img.ctypes.data_as(C.POINTER(C.c_float)))
        self.sensor._check(rc)   # (the library has staged the frame: the buffer is the caller's again)
        self._in_flight += 1

    def result(self):
        """The moving-average estimate of the oldest submitted frame (rbs_gauss_result); covariance is updated here."""
        self._live()
        out = np.empty(self.D)
        cov = np.empty((self.D, self.D))
        dp = C.POINTER(C.c_double)
        self.sensor._check(self._lib.rbs_gauss_result(self._g, out.ctypes.data_as(dp), cov.ctypes.data_as(dp)))
        self._in_flight = max(0, self._in_flight - 1)
        return self._finish(out, cov)

    def _finish(self, out, cov):
        self.default, self._cov = out, cov
        est = self._from_model(out)
        rate = self.params.moving_average_update_rate
        self.moving_average = est if self.moving_average is None else rate * est + (1 - rate) * self.moving_average
        return self.moving_average.copy()

    @property
    def covariance(self):
        """The belief's covariance (D x D, model coordinates, state order) after the last frame (before the
        first: cov0 as given to initialize, or None for the library's default)."""
        return None if self._cov is None else self._cov.copy()

    # -- inspection (parity tests, tools) ----------------------------------------------------
    def prior(self):
        """(default state z, predicted mean, predicted covariance) of the last frame."""
        self._live()
        z, m, c = np.empty(self.D), np.empty(self.D), np.empty((self.D, self.D))
        dp = C.POINTER(C.c_double)
        self.sensor._check(self._lib.rbs_gauss_get_prior(self._g, z.ctypes.data_as(dp), m.ctypes.data_as(dp), c.ctypes.data_as(dp)))
        return z, m, c

    def sigma_poses(self):
        """The last frame's distinct sigma poses [1 + 12 parts, parts, 12] (R|t)."""
        self._live()
        n = C.c_int32()
        self.sensor._check(self._lib.rbs_gauss_get_sigma_poses(self._g, None, C.byref(n)))
        out = np.empty((n.value, self.parts, 12))
        self.sensor._check(self._lib.rbs_gauss_get_sigma_poses(self._g, out.ctypes.data_as(C.POINTER(C.c_double)), C.byref(n)))
        return out

    def render(self, k):
        """Depth image [rows*cols] float32 of sigma pose k (+inf where nothing is covered)."""
        self._live()
        out = np.empty(self.sensor.rows * self.sensor.cols, dtype=np.float32)
        self.sensor._check(self._lib.rbs_gauss_get_render(self._g, int(k), out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def moments(self, raw=False):
        """The last frame's reduced moments in the whitened space: (Lambda [6 parts, 6 parts] with the identity added,
        eta [6 parts]), GaussTwin.whitened_update's convention.  raw=True: the entries exactly as the library read
        them from the device, [6p(6p+1)/2 + 6p] -- the upper triangle of Lambda - I row-major, then eta."""
        self._live()
        NP = 6 * self.parts
        out = np.empty(NP * (NP + 1) // 2 + NP)
        n = C.c_int32()
        self.sensor._check(self._lib.rbs_gauss_get_moments(self._g, out.ctypes.data_as(C.POINTER(C.c_double)), C.byref(n)))
        if n.value != out.size:
            raise RbSensorError(_capi.RBS_ERR_INVALID_ARGUMENT, f"gauss_get_moments: {n.value} entries, expected {out.size}")
        if raw:
            return out
        iu = np.triu_indices(NP)
        lam = np.zeros((NP, NP))
        lam[iu] = out[:iu[0].size]
        lam = lam + np.triu(lam, 1).T + np.eye(NP)
        return lam, out[iu[0].size:].copy()

    def kernel_ms(self):
        """Device ms of the last frame: (render, moments, reduction; after submit / result: reduction + update)."""
        self._live()
        out = (C.c_float * 3)()
        self.sensor._check(self._lib.rbs_gauss_kernel_ms(self._g, out))
        return tuple(float(v) for v in out)

