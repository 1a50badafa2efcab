"""ctypes wrapper of the value-by-value probes of the per-pixel likelihood (dbot_ros_amd/csrc/rbsensor_probes.hip):
entry points of the TEST build of the library only (librbsensor_mi355x_hooks.so), so they are no part of
dbot_ros_amd._capi.EXPORTS.  Test infrastructure."""
import ctypes as C

import numpy as np

PROBE_SYMBOLS = ("rbs_test_exp_nonpos", "rbs_test_erfc_pos", "rbs_test_log_f32", "rbs_test_div_f32", "rbs_test_rcp_f64",
                 "rbs_test_frame_terms", "rbs_test_pixel_f64", "rbs_test_pixel_f32")
RBS_OK, RBS_ERR_INVALID_ARGUMENT = 0, -1
LAMBDA = float(np.log(2.0))   # ln 2 / half_life_depth, half_life_depth = 1


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class Probes:
    def __init__(self, path):
        self.lib = C.CDLL(path)
        for s in PROBE_SYMBOLS:
            getattr(self.lib, s).restype = C.c_int32

    def _ok(self, rc):
        assert rc == RBS_OK, rc

    def _map(self, fn, x, in_dtype, out_dtype, *extra):
        x = np.ascontiguousarray(x, dtype=in_dtype)
        out = np.empty(x.size, dtype=out_dtype)
        self._ok(getattr(self.lib, fn)(_ptr(x), _ptr(out), C.c_int64(x.size), *extra))
        return out

    def exp_nonpos(self, x):
        return self._map("rbs_test_exp_nonpos", x, np.float64, np.float64)

    def erfc_pos(self, z, lds):
        return self._map("rbs_test_erfc_pos", z, np.float64, np.float64, C.c_int32(int(lds)))

    def log_f32(self, x, lds):
        return self._map("rbs_test_log_f32", x, np.float32, np.float64, C.c_int32(int(lds)))

    def rcp_f64(self, x):
        return self._map("rbs_test_rcp_f64", x, np.float64, np.float64)

    def div_f32(self, a, b):
        a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
        assert a.shape == b.shape
        out = np.empty(a.size, dtype=np.float32)
        self._ok(self.lib.rbs_test_div_f32(_ptr(a), _ptr(b), _ptr(out), C.c_int64(a.size)))
        return out

    @staticmethod
    def _model(tw, ms, sf, lam):
        return C.c_double(tw), C.c_double(ms), C.c_double(sf), C.c_double(lam)

    def frame_terms(self, obs, tw, ms, sf, lam=LAMBDA):
        obs = np.ascontiguousarray(obs, dtype=np.float32)
        out = np.empty((obs.size, 4))
        self._ok(self.lib.rbs_test_frame_terms(_ptr(obs), C.c_int64(obs.size), *self._model(tw, ms, sf, lam), _ptr(out)))
        return out

    def _pixel(self, fn, obs, depth, prior, tw, ms, sf, lam):
        o, r, p = (np.ascontiguousarray(v, dtype=np.float32) for v in (obs, depth, prior))
        assert o.shape == r.shape == p.shape
        term, post = np.empty(o.size), np.empty(o.size, dtype=np.float32)
        self._ok(getattr(self.lib, fn)(_ptr(o), _ptr(r), _ptr(p), C.c_int64(o.size), *self._model(tw, ms, sf, lam), _ptr(term), _ptr(post)))
        return term, post

    def pixel_f64(self, obs, depth, prior, tw, ms, sf, lam=LAMBDA):
        return self._pixel("rbs_test_pixel_f64", obs, depth, prior, tw, ms, sf, lam)

    def pixel_f32(self, obs, depth, prior, tw, ms, sf, lam=LAMBDA):
        return self._pixel("rbs_test_pixel_f32", obs, depth, prior, tw, ms, sf, lam)
