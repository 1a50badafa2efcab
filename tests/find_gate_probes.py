"""ctypes wrapper of rbs_test_findc_evidence, the probe of the finder's evidence kernel in the TEST build of the library
(dbot_ros_amd/csrc/rbsensor_probes.hip, librbsensor_mi355x_hooks.so): rbf::launch_evidence alone, over a sensor's geometry.  As
in tests/find_probes.py the output arrays are `TAIL` rows longer than the kernel may write and filled with a sentinel before the
call, and the whole arrays are handed back.  Test infrastructure."""
import ctypes as C

import numpy as np

from dbot_ros_amd import _capi
from find_probes import RBS_ERR_INVALID_ARGUMENT, RBS_OK, TAIL, _p, child_outcomes, hooks_path, sentinel, untouched  # noqa: F401

FINDC_SYMBOLS = ("rbs_test_findc_evidence",)
FIELDS = 10


def c_gate(params, require_confirmed=False):
    g = _capi.RbsFindGate()
    g.enabled, g.require_confirmed = 1, int(require_confirmed)
    for k, v in params.items():
        setattr(g, k, v)
    return g


class GateProbe:
    def __init__(self, path):
        self.lib = C.CDLL(path)
        for s in FINDC_SYMBOLS:
            getattr(self.lib, s).restype = C.c_int32

    def evidence(self, sensor, params, frame, poses):
        """sensor: an RbSensor of one body made by the same library.  -> rec [n + TAIL][10] int32, cls [n + TAIL] int32."""
        frame = np.ascontiguousarray(frame, dtype=np.float32).ravel()
        assert frame.size == sensor.rows * sensor.cols
        poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 12)
        n = len(poses)
        rec, cls = sentinel((n + TAIL, FIELDS), np.int32), sentinel(n + TAIL, np.int32)
        g = c_gate(params)
        rc = self.lib.rbs_test_findc_evidence(C.c_void_p(sensor._h.value), C.byref(g), _p(frame), _p(poses), C.c_int32(n), _p(rec), _p(cls),
                                              C.c_int64(TAIL))
        assert rc == RBS_OK, rc
        return rec, cls
