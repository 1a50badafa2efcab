"""ctypes wrappers of rbs_test_findfg_*, the probes of the object finder's step 1b in the TEST build of the library
(dbot_ros_amd/csrc/rbsensor_probes.hip, librbsensor_mi355x_hooks.so): one per launch helper (rbf::launch_plane_trials,
launch_plane_count, launch_plane_best, launch_mask).  As in tests/find_probes.py every output array is `TAIL` elements (rows)
longer than the kernel may write and filled with a sentinel before the call, and the whole array is handed back.
Test infrastructure."""
import ctypes as C

import numpy as np

from find_probes import RBS_ERR_INVALID_ARGUMENT, RBS_OK, TAIL, _p, child_outcomes, hooks_path, sentinel, untouched  # noqa: F401

FINDFG_SYMBOLS = ("rbs_test_findfg_trials", "rbs_test_findfg_count", "rbs_test_findfg_best", "rbs_test_findfg_mask")
RECORD, MAX_TRIALS = 8, 4096                                   # kFgRecord, kFgMaxTrials

_i32, _i64, _u64, _f64 = C.c_int32, C.c_int64, C.c_uint64, C.c_double


class ForegroundProbe:
    def __init__(self, path):
        self.lib = C.CDLL(path)
        for s in FINDFG_SYMBOLS:
            getattr(self.lib, s).restype = C.c_int32

    def trials(self, frame, rows, cols, dmin, dmax, seed, n_trials):
        """-> planes [n_trials + TAIL][4]."""
        src = np.ascontiguousarray(frame, dtype=np.float32).ravel()
        planes = sentinel((n_trials + TAIL, 4), np.float64)
        rc = self.lib.rbs_test_findfg_trials(_p(src), _i32(rows), _i32(cols), _f64(dmin), _f64(dmax), _u64(seed), _i32(n_trials),
                                             _p(planes), _i64(TAIL))
        assert rc == RBS_OK, rc
        return planes

    def counts(self, frame, rows, cols, dmin, dmax, model_sigma, sigma_factor, planes, ransac_sigmas):
        """-> counts [len(planes) + 1 + TAIL] int32."""
        src = np.ascontiguousarray(frame, dtype=np.float32).ravel()
        planes = np.ascontiguousarray(planes, dtype=np.float64).reshape(-1, 4)
        T = len(planes)
        out = sentinel(T + 1 + TAIL, np.int32)
        rc = self.lib.rbs_test_findfg_count(_p(src), _i32(rows), _i32(cols), _f64(dmin), _f64(dmax), _f64(model_sigma), _f64(sigma_factor),
                                            _p(planes) if T else None, _i32(T), _f64(ransac_sigmas), _p(out), _i64(TAIL))
        assert rc == RBS_OK, rc
        return out

    def best(self, planes, counts, min_inlier_fraction):
        """-> record [RECORD + TAIL]."""
        planes = np.ascontiguousarray(planes, dtype=np.float64).reshape(-1, 4)
        counts = np.ascontiguousarray(counts, dtype=np.int32)
        assert len(counts) == len(planes) + 1
        rec = sentinel(RECORD + TAIL, np.float64)
        rc = self.lib.rbs_test_findfg_best(_p(planes), _p(counts), _i32(len(planes)), _f64(min_inlier_fraction), _p(rec), _i64(TAIL))
        assert rc == RBS_OK, rc
        return rec

    def mask(self, frame, rows, cols, model_sigma, sigma_factor, rec, mask_sigmas):
        """-> the seeding frame [rows * cols + TAIL] float32."""
        src = np.ascontiguousarray(frame, dtype=np.float32).ravel()
        rec = np.ascontiguousarray(rec, dtype=np.float64)[:RECORD].copy()
        out = sentinel(rows * cols + TAIL, np.float32)
        rc = self.lib.rbs_test_findfg_mask(_p(src), _i32(rows), _i32(cols), _f64(model_sigma), _f64(sigma_factor), _p(rec), _f64(mask_sigmas),
                                           _p(out), _i64(TAIL))
        assert rc == RBS_OK, rc
        return out
