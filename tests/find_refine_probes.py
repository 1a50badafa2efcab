"""ctypes wrappers of rbs_test_findr_*, the probes of the object finder's step 6b in the TEST build of the library
(dbot_ros_amd/csrc/rbsensor_probes.hip, librbsensor_mi355x_hooks.so): rbf::launch_refine_init + launch_refine_children and
rbf::launch_refine_update.  As in tests/find_probes.py every output array is `TAIL` elements (rows) longer than the kernel
may write and filled with a sentinel before the call, and the whole array is handed back.  Test infrastructure."""
import ctypes as C

import numpy as np

from find_probes import RBS_ERR_INVALID_ARGUMENT, RBS_OK, TAIL, _p, child_outcomes, hooks_path, sentinel, untouched  # noqa: F401

FINDR_SYMBOLS = ("rbs_test_findr_children", "rbs_test_findr_update")

_i32, _i64, _u64, _f64 = C.c_int32, C.c_int64, C.c_uint64, C.c_double


class RefinementProbe:
    def __init__(self, path):
        self.lib = C.CDLL(path)
        for s in FINDR_SYMBOLS:
            getattr(self.lib, s).restype = C.c_int32

    def children(self, surv, n_children, rnd, seed, factors=None, sigma_angle=0.0, sigma_translation=0.0, jitter=0.0):
        """factors [S][36]: the children through them; None: through the factors the device makes of the initial covariance
        of (sigma_angle, sigma_translation).  -> poses [S * children + TAIL][12], d [S * children + TAIL][6],
        cov [S + TAIL][36] (None when factors are given)."""
        surv = np.ascontiguousarray(surv, dtype=np.float64)
        S = len(surv)
        fac = None if factors is None else np.ascontiguousarray(factors, dtype=np.float64).reshape(S, 36)
        cov = sentinel((S + TAIL, 36), np.float64) if fac is None else None
        out = sentinel((S * n_children + TAIL, 12), np.float64)
        dd = sentinel((S * n_children + TAIL, 6), np.float64)
        rc = self.lib.rbs_test_findr_children(_p(surv), _p(fac), _i32(S), _i32(n_children), _i32(rnd), _u64(seed), _f64(sigma_angle),
                                              _f64(sigma_translation), _f64(jitter), _p(cov), _p(out), _p(dd), _i64(TAIL))
        assert rc == RBS_OK, rc
        return out, dd, cov

    def update(self, scores, d, cov, elite, mix, shrink, jitter):
        """scores [S][children], d [S][children][6], cov [S][36] -> cov' [S + TAIL][36], factors [S + TAIL][36]."""
        scores = np.ascontiguousarray(scores, dtype=np.float64)
        S, n_children = scores.shape
        d = np.ascontiguousarray(d, dtype=np.float64).reshape(S, n_children, 6)
        c = sentinel((S + TAIL, 36), np.float64)
        c[:S] = np.asarray(cov, dtype=np.float64).reshape(S, 36)
        fac = sentinel((S + TAIL, 36), np.float64)
        rc = self.lib.rbs_test_findr_update(_p(scores), _p(d), _i32(S), _i32(n_children), _i32(elite), _f64(mix), _f64(shrink), _f64(jitter),
                                            _p(c), _p(fac), _i64(TAIL))
        assert rc == RBS_OK, rc
        return c, fac
