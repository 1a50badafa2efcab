"""ctypes wrappers of rbs_test_find_*, the object finder's probes in the TEST build of the library
(dbot_ros_amd/csrc/rbsensor_probes.hip, librbsensor_mi355x_hooks.so): one per launch helper of rbsensor_find.hip.  Every output
array is `TAIL` elements (rows) longer than the kernel may write and filled with a sentinel before the call; the wrappers hand
back the whole array, so a test sees what was written, what was left alone and whether the tail still holds the sentinel.
Test infrastructure."""
import ctypes as C

import numpy as np

from filter_probes import RBS_ERR_INVALID_ARGUMENT, RBS_OK, child_outcomes, hooks_path  # noqa: F401  (re-exported)

FIND_SYMBOLS = ("rbs_test_find_subsample", "rbs_test_find_seeds", "rbs_test_find_hyp", "rbs_test_find_topk", "rbs_test_find_nms",
                "rbs_test_find_children", "rbs_test_find_select", "rbs_test_find_order")
TAIL = 5
SENTINEL, ISENTINEL = 7.25, -7
MAX_SURVIVORS, MAX_CANDIDATES, TOP_CHUNK = 64, 1024, 2048      # kMaxSurvivors, kMaxCandidates, kTopC

_i32, _i64, _u64, _f64 = C.c_int32, C.c_int64, C.c_uint64, C.c_double


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def sentinel(shape, dtype):
    return np.full(shape, SENTINEL if np.dtype(dtype).kind == "f" else ISENTINEL, dtype=dtype)


def untouched(a):
    return bool(np.all(a == (SENTINEL if a.dtype.kind == "f" else ISENTINEL)))


class FindProbe:
    def __init__(self, path):
        self.lib = C.CDLL(path)
        for s in FIND_SYMBOLS:
            getattr(self.lib, s).restype = C.c_int32

    def subsample(self, frame, rows, cols, f):
        """-> dst [(rows // f) * (cols // f) + TAIL] float32."""
        src = np.ascontiguousarray(frame, dtype=np.float32).ravel()
        dst = sentinel((rows // f) * (cols // f) + TAIL, np.float32)
        rc = self.lib.rbs_test_find_subsample(_p(src), _i32(rows), _i32(cols), _i32(f), _p(dst), _i64(TAIL))
        assert rc == RBS_OK, rc
        return dst

    def seeds(self, frame, rows, cols, stride, dmin, dmax, max_seeds):
        """-> cells [ncell + TAIL], seeds [min(max_seeds, ncell) + TAIL][4], info [2 + TAIL]."""
        src = np.ascontiguousarray(frame, dtype=np.float32).ravel()
        ncell = -(-rows // stride) * -(-cols // stride)
        cells = sentinel(ncell + TAIL, np.int32)
        seeds = sentinel((min(max_seeds, ncell) + TAIL, 4), np.float64)
        info = sentinel(2 + TAIL, np.int32)
        rc = self.lib.rbs_test_find_seeds(_p(src), _i32(rows), _i32(cols), _i32(stride), _f64(dmin), _f64(dmax), _i32(max_seeds),
                                          _p(cells), _p(seeds), _p(info), _i64(TAIL))
        assert rc == RBS_OK, rc
        return cells, seeds, info

    def hyp(self, seeds, n_rot, K, offset, h0=0, n=0, idx=None):
        """idx None: hypotheses h0 .. h0 + n - 1 (rbs_find_hyp_kernel); else those of idx (rbs_find_gather_kernel).
        -> poses [n + TAIL][12]."""
        seeds = np.ascontiguousarray(seeds, dtype=np.float64)
        idx = None if idx is None else np.ascontiguousarray(idx, dtype=np.int64)
        n = n if idx is None else len(idx)
        poses = sentinel((n + TAIL, 12), np.float64)
        rc = self.lib.rbs_test_find_hyp(_p(seeds), _i32(len(seeds)), _i32(n_rot), _f64(K[0][0]), _f64(K[1][1]), _f64(K[0][2]), _f64(K[1][2]),
                                        _f64(offset), _i64(h0), _p(idx), _i32(n), _p(poses), _i64(TAIL))
        assert rc == RBS_OK, rc
        return poses

    def topk(self, scores, idx, k):
        """-> out_score [k], out_idx [k], the ping-pong buffers' tails (tail_s, tail_i) [2][TAIL], passes."""
        scores = np.ascontiguousarray(scores, dtype=np.float64)
        idx = None if idx is None else np.ascontiguousarray(idx, dtype=np.int64)
        out_s, out_i = sentinel(k, np.float64), sentinel(k, np.int64)
        tail_s, tail_i = sentinel((2, TAIL), np.float64), sentinel((2, TAIL), np.int64)
        passes = _i32(0)
        rc = self.lib.rbs_test_find_topk(_p(scores), _p(idx), _i64(len(scores)), _i32(k), _p(out_s), _p(out_i), _p(tail_s), _p(tail_i),
                                         _i64(TAIL), C.byref(passes))
        assert rc == RBS_OK, rc
        return out_s, out_i, tail_s, tail_i, passes.value

    def nms(self, poses, scores, idx, nms_t, nms_a, max_keep):
        """-> kept [64 + TAIL], count [1 + TAIL], surv [max_keep + TAIL][12], surv_score, surv_idx [max_keep + TAIL]."""
        poses = np.ascontiguousarray(poses, dtype=np.float64)
        scores = np.ascontiguousarray(scores, dtype=np.float64)
        idx = np.ascontiguousarray(idx, dtype=np.int64)
        kept, count = sentinel(MAX_SURVIVORS + TAIL, np.int32), sentinel(1 + TAIL, np.int32)
        surv = sentinel((max_keep + TAIL, 12), np.float64)
        surv_score, surv_idx = sentinel(max_keep + TAIL, np.float64), sentinel(max_keep + TAIL, np.int64)
        rc = self.lib.rbs_test_find_nms(_p(poses), _p(scores), _p(idx), _i32(len(scores)), _f64(nms_t), _f64(nms_a), _i32(max_keep),
                                        _p(kept), _p(count), _p(surv), _p(surv_score), _p(surv_idx), _i64(TAIL))
        assert rc == RBS_OK, rc
        return kept, count, surv, surv_score, surv_idx

    def children(self, surv, n_children, rnd, seed, st, sa):
        """-> out [S * children + TAIL][12]."""
        surv = np.ascontiguousarray(surv, dtype=np.float64)
        out = sentinel((len(surv) * n_children + TAIL, 12), np.float64)
        rc = self.lib.rbs_test_find_children(_p(surv), _i32(len(surv)), _i32(n_children), _i32(rnd), _u64(seed), _f64(st), _f64(sa),
                                             _p(out), _i64(TAIL))
        assert rc == RBS_OK, rc
        return out

    def select(self, child, child_score, S, n_children):
        """-> surv [S + TAIL][12], surv_score [S + TAIL]."""
        child = np.ascontiguousarray(child, dtype=np.float64)
        child_score = np.ascontiguousarray(child_score, dtype=np.float64)
        surv, surv_score = sentinel((S + TAIL, 12), np.float64), sentinel(S + TAIL, np.float64)
        rc = self.lib.rbs_test_find_select(_p(child), _p(child_score), _i32(S), _i32(n_children), _p(surv), _p(surv_score), _i64(TAIL))
        assert rc == RBS_OK, rc
        return surv, surv_score

    def order(self, surv, surv_score, order):
        """-> out_pose [S + TAIL][12], out_score [S + TAIL]."""
        surv = np.ascontiguousarray(surv, dtype=np.float64)
        surv_score = np.ascontiguousarray(surv_score, dtype=np.float64)
        order = np.ascontiguousarray(order, dtype=np.int64)
        S = len(order)
        out_pose, out_score = sentinel((S + TAIL, 12), np.float64), sentinel(S + TAIL, np.float64)
        rc = self.lib.rbs_test_find_order(_p(surv), _p(surv_score), _p(order), _i32(S), _p(out_pose), _p(out_score), _i64(TAIL))
        assert rc == RBS_OK, rc
        return out_pose, out_score
