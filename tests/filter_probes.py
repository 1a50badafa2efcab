"""ctypes wrapper of rbs_test_filter, the particle filter's probe in the TEST build of the library
(dbot_ros_amd/csrc/rbsensor_probes.hip, librbsensor_mi355x_hooks.so), the synthetic filter states the device tests feed
it, and the child re-run two builds of the library need.  Test infrastructure."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np

FILTER_SYMBOLS = ("rbs_test_filter",)
RBS_OK, RBS_ERR_INVALID_ARGUMENT = 0, -1
BODY = 12
PROPAGATE, WEIGHTS, RESAMPLE_GATHER, GATHER, FILTER_TAIL, FILTER_STEP, MEAN, RECENTRE, SWAP = range(9)
SENTINEL, ISENTINEL = 7.25, -7      # what the arrays no input fills hold before a call

_DOUBLES = ("part_old", "part_new", "part_old2", "part_new2", "noise", "noise2", "logw", "ll", "ll2", "ll_new", "cdf")
_INTS = ("idx", "idx2", "parents")
_ORDER = _DOUBLES + _INTS + ("deflt", "mean", "poses", "flag", "normals", "uniforms", "host_state", "host_flags")
ARRAYS = tuple(k for k in _ORDER if k not in ("normals", "uniforms"))


class FilterIO(C.Structure):
    _fields_ = ([("n", C.c_int32), ("parts", C.c_int32), ("sigma", C.c_double * 6), ("vf", C.c_double), ("max_kl", C.c_double),
                 ("seed", C.c_uint64), ("frame", C.c_uint64)] + [(k, C.c_void_p) for k in _ORDER])


class FilterStep(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("code", "b", "updated", "last", "recentre")]


def step(code, b=0, updated=0, last=0, recentre=0):
    return (code, b, updated, last, recentre)


def shapes(n, parts):
    D = parts * BODY
    s = {k: (n, D) for k in ("part_old", "part_new", "part_old2", "part_new2")}
    s.update({k: (n, parts, 6) for k in ("noise", "noise2")})
    s.update({k: (n,) for k in ("logw", "ll", "ll2", "ll_new", "cdf", "idx", "idx2", "parents")})
    s.update(deflt=(D,), mean=(D + parts * 9,), poses=(n, parts, 12), flag=(2,), host_state=(D,), host_flags=(3,),
             normals=(parts, n, 6), uniforms=(parts, n))
    return s


def dtype_of(name):
    return np.int32 if name in _INTS + ("flag", "host_flags") else np.float64


class FilterProbe:
    def __init__(self, path):
        self.lib = C.CDLL(path)
        self.lib.rbs_test_filter.restype = C.c_int32

    def raw(self, io, steps, n_steps):
        return self.lib.rbs_test_filter(io, steps, C.c_int32(n_steps))

    def pack(self, state, steps):
        """-> (FilterIO, step array, the arrays the call will write: copies of the state's)."""
        n, parts = state["n"], state["parts"]
        io = FilterIO(n=n, parts=parts, vf=state["vf"], max_kl=state["max_kl"], seed=state["seed"], frame=state["frame"])
        io.sigma = (C.c_double * 6)(*state["sigma"])
        out = {}
        for name, shape in shapes(n, parts).items():
            a = state.get(name)
            if a is None:
                assert name in ("normals", "uniforms"), name
                continue
            a = np.array(a, dtype=dtype_of(name), order="C")     # (a copy: the caller's state stays as it was)
            assert a.shape == shape, (name, a.shape, shape)
            out[name] = a
            setattr(io, name, a.ctypes.data_as(C.c_void_p))
        arr = (FilterStep * max(1, len(steps)))(*[FilterStep(*s) for s in steps])
        return io, arr, out

    def run(self, state, steps):
        io, arr, out = self.pack(state, steps)
        rc = self.raw(C.byref(io), arr, len(steps))
        assert rc == RBS_OK, rc
        return out


def make_state(n, parts, seed, max_kl=2.0, frame=0, rng_seed=0):
    """A filter state before a sampling block's weight step: small random deltas around a random default pose, flat
    log-likelihoods (ll_new == ll) and zero log-weights; every array no input fills holds its sentinel."""
    rng = np.random.default_rng([n, parts, rng_seed])
    D = parts * BODY
    scale = np.tile(np.repeat([0.01, 0.05, 0.002, 0.02], 3), parts)
    st = dict(n=n, parts=parts, sigma=[0.0025] * 3 + [0.02] * 3, vf=0.8, max_kl=max_kl, seed=seed, frame=frame)
    st["part_old"] = rng.standard_normal((n, D)) * scale
    st["part_new"] = rng.standard_normal((n, D)) * scale
    st["noise"] = rng.standard_normal((n, parts, 6))
    st["logw"] = np.zeros(n)
    st["ll"] = rng.normal(-500.0, 20.0, n)
    st["ll_new"] = st["ll"].copy()
    st["idx"] = rng.integers(0, n, n).astype(np.int32)
    z = np.zeros((parts, BODY))
    z[:, 0:3] = rng.normal([0.0, 0.0, 1.0], 0.1, (parts, 3))
    z[:, 3:6] = rng.normal(0.0, 0.7, (parts, 3))
    st["deflt"] = z.ravel()
    st["flag"] = np.array([0, 5], dtype=np.int32)
    st["normals"] = rng.standard_normal((parts, n, 6))
    st["uniforms"] = rng.random((parts, n))
    for name, shape in shapes(n, parts).items():
        if name not in st:
            st[name] = np.full(shape, ISENTINEL if dtype_of(name) == np.int32 else SENTINEL, dtype=dtype_of(name))
    return st


# ---------------------------------------------------------------- the hooks build in a child
def hooks_path(lib_path):
    return os.path.join(os.path.dirname(os.path.abspath(lib_path)), "librbsensor_mi355x_hooks.so")


def child_outcomes(test_file, hooks, timeout):
    """Re-run `test_file` once with RBS_LIB_PATH set to the hooks build: {test id: PASSED | FAILED | ERROR} and the output's end."""
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-rA", "-m", "gpu", "-p", "no:cacheprovider", test_file],
                       capture_output=True, text=True, timeout=timeout, env=dict(os.environ, RBS_LIB_PATH=hooks))
    outcome = dict((m.group(2), m.group(1)) for m in re.finditer(r"^(PASSED|FAILED|ERROR) \S+?::(\S+)", r.stdout, re.M))
    return outcome, r.stdout[-8000:] + r.stderr[-2000:]
