"""CPU-side checks of the pose assessor (rbs_assess_*, include/rbsensor_mi355x.h): the numpy twin of the rule on planted
planes and frames, and what the library answers without a device -- the verdict (a pure host function), the exported
symbols, the refusals and the record's layout."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import assess_twin as tw
from dbot_ros_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# a noise model whose tau is exact in binary: sigmas (ms + sf d d) = 3 (2^-8 + 2^-10) = 15 / 1024 at d = 1
MS, SF = 2.0 ** -8, 2.0 ** -10
INF = np.float32(np.inf)


def f32(*v):
    return np.array(v, dtype=np.float32)


# ---------------------------------------------------------------------------------------------- the twin
def test_ties_go_to_the_lowest_body():
    planes = np.stack([f32(1.0, 1.0, INF, 2.0), f32(1.0, 0.5, 1.0, INF), f32(1.0, 0.5, 1.0, 2.0)])
    owner, best = tw.owners(planes)
    assert owner.tolist() == [0, 1, 1, 0]
    assert best.tolist() == [1.0, 0.5, 1.0, 2.0]
    c = tw.counts(planes, f32(1.0, 0.5, 1.0, 2.0), MS, SF)
    assert c[:, 0].tolist() == [2, 2, 0]          # a duplicate of a lower body owns nothing
    assert c[:, 2].tolist() == [2, 2, 0]


def test_reading_equal_to_the_depth_is_support():
    c = tw.counts(f32(1.0, 0.7, 3.25)[None], f32(1.0, 0.7, 3.25), 0.003, 0.0014247)
    assert c.tolist() == [[3, 3, 3, 0, 0]]


def test_the_class_boundaries_are_inclusive_and_one_ulp_decides():
    tau = 15.0 / 1024.0
    assert 3.0 * (MS + SF * 1.0) == tau
    hi, lo = np.float32(1.0 + tau), np.float32(1.0 - tau)
    assert float(hi) - 1.0 == tau and float(lo) - 1.0 == -tau          # the frame's float holds d +- tau exactly
    ys = f32(hi, np.nextafter(hi, INF), np.nextafter(hi, -INF), lo, np.nextafter(lo, -INF), np.nextafter(lo, INF))
    for y, want in zip(ys, ("support", "behind", "support", "support", "in_front", "support")):
        c = tw.counts(f32(1.0)[None], f32(y), MS, SF)[0]
        col = {"support": 2, "in_front": 3, "behind": 4}[want]
        assert c.tolist() == [1, 1] + [1 if k == col else 0 for k in (2, 3, 4)], (float(y), want)


def test_readings_that_are_not_finite_zero_or_negative():
    planes = np.full((1, 6), 1.0, dtype=np.float32)
    frame = f32(np.inf, -np.inf, np.nan, 0.0, -2.0, 1.0)
    c = tw.counts(planes, frame, MS, SF)[0]
    # +-inf and NaN: no reading; 0 and negative depths are finite readings far in front of the body
    assert c.tolist() == [6, 3, 1, 2, 0]


def test_empty_planes_own_nothing():
    planes = np.full((3, 50), np.inf, dtype=np.float32)
    c, v = tw.assess(planes, np.ones(50, dtype=np.float32), MS, SF)
    assert not c.any() and v.tolist() == [tw.OUT_OF_VIEW] * 3
    planes[1, :20] = 1.0                                               # one body alone in view
    c, v = tw.assess(planes, np.ones(50, dtype=np.float32), MS, SF)
    assert c.tolist() == [[0] * 5, [20, 20, 20, 0, 0], [0] * 5]
    assert v.tolist() == [tw.OUT_OF_VIEW, tw.SUPPORTED, tw.OUT_OF_VIEW]


def test_the_verdict_rule_in_order():
    assert tw.verdict([15, 15, 15, 0, 0]) == tw.OUT_OF_VIEW            # 1. too few pixels, whatever they say
    assert tw.verdict([100, 100, 10, 80, 10]) == tw.OCCLUDED           # 2. u = 20 < 25
    assert tw.verdict([100, 100, 13, 75, 12]) == tw.SUPPORTED          # 3. u = 25, support 13 >= 12.5
    assert tw.verdict([100, 100, 12, 75, 13]) == tw.LOST               # 4.
    assert tw.verdict([100, 0, 0, 0, 0]) == tw.OCCLUDED                # an all-NaN frame decides nothing
    assert tw.verdict([100, 0, 0, 0, 0], min_visible_fraction=0.0) == tw.SUPPORTED   # 0 >= 0.5 x 0: the rule as written


# ---------------------------------------------------------------------------------------------- the library, no device
def lib_verdict(lib, c, params=None):
    body = _capi.RbsAssessBody(*(int(v) for v in c[:5]))
    v = C.c_int32(-7)
    p = None
    if params is not None:
        p = _capi.RbsAssessParams(params["sigmas"], params["min_support_fraction"], params["min_visible_fraction"],
                                  params["min_pixels"], 0)
    rc = lib.rbs_assess_verdict(C.byref(p) if p is not None else None, C.byref(body), C.byref(v))
    return rc, v.value


def test_library_verdict_equals_the_twin_on_random_records():
    lib = _capi.load()
    rng = np.random.default_rng(5)
    seen = set()
    for _ in range(4000):
        rendered = int(rng.choice([0, 1, 15, 16, 17, 100, 1000, 307200]))
        valid = int(rng.integers(0, rendered + 1))
        parts = rng.multinomial(valid, rng.dirichlet(np.ones(3) * 0.5))
        c = [rendered, valid, int(parts[0]), int(parts[1]), int(parts[2])]
        params = dict(sigmas=float(rng.choice([1.0, 3.0])), min_support_fraction=float(rng.choice([0.0, 0.25, 0.5, 0.9, 1.0])),
                      min_visible_fraction=float(rng.choice([0.0, 0.25, 0.5, 1.0])), min_pixels=int(rng.choice([1, 16, 64])))
        rc, v = lib_verdict(lib, c, params)
        assert rc == _capi.RBS_OK
        assert v == tw.verdict(c, **params), (c, params)
        seen.add(v)
    assert seen == {0, 1, 2, 3}


def test_library_verdict_on_each_boundary_and_the_defaults():
    lib = _capi.load()
    d = _capi.RbsAssessParams()
    lib.rbs_assess_default_params(C.byref(d))
    assert (d.sigmas, d.min_support_fraction, d.min_visible_fraction, d.min_pixels, d.reserved) == (3.0, 0.5, 0.25, 16, 0)
    assert tw.DEFAULTS == dict(sigmas=3.0, min_support_fraction=0.5, min_visible_fraction=0.25, min_pixels=16)
    cases = [([15, 15, 15, 0, 0], tw.OUT_OF_VIEW), ([16, 16, 16, 0, 0], tw.SUPPORTED),        # rendered < min_pixels
             ([100, 100, 24, 76, 0], tw.OCCLUDED), ([100, 100, 25, 75, 0], tw.SUPPORTED),      # u < 0.25 rendered
             ([100, 100, 20, 60, 20], tw.SUPPORTED), ([100, 100, 20, 59, 21], tw.LOST),        # support >= 0.5 u
             ([0, 0, 0, 0, 0], tw.OUT_OF_VIEW)]
    for c, want in cases:
        assert tw.verdict(c) == want, c
        assert lib_verdict(lib, c) == (_capi.RBS_OK, want), c                                  # NULL params: the defaults
        assert lib_verdict(lib, c, tw.DEFAULTS) == (_capi.RBS_OK, want), c


def test_symbols_are_declared_and_exported():
    text = open(os.path.join(ROOT, "include", "rbsensor_mi355x.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = C.CDLL(_capi.LIB_PATH)
    names = ("rbs_assess_default_params", "rbs_assess_poses", "rbs_assess_verdict", "rbs_assess_get_plane", "rbs_assess_kernel_ms")
    for s in names:
        assert re.search(r"\b" + s + r"\s*\(", text), s
        assert s in _capi.EXPORTS and hasattr(lib, s), s
    assert sorted(set(re.findall(r"\b(rbs_assess_[a-z0-9_]+)\s*\(", text))) == sorted(names)
    for k, name in enumerate(("RBS_ASSESS_OUT_OF_VIEW", "RBS_ASSESS_OCCLUDED", "RBS_ASSESS_SUPPORTED", "RBS_ASSESS_LOST")):
        assert re.search(name + r"\s*=\s*%d\b" % k, text) and getattr(_capi, name) == k
    release = open(_capi.LIB_PATH, "rb").read() if _capi.LIB_PATH.endswith("librbsensor_mi355x.so") else b""
    assert b"rbs_test_assess" not in release
    src = open(os.path.join(ROOT, "dbot_ros_amd", "csrc", "rbsensor_assess.hip")).read()
    kernels = re.findall(r"__global__[^\n]*?void\s+(\w+)\s*\(", src)
    assert kernels == ["rbs_assess_count_kernel"]          # (the planes: rbs_planes_render_kernel, shared, rbs_pose_planes.h)
    shared = open(os.path.join(ROOT, "dbot_ros_amd", "csrc", "rbs_pose_planes.h")).read()
    assert re.findall(r"__global__[^\n]*?void\s+(\w+)\s*\(", shared) == ["rbs_planes_render_kernel"]
    assert not any(re.fullmatch(r"rbs_find_\w*_kernel", k) for k in kernels)


def test_record_and_params_layout():
    assert C.sizeof(_capi.RbsAssessBody) == 32 and _capi.RbsAssessBody.verdict.offset == 20
    assert C.sizeof(_capi.RbsAssessParams) == 32 and _capi.RbsAssessParams.min_pixels.offset == 24
    src = open(os.path.join(ROOT, "dbot_ros_amd", "csrc", "rbsensor_assess.hip")).read()
    assert "static_assert(sizeof(rbs_assess_body) == 32" in src


def test_bad_arguments_are_refused_before_any_device_call():
    lib = _capi.load()
    inv = _capi.RBS_ERR_INVALID_ARGUMENT
    poses = np.zeros(12)
    out = (_capi.RbsAssessBody * 1)()
    assert lib.rbs_assess_poses(None, None, None, poses.ctypes.data_as(C.POINTER(C.c_double)), 1, out) == inv
    plane = np.zeros(4, dtype=np.float32)
    assert lib.rbs_assess_get_plane(None, 0, 0, plane.ctypes.data_as(C.POINTER(C.c_float))) == inv
    assert lib.rbs_assess_kernel_ms(None, (C.c_float * 2)()) == inv
    lib.rbs_assess_default_params(None)   # no-op
    body, v = _capi.RbsAssessBody(100, 100, 50, 0, 50), C.c_int32()
    assert lib.rbs_assess_verdict(None, None, C.byref(v)) == inv
    assert lib.rbs_assess_verdict(None, C.byref(body), None) == inv
    good = dict(tw.DEFAULTS)
    for key, bad in (("sigmas", 0.0), ("sigmas", -1.0), ("sigmas", float("inf")), ("sigmas", float("nan")),
                     ("min_support_fraction", -0.1), ("min_support_fraction", 1.5), ("min_support_fraction", float("nan")),
                     ("min_visible_fraction", -0.1), ("min_visible_fraction", 1.0001), ("min_visible_fraction", float("nan")),
                     ("min_pixels", 0), ("min_pixels", -3)):
        rc, _ = lib_verdict(lib, [100, 100, 50, 0, 50], dict(good, **{key: bad}))
        assert rc == inv, (key, bad)
    assert lib_verdict(lib, [100, 100, 50, 0, 50], good) == (_capi.RBS_OK, tw.SUPPORTED)


def test_python_parameters_mirror_the_c_defaults():
    from dbot_ros_amd.assess import PoseAssessor
    p = PoseAssessor.Parameters()
    assert (p.sigmas, p.min_support_fraction, p.min_visible_fraction, p.min_pixels) == (3.0, 0.5, 0.25, 16)
    q = PoseAssessor.Parameters.from_mapping({"sigmas": 2, "min_pixels": 8})
    assert (q.sigmas, q.min_pixels) == (2.0, 8)
    with pytest.raises(ValueError):
        PoseAssessor.Parameters.from_mapping({"sigma": 2})
