"""The object finder's host-side contract without a GPU: the numpy twin's own checks, the compiler's report for
the finder's kernels, the exported C-ABI and the parameter checks of rbs_find_create."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import find_twin as tw
from dbot_ros_amd import _capi
from dbot_ros_amd.finder import ObjectFinder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("subsample", "seed", "hyp", "gather", "topk", "nms", "children", "select", "order", "keep")


def test_philox_known_answer():
    # Random123's Philox4x32-10 known-answer vector: key 0, counter 0
    assert tw.philox(0, 0, 0) == (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)


def test_super_fibonacci_grid():
    q = tw.sf_quaternions(1024)
    assert q.shape == (1024, 4)
    assert np.abs(np.linalg.norm(q, axis=1) - 1.0).max() < 1e-15
    R = tw.sf_rotations(1024).reshape(-1, 3, 3)
    assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() < 1e-14
    # covering radius, sampled: the geodesic ball that holds 1/1 024 of SO(3) has radius 15.1 degrees, so no grid of
    # 1 024 rotations covers with less; this one leaves no random rotation further than 25 degrees from a grid point
    rng = np.random.default_rng(0)
    r = rng.normal(size=(20000, 4))
    r /= np.linalg.norm(r, axis=1, keepdims=True)
    ang = np.degrees(2.0 * np.arccos(np.clip(np.abs(r @ q.T).max(1), -1.0, 1.0)))
    assert 15.1 < ang.max() < 25.0, ang.max()


def test_subsample_seeds_and_hypotheses():
    rng = np.random.default_rng(1)
    rows, cols = 120, 160
    frame = rng.uniform(0.1, 3.5, rows * cols).astype(np.float32)
    frame[rng.random(frame.shape) < 0.2] = np.nan
    assert tw.coarse_factor(640) == 4 and tw.coarse_factor(320) == 2 and tw.coarse_factor(160) == 1
    coarse, r, c = tw.subsample(frame, rows, cols, 2)
    assert (r, c) == (60, 80)
    assert coarse[3, 5] == frame.reshape(rows, cols)[6, 10] or (np.isnan(coarse[3, 5]) and np.isnan(frame.reshape(rows, cols)[6, 10]))
    s, n = tw.seeds(coarse, 4, 0.2, 3.0, 64)
    assert n > 64 and len(s) == -(-n // -(-n // 64)) and len(s) <= 64
    assert np.all((s[:, 2] >= 0.2) & (s[:, 2] <= 3.0))
    assert np.all(np.diff(s[:, 3]) > 0)     # row-major order
    K = tw.coarse_K(np.array([[570.3, 0, 79.5], [0, 570.3, 59.5], [0, 0, 1.0]]), 2)
    hp = tw.hypotheses(s, 8, K, 0.05)
    assert hp.shape == (len(s) * 8, 12)
    # the centre lies depth_offset behind the observed point, along the viewing ray
    p = s[0]
    x, y = (p[0] - K[0, 2]) / K[0, 0], (p[1] - K[1, 2]) / K[1, 1]
    surface = p[2] * np.array([x, y, 1.0])
    assert abs(np.linalg.norm(hp[0, 9:] - surface) - 0.05) < 1e-12
    assert abs(np.linalg.norm(hp[0, 9:]) - np.linalg.norm(surface) - 0.05) < 1e-12


def test_nms_and_selection():
    poses = np.zeros((5, 12))
    poses[:, [0, 4, 8]] = 1.0
    poses[:, 9:] = [[0, 0, 1], [0.01, 0, 1], [0.05, 0, 1], [0.05, 0, 1], [0.05, 0.001, 1]]
    from dbot_ros_amd.pose import rotvec_to_matrix
    poses[3, :9] = rotvec_to_matrix(np.array([0, 0, math.radians(45)])).ravel()   # same place, another orientation
    assert tw.nms(poses, 0.02, math.radians(30), 10) == [0, 2, 3]
    assert tw.nms(poses, 0.02, math.radians(30), 2) == [0, 2]
    order = tw.select_order(np.array([1.0, np.nan, 3.0, 3.0, -np.inf]))
    assert list(order) == [2, 3, 0, 4]


def test_perturbation_formula():
    surv = np.zeros((2, 12))
    surv[:, [0, 4, 8]] = 1.0
    surv[:, 9:] = [[0, 0, 1], [0.1, 0, 1]]
    ch = tw.children(surv, 4, 0, 7, 0.01, math.radians(10))
    np.testing.assert_array_equal(ch[:, 0], surv)
    nz = tw.child_normals(7, 0, 1, 2)
    np.testing.assert_allclose(ch[1, 2, 9:], surv[1, 9:] + 0.01 * nz[3:], rtol=0, atol=1e-16)
    R = ch[1, 2, :9].reshape(3, 3)
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-15
    # the rotation angle is sigma_a * |n|
    ang = math.acos(max(-1.0, min(1.0, (np.trace(R) - 1.0) / 2.0)))
    assert abs(ang - math.radians(10) * np.linalg.norm(nz[:3])) < 1e-7
    assert tw.best_child(np.array([[1.0, 2.0, 2.0], [np.nan, np.nan, 0.5], [3.0, np.nan, 3.0]])).tolist() == [1, 2, 0]


def test_finder_kernels_do_not_spill():
    txt = open(os.path.join(ROOT, "dbot_ros_amd", "lib", "resource_usage.txt")).read()
    blocks = re.split(r"remark: Function Name: ", txt)[1:]
    seen = set()
    for b in blocks:
        name = b.split()[0]
        m = re.search(r"rbs_find_(\w+?)_kernel", name)
        if not m:
            continue
        seen.add(m.group(1))
        assert re.search(r"ScratchSize \[bytes/lane\]: 0\b", b), name
        assert re.search(r"SGPRs Spill: 0\b", b) and re.search(r"VGPRs Spill: 0\b", b), name
    assert seen == set(KERNELS), seen


def test_exports_and_parameter_checks_without_a_device():
    lib = _capi.load()
    for s in ("rbs_find_create", "rbs_find_run", "rbs_find_get_stage", "rbs_find_destroy"):
        assert s in _capi.EXPORTS and hasattr(lib, s)
    p = _capi.RbsFindParams()
    lib.rbs_find_default_params(C.byref(p))
    d = ObjectFinder.Parameters()
    for f in p._fields_:
        assert getattr(p, f[0]) == pytest.approx(getattr(d, f[0])), f[0]
    out = C.c_void_p()
    for field, bad, message in (("n_candidates", 2000, "find: n_candidates outside 1..1024"),
                                ("decay", 0.0, "find: decay outside (0, 1]"),
                                ("n_survivors", 100, "find: n_survivors outside 1..min(64, n_candidates)"),
                                ("batch", 0, "find: batch outside 1..2^20"),
                                ("seed_stride", 0, "find: seed_stride outside 1..4096"),
                                ("min_depth", -1.0, "find: need 0 < min_depth <= max_depth < inf"),
                                ("coarse_downsampling", 3, "find: coarse_downsampling must be 0, 1, 2 or 4")):
        q = _capi.RbsFindParams()
        lib.rbs_find_default_params(C.byref(q))
        setattr(q, field, bad)
        assert lib.rbs_find_create(None, C.byref(q), C.byref(out)) == _capi.RBS_ERR_INVALID_ARGUMENT
        assert lib.rbs_last_error(None).decode() == message, field
    assert lib.rbs_find_create(None, C.byref(p), C.byref(out)) == _capi.RBS_ERR_INVALID_ARGUMENT   # (no sensor)
    assert not out.value


def test_parameters_from_rosparam():
    p = ObjectFinder.Parameters.from_rosparam({"object_finder": {"n_rotations": 2048, "nms_angle_deg": 45, "min_score": 10}})
    assert p.n_rotations == 2048 and p.nms_angle == pytest.approx(math.radians(45)) and p.min_score == 10.0
    assert ObjectFinder.Parameters.from_rosparam({}) == ObjectFinder.Parameters()
    with pytest.raises(ValueError):
        ObjectFinder.Parameters.from_rosparam({"object_finder": {"n_rotation": 1}})
