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


def _before(a, b):
    """rbs_find_topk_kernel's `before`: larger score first, NaN last, then smaller index."""
    (sa, ia), (sb, ib) = a, b
    na, nb = sa != sa, sb != sb
    if na != nb:
        return nb
    if not na and sa != sb:
        return sa > sb
    return ia < ib


def test_topk_is_a_sort_by_the_kernels_order():
    import functools
    rng = np.random.default_rng(2)
    values = np.array([np.nan, -np.inf, np.inf, -0.0, 0.0, 1.0, 1.0 + 2.0 ** -52, -3.5])
    for n in (1, 2, 5, 64, 300):
        for index in (None, rng.permutation(n).astype(np.int64) * 5 + (1 << 31)):
            s = rng.choice(values, n)
            items = list(zip(s.tolist(), (range(n) if index is None else index.tolist())))
            ref = sorted(items, key=functools.cmp_to_key(lambda a, b: -1 if _before(a, b) else 1 if _before(b, a) else 0))
            for k in (1, n, n + 3):
                ts, ti = tw.topk(s, index, k)
                want = ref[:k] + [(math.nan, tw.INT64_MAX)] * max(0, k - n)
                assert ti.tolist() == [i for _, i in want], (n, k)
                ws = np.array([v for v, _ in want])
                assert np.array_equal(np.isnan(ts), np.isnan(ws)) and np.array_equal(np.signbit(ts), np.signbit(ws))
                assert np.array_equal(ts[~np.isnan(ts)], ws[~np.isnan(ws)])
    # NaN items stay, in index order at the end; select_order drops them; the final sort keeps them
    s = np.array([1.0, np.nan, 3.0, 3.0, np.nan, -np.inf])
    assert tw.topk(s)[1].tolist() == [2, 3, 0, 5, 1, 4] and tw.result_order(s).tolist() == [2, 3, 0, 5, 1, 4]
    assert tw.select_order(s).tolist() == [2, 3, 0, 5]


def test_philox_reproduces_the_random123_known_answers():
    from test_filter_twin_cpu import KNOWN_ANSWERS, _words
    for ctr, key, out in KNOWN_ANSWERS:
        c, k = _words(ctr), _words(key)
        assert tw.philox(k[1] << 32 | k[0], c[3] << 32 | c[2], c[1] << 32 | c[0]) == _words(out)
    # the finder's counter: (round << 32 | k) above (j << 2 | pair); the array form draws the integer form's normals
    nz = tw.child_normals_array(0xC0FFEE1234ABCDEF, 63, 3, 70)
    for k, j in ((0, 1), (2, 69), (1, 33)):
        np.testing.assert_allclose(nz[k, j], tw.child_normals(0xC0FFEE1234ABCDEF, 63, k, j), rtol=0, atol=4e-15)
    assert not np.allclose(tw.child_normals(5, 1, 2, 3), tw.child_normals(5, 2, 1, 3))


def test_extended_precision_twin_against_the_binary64_one():
    """The extended evaluation (mpmath where installed, long double otherwise) and the binary64 one are the same formulas: they
    agree to the binary64 one's rounding, and the two extended back ends agree to long double's."""
    rng = np.random.default_rng(4)
    idx = np.array([0, 1, 63, 64, 127])
    for use_mp in (True, False):
        R = tw.sf_rotations_ext(128, idx, use_mpmath=use_mp)
        assert R.dtype == np.longdouble and np.abs(R - tw.sf_rotations(128)[idx]).max() < 2e-13
    assert np.abs(tw.sf_rotations_ext(128, idx) - tw.sf_rotations_ext(128, idx, use_mpmath=False)).max() < 1e-16
    # at 2^20 rotations the angles reach 4.7e6 rad: the binary64 path is 1e-9 off, not 1e-15
    big = np.array([0, (1 << 20) - 1])
    err = np.abs(tw.sf_rotations_ext(1 << 20, big) - tw.sf_rotations(1 << 20)[big]).max()
    assert err < 4e-9, err
    seeds = np.stack([rng.integers(0, 160, 9), rng.integers(0, 120, 9), rng.uniform(0.3, 2.0, 9), np.zeros(9)], -1).astype(np.float64)
    K = tw.coarse_K(np.array([[570.3, 0, 159.5], [0, 570.3, 119.5], [0, 0, 1.0]]), 2)
    h = np.array([0, 7, 8, 71])
    ext = tw.hypotheses_ext(seeds, 8, K, 0.05, h)
    # (the angles reach 33 rad at 8 rotations: three roundings of one are 1e-14 rad)
    assert np.abs(ext - tw.hypotheses(seeds, 8, K, 0.05, h)).max() < 5e-14
    assert np.abs(ext[:, 9:] - tw.hypotheses(seeds, 8, K, 0.05, h)[:, 9:]).max() < 1e-15
    surv = tw.hypotheses(seeds, 8, K, 0.05, h)
    ch = tw.children(surv, 5, 3, 77, 0.01, 0.2)
    for use_mp in (True, False):
        ext = tw.children_ext(surv, 5, 3, 77, 0.01, 0.2, use_mpmath=use_mp).reshape(4, 5, 12)
        assert np.abs(ext - ch).max() < 1e-14
        assert np.array_equal(ext[:, 0], surv.astype(np.longdouble))
    assert np.abs(tw.children_array(surv, 5, 3, 77, 0.01, 0.2) - ch).max() < 1e-14
    assert np.abs(tw.child_normals_ext(77, 3, 1, 2) - tw.child_normals(77, 3, 1, 2)).max() < 1e-14


def test_suppression_stops_at_a_nan_score_and_best_child_rules():
    poses = np.zeros((4, 12))
    poses[:, [0, 4, 8]] = 1.0
    poses[:, 9] = [0.0, 1.0, 2.0, 3.0]
    assert tw.nms(poses, 0.02, 0.5, 10) == [0, 1, 2, 3]
    assert tw.nms(poses, 0.02, 0.5, 10, np.array([3.0, 2.0, np.nan, 1.0])) == [0, 1]
    assert tw.nms(poses, 0.02, 0.5, 10, np.array([np.nan, 2.0, 1.0, 0.0])) == []
    nan, ninf = np.nan, -np.inf
    rows = np.array([[nan, nan, nan], [nan, ninf, ninf], [ninf, nan, 1.0], [ninf, ninf, ninf], [nan, 2.0, 2.0], [np.inf, nan, np.inf]])
    assert tw.best_child(rows).tolist() == [0, 1, 2, 0, 1, 0]


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
