"""The object finder's step 1b, the foreground, without a device: the numpy twin (tests/find_fg_twin.py) on the six synthetic
scenes of the accuracy bar (it must take the background plane away and leave the object), the frames without a plane, the
parameters' round trip through rosparam, and what the libraries export."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import find_fg_twin as fg
import find_twin as tw
import oracle_binding as ob
import scenarios as sc
from dbot_ros_amd import _capi, synth
from dbot_ros_amd.finder import ObjectFinder
from dbot_ros_amd.pose import quat_to_matrix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = fg.SCENES
DMIN, DMAX = ObjectFinder.Parameters().min_depth, ObjectFinder.Parameters().max_depth


def scene_truth(cols, rows, seed):
    """The pose of tests/test_gpu_finder.py's _scene for this seed (the same draws), and the generator after them."""
    rng = np.random.default_rng(seed)
    K = synth.camera_matrix(cols, rows)
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    rot = quat_to_matrix(q)
    z = rng.uniform(0.55, 0.9)
    u, v = rng.uniform(0.3, 0.7) * cols, rng.uniform(0.3, 0.7) * rows
    t = np.array([(u - K[0, 2]) / K[0, 0] * z, (v - K[1, 2]) / K[1, 1] * z, z])
    return np.concatenate([np.asarray(rot).ravel(), t]), rng


@pytest.mark.parametrize("mesh, seed", SCENES)
def test_twin_removes_the_plane_and_keeps_the_object(mesh, seed):
    cols, rows, f = 640, 480, 4
    om, cam, P = sc.make_scene((mesh,), cols, rows, max_particles=1)
    truth, rng = scene_truth(cols, rows, 100 + seed)
    depth = ob.Oracle(om, cam, P, max_particles=1, mode=ob.EAGER).render_depth(truth)       # the oracle's CPU renderer
    depth = np.where(np.isfinite(depth), depth, np.inf)
    frame = synth.make_frame(depth, rows, cols, rng)
    coarse, cr, cc = tw.subsample(frame, rows, cols, f)
    labels = fg.scene_labels(depth, rows, cols)[: cr * f: f, : cc * f: f]
    rec, seed_frame = fg.foreground(coarse, cr, cc, DMIN, DMAX, P.kinect.model_sigma, P.kinect.sigma_factor, ObjectFinder.Parameters().seed)
    kp, ko = fg.check_caps(rec, seed_frame, coarse, labels, DMIN, DMAX)
    print(f"{mesh} seed {seed}: plane {rec[1:4]}, count {rec[4]:.0f} of {rec[5]:.0f}, masked {rec[7]:.0f}; kept {kp:.4%} of the plane, "
          f"{ko:.2%} of the object")
    # kept pixels keep their bits; the record's count of masked pixels is the valid pixels that went
    same = fg.valid(seed_frame, DMIN, DMAX).reshape(coarse.shape)
    assert np.array_equal(seed_frame[same].view(np.uint32), coarse[same].view(np.uint32))
    assert rec[7] == fg.valid(coarse, DMIN, DMAX).sum() - same.sum() > 0


def test_frames_without_a_plane_pass_through():
    rows, cols = 30, 40
    nan = np.full((rows, cols), np.nan, dtype=np.float32)
    two = nan.copy()
    two[3, 4], two[20, 31] = 0.7, 1.1
    junk = nan.copy()
    junk[0, :3] = [np.inf, -np.inf, 0.0]
    junk[5, 5], junk[6, 9], junk[9, 6] = 0.1, 3.5, -1.0              # outside [min_depth, max_depth]
    for frame, n_valid in ((nan, 0), (two, 2), (junk, 0)):
        rec, out = fg.foreground(frame, rows, cols, DMIN, DMAX, 0.003, 0.0014247, 5)
        assert rec.tolist() == [0.0, 0.0, 0.0, 0.0, -1.0, n_valid, 0.0, 0.0]
        assert np.array_equal(out.view(np.uint32), frame.view(np.uint32))
    # three valid pixels in a line: every trial is void too
    line = nan.copy()
    line[2, 2], line[4, 4], line[6, 6] = 0.5, 0.6, 0.7
    rec, out = fg.foreground(line, rows, cols, DMIN, DMAX, 0.003, 0.0014247, 5, plane_trials=4096)
    assert rec[0] == 0.0 and rec[4] == -1 and np.array_equal(out.view(np.uint32), line.view(np.uint32))


def test_a_frame_that_is_one_plane_gives_no_seeds():
    rows, cols = 120, 160
    cc, rr = np.meshgrid(np.arange(cols), np.arange(rows))
    z = 1.0 / (0.7 + 0.0004 * cc - 0.0007 * rr)                       # a plane in inverse depth, 0.5 .. 1.5 m
    frame = (z + np.random.default_rng(1).normal(size=z.shape) * (0.003 + 0.0014247 * z * z)).astype(np.float32)
    rec, out = fg.foreground(frame, rows, cols, DMIN, DMAX, 0.003, 0.0014247, 0)
    assert rec[0] == 1.0 and rec[4] >= 0.2 * rec[5] and rec[5] == rows * cols
    for stride in (1, 4):
        seeds, n = tw.seeds(out, stride, DMIN, DMAX, 1024)
        assert n == 0 and len(seeds) == 0
    assert rec[7] == rows * cols and np.isnan(out).all()


def test_ties_go_to_the_lowest_trial_and_the_acceptance_is_at_the_fraction():
    planes = np.array([[1.0, 0, 0, 0], [2.0, 0, 0, 0], [3.0, 0, 0, 1], [4.0, 0, 0, 0]])
    rec = fg.best(planes, np.array([5, 9, -1, 9, 36]), 0.25)
    assert rec.tolist() == [1.0, 2.0, 0.0, 0.0, 9.0, 36.0, 1.0, 0.0]               # 9 >= 0.25 * 36, trial 1 before trial 3
    assert fg.best(planes, np.array([5, 9, -1, 9, 37]), 0.25)[0] == 0.0             # 9 < 9.25
    assert fg.best(planes, np.array([2, 2, -1, 1, 4]), 0.25).tolist() == [0.0, 1.0, 0.0, 0.0, 2.0, 4.0, 0.0, 0.0]   # count < 3
    # the draws: word k of Philox (key, (t, 0, 0, 0xFFFFFFFF)) scaled to the pixels
    w = tw.philox(7, 0xFFFFFFFF << 32, 3)
    assert fg.trial_pixels(7, 3, 19200) == [(w[k] * 19200) >> 32 for k in range(3)] and max(fg.trial_pixels(7, 3, 19200)) < 19200
    assert fg.trial_pixels(7, 3, 1) == [0, 0, 0]


def test_foreground_from_rosparam_round_trip():
    F, Pm = ObjectFinder.Foreground, ObjectFinder.Parameters
    assert Pm.from_rosparam({}).foreground is None and Pm().foreground is None
    p = Pm.from_rosparam({"object_finder": {"seed_stride": 1, "foreground": {}}})
    assert p.foreground == F() and p.seed_stride == 1
    p = Pm.from_rosparam({"object_finder": {"foreground": {"plane_trials": 512, "mask_sigmas": 4, "enabled": 0, "ransac_sigmas": 2.5,
                                                              "min_inlier_fraction": 0.3}}})
    assert p.foreground == F(enabled=False, plane_trials=512, ransac_sigmas=2.5, mask_sigmas=4.0, min_inlier_fraction=0.3)
    assert isinstance(p.foreground.plane_trials, int) and isinstance(p.foreground.mask_sigmas, float)
    g = p.foreground.c_params()
    assert (g.enabled, g.plane_trials, g.ransac_sigmas, g.mask_sigmas, g.min_inlier_fraction) == (0, 512, 2.5, 4.0, 0.3)
    with pytest.raises(ValueError, match="object_finder/foreground/trials"):
        Pm.from_rosparam({"object_finder": {"foreground": {"trials": 5}}})
    with pytest.raises(ValueError):
        Pm.from_rosparam({"object_finder": {"foregrounds": {}}})
    # the C parameters never carry the Python-side setting
    assert [f[0] for f in _capi.RbsFindParams._fields_] == [f for f in Pm.__dataclass_fields__ if f != "foreground"]


def test_exports_defaults_and_checks_without_a_device():
    lib = _capi.load()
    for s in ("rbs_find_default_foreground", "rbs_find_set_foreground", "rbs_find_get_plane", "rbs_find_get_seed_frame"):
        assert s in _capi.EXPORTS and hasattr(lib, s)
    g = _capi.RbsFindForeground()
    lib.rbs_find_default_foreground(C.byref(g))
    d = ObjectFinder.Foreground()
    assert (g.enabled, g.plane_trials, g.ransac_sigmas, g.mask_sigmas, g.min_inlier_fraction) == \
        (1, d.plane_trials, d.ransac_sigmas, d.mask_sigmas, d.min_inlier_fraction) == (1, 256, 2.0, 5.0, 0.2)
    assert C.sizeof(_capi.RbsFindForeground) == 32
    out, n = (C.c_double * 8)(), C.c_int64()
    bad = _capi.RBS_ERR_INVALID_ARGUMENT
    assert lib.rbs_find_set_foreground(None, C.byref(g)) == bad and lib.rbs_find_get_plane(None, out) == bad
    assert lib.rbs_find_get_seed_frame(None, None, C.byref(n)) == bad


def test_foreground_kernels_do_not_spill_and_the_probes_stay_in_the_test_build():
    from find_fg_probes import FINDFG_SYMBOLS
    txt = open(os.path.join(ROOT, "dbot_ros_amd", "lib", "resource_usage.txt")).read()
    seen = set()
    for b in re.split(r"remark: Function Name: ", txt)[1:]:
        m = re.search(r"rbs_findfg_(\w+?)_kernel", b.split()[0])
        if not m:
            continue
        seen.add(m.group(1))
        assert re.search(r"ScratchSize \[bytes/lane\]: 0\b", b) and re.search(r"SGPRs Spill: 0\b", b) and re.search(r"VGPRs Spill: 0\b", b), b
    assert seen == {"trials", "count", "best", "mask"}, seen
    lib = os.path.join(ROOT, "dbot_ros_amd", "lib")
    release = open(os.path.join(lib, "librbsensor_mi355x.so"), "rb").read()
    test_build = open(os.path.join(lib, "librbsensor_mi355x_hooks.so"), "rb").read()
    assert b"rbs_test_" not in release
    for s in FINDFG_SYMBOLS:
        assert s.encode() + b"\0" in test_build, s
