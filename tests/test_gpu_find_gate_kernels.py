"""The finder's evidence kernel alone (rbs_findc_evidence_kernel, dbot_ros_amd/csrc/rbsensor_find_gate.hip) through the
rbs_test_findc_evidence probe of the TEST build: all ten counts and the class of every pose against the numpy twin
(tests/find_gate_twin.py, which composes assess_twin and contour_twin) on the one-body oracle's plane, and against
rbs_contour_poses on the same pose and frame -- exactly.  Poses: the assessor's (truth, shifted, every border and a corner,
off screen, behind the camera) and the contour rule's in-wall poses; scenes: m1 at 80 x 60 (one tile), 161 x 121 (an odd
width, several tiles at the borders) and 640 x 480 with the pose 11 cm from the camera (many tiles and halos); radius 1, 2
and 8; an all-NaN frame; launches of 1, 255, 256 and 257 poses with a sentinel-filled tail; the same bits on a second run.

The probe lives in librbsensor_mi355x_hooks.so only.  As tests/test_gpu_finder_kernels.py does, the first test re-runs this
file once in a child with RBS_LIB_PATH set to the hooks build, and every test reports its own outcome of that run."""
import os

import numpy as np
import pytest

import assess_scenes as asc
import contour_scenes as cs
import find_gate_probes as gp
import find_gate_twin as gt
from dbot_ros_amd import RbSensor, _capi
from find_gate_probes import TAIL, untouched

pytestmark = pytest.mark.gpu

HOOKS = gp.hooks_path(_capi.LIB_PATH)
IN_HOOKS_PROCESS = os.path.abspath(_capi.LIB_PATH) == os.path.abspath(HOOKS)
_child = {}
RADII = (1, 2, 8)
SCENES = {"m1_80": (80, 60), "m1_161": (161, 121), "m1_640": (640, 480)}
PARAMS = dict(gt.DEFAULTS)                     # stated, not the library's defaults


def _delegated(request):
    """True: this process has not loaded the hooks build -- the test's outcome is the one of the child run."""
    if IN_HOOKS_PROCESS:
        return False
    if not _child:
        assert os.path.exists(HOOKS), "build() makes librbsensor_mi355x_hooks.so"
        _child["outcome"], _child["out"] = gp.child_outcomes(__file__, HOOKS, 900)
    assert _child["outcome"].get(request.node.name) == "PASSED", _child["out"]
    return True


@pytest.fixture(scope="module")
def probe(gpu_lib):
    return gp.GateProbe(HOOKS) if IN_HOOKS_PROCESS else None


@pytest.fixture(scope="module")
def scenes(gpu_lib):
    """name -> (Scene, sensor, pose names, poses [n, 12]): shared, read-only.  The child process only."""
    out = {}
    if not IN_HOOKS_PROCESS:
        yield out
        return
    for name, (cols, rows) in SCENES.items():
        s = asc.Scene(("m1",), cols, rows)
        poses = cs.poses(s)
        if name == "m1_640":                   # the size is there for the pose that spans many tiles and halos
            poses = {k: poses[k] for k in ("fills the image", "truth", "corner")}
        out[name] = (s, RbSensor(s.om, s.cam, s.P, max_particles=1), list(poses), np.stack([p.reshape(12) for p in poses.values()]))
    yield out
    for s, sensor, *_ in out.values():
        sensor.close()
        s.close()


def twin(s, pose, frame, **params):
    return gt.evidence(s.planes(pose)[0], frame, s.rows, s.cols, s.ms, s.sf, **dict(PARAMS, **params))


@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("name", list(SCENES))
def test_counts_and_class_equal_the_twin_and_rbs_contour_poses(request, probe, scenes, name, radius):
    if _delegated(request):
        return
    from dbot_ros_amd.assess import PoseAssessor
    s, sensor, names, stack = scenes[name]
    params = dict(PARAMS, radius=radius)
    rec, cls = probe.evidence(sensor, params, s.frame, stack)
    assert untouched(rec[len(names):]) and untouched(cls[len(names):])
    ap = PoseAssessor.Parameters(**{k: params[k] for k in gt.ASSESS_KEYS})
    cp = PoseAssessor.ContourParameters(**{k: params[k] for k in gt.CONTOUR_KEYS})
    lib = PoseAssessor(sensor, ap, cp).assess(stack[:, None, :], s.frame)
    classes = set()
    for k, pn in enumerate(names):
        want, wc = twin(s, stack[k], s.frame, radius=radius)
        print(name, "r", radius, pn, "device", rec[k].tolist(), int(cls[k]), "twin", want.tolist(), wc)
        assert np.array_equal(rec[k], want) and cls[k] == wc, (name, radius, pn)
        assert np.array_equal(rec[k, :5], lib.counts[k, 0]) and np.array_equal(rec[k, 5:], lib.contour_counts[k, 0]), (name, radius, pn)
        assert cls[k] == (0 if lib.confirmed_mask()[k] else 1), (name, radius, pn)
        classes.add(int(cls[k]))
    for pn in ("off screen", "behind the camera"):
        if pn in names:
            assert not rec[names.index(pn)].any() and cls[names.index(pn)] == 1, pn
    assert rec[names.index("truth"), 0] > 0 and rec[names.index("truth"), 5] > 0
    if name != "m1_640":
        assert classes == {0, 1}, "the poses take both classes"
    if "fills the image" in names and name == "m1_640":
        k = names.index("fills the image")
        tiles = -(-s.cols // (64 - 2 * radius)) * -(-s.rows // (64 - 2 * radius))
        assert rec[k, 0] > 64 * 64 * 4 and tiles > 50, "the pose spans many tiles"
    # the same bits on a second run
    rec2, cls2 = probe.evidence(sensor, params, s.frame, stack)
    assert np.array_equal(rec, rec2) and np.array_equal(cls, cls2)


@pytest.mark.parametrize("name", ["m1_80", "m1_161"])
def test_an_all_nan_frame_leaves_rendered_and_rim_alone(request, probe, scenes, name):
    if _delegated(request):
        return
    s, sensor, names, stack = scenes[name]
    nan = np.full(s.rows * s.cols, np.nan, dtype=np.float32)
    rec, cls = probe.evidence(sensor, PARAMS, nan, stack)
    ref, _ = probe.evidence(sensor, PARAMS, s.frame, stack)
    for k, pn in enumerate(names):
        want, wc = twin(s, stack[k], nan)
        assert np.array_equal(rec[k], want) and cls[k] == wc == 1, pn
    n = len(names)
    assert np.array_equal(rec[:n, 0], ref[:n, 0]) and np.array_equal(rec[:n, 5], ref[:n, 5])
    assert not rec[:n, 1:5].any() and not rec[:n, 6:].any()


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_a_launch_of_n_poses_writes_n_records_and_nothing_behind_them(request, probe, scenes, n):
    if _delegated(request):
        return
    s, sensor, names, stack = scenes["m1_80"]
    one, one_cls = probe.evidence(sensor, PARAMS, s.frame, stack)
    pick = (np.arange(n) * 7 + 3) % len(names)
    rec, cls = probe.evidence(sensor, PARAMS, s.frame, stack[pick])
    assert rec.shape == (n + TAIL, 10) and untouched(rec[n:]) and untouched(cls[n:])
    assert np.array_equal(rec[:n], one[pick]) and np.array_equal(cls[:n], one_cls[pick])


def test_each_threshold_of_the_class_is_taken_on_the_device(request, probe, scenes):
    """The class from the device's own counts at the five thresholds: equality and one count either side, through the
    thresholds themselves (a fraction a / b is exact where b is a power of two; elsewhere the twin takes the same binary64
    comparison)."""
    if _delegated(request):
        return
    s, sensor, names, stack = scenes["m1_80"]
    k = names.index("truth")
    base, _ = probe.evidence(sensor, PARAMS, s.frame, stack[k:k + 1])
    c = base[0]
    rendered, support, behind, rim, valid, beyond = (int(c[i]) for i in (0, 2, 4, 5, 6, 9))
    u = support + behind
    cases = [dict(min_pixels=rendered), dict(min_pixels=rendered + 1), dict(min_rim_pixels=rim), dict(min_rim_pixels=rim + 1)]
    for key, num, den in (("min_visible_fraction", u, rendered), ("min_support_fraction", support, u), ("min_valid_fraction", valid, rim),
                          ("min_contour_fraction", beyond, valid)):
        f = num / den
        cases += [{key: f}, {key: float(np.nextafter(f, 2.0))}, {key: float(np.nextafter(f, -1.0))}]
    seen = set()
    for params in cases:
        p = dict(PARAMS, **{k_: min(v, 1.0) if isinstance(v, float) else v for k_, v in params.items()})
        rec, cls = probe.evidence(sensor, p, s.frame, stack[k:k + 1])
        assert np.array_equal(rec[0], c)
        assert cls[0] == gt.class_of(c, **p), params
        seen.add(int(cls[0]))
    assert seen == {0, 1}


def test_the_probe_refuses_bad_arguments(request, probe, scenes):
    if _delegated(request):
        return
    import ctypes as C
    s, sensor, names, stack = scenes["m1_80"]
    g = gp.c_gate(PARAMS)
    rec, cls = gp.sentinel((4, 10), np.int32), gp.sentinel(4, np.int32)
    frame, poses = np.ascontiguousarray(s.frame), np.ascontiguousarray(stack[:1])
    h, p = C.c_void_p(sensor._h.value), gp._p
    call = probe.lib.rbs_test_findc_evidence
    bad = gp.RBS_ERR_INVALID_ARGUMENT
    assert call(None, C.byref(g), p(frame), p(poses), C.c_int32(1), p(rec), p(cls), C.c_int64(0)) == bad
    assert call(h, None, p(frame), p(poses), C.c_int32(1), p(rec), p(cls), C.c_int64(0)) == bad
    assert call(h, C.byref(g), None, p(poses), C.c_int32(1), p(rec), p(cls), C.c_int64(0)) == bad
    assert call(h, C.byref(g), p(frame), p(poses), C.c_int32(-1), p(rec), p(cls), C.c_int64(0)) == bad
    assert call(h, C.byref(g), p(frame), p(poses), C.c_int32(1), p(rec), p(cls), C.c_int64(-1)) == bad
    g9 = gp.c_gate(dict(PARAMS, radius=9))
    assert call(h, C.byref(g9), p(frame), p(poses), C.c_int32(1), p(rec), p(cls), C.c_int64(0)) == bad
    assert call(h, C.byref(g), p(frame), p(poses), C.c_int32(0), p(rec), p(cls), C.c_int64(0)) == gp.RBS_OK
    assert untouched(rec) and untouched(cls)
