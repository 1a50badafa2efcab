"""The object finder's step 6b, the adaptive refinement, through the release library (rbs_find_set_refinement,
rbs_find_get_covariance, rbs_find_get_perturbations; ObjectFinder.Refinement): off it changes no bit of a find; on, every round
is the numpy twin (tests/find_refine_twin.py) from the device's own previous round -- the elite, the covariances and the
factors the next children are drawn through, exactly; it is deterministic whatever `batch`; a find with it leaves the sensor
and a tracker over it alone; the C++ mirror drives it; and the accuracy bar of tests/test_gpu_finder.py measured with it on."""
import math
import os
import subprocess

import numpy as np
import pytest

import find_refine_twin as rt
import find_twin as tw
import test_find_object_cpu as drv
from dbot_ros_amd import RbSensor, RbSensorBuilder, _capi, synth
from dbot_ros_amd.finder import ObjectFinder
from dbot_ros_amd.sensor import RbSensorError
from find_fg_twin import SCENES
from test_gpu_finder import SMALL, TINY, _iou, _params, _reference_scores, _scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAGES = ("seeds", "coarse", "candidates", "survivors", "result")
FG, RF = ObjectFinder.Foreground, ObjectFinder.Refinement
WIDE = dict(sigma_angle=math.radians(25.0), sigma_translation=0.015)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


def _all_stages(fnd, rounds):
    out = [fnd.stage(s) for s in STAGES] + [fnd.stage("children", r) for r in range(rounds)]
    return [a for st in out for a in st]


def _assert_same_bits(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.shape == y.shape and np.array_equal(_bits(x), _bits(y))


def _covariances(fnd, rounds):
    return [fnd.covariance(r) for r in range(rounds + 1)] + [fnd.perturbations(r) for r in range(rounds)]


def test_off_and_on_then_off_are_a_finder_never_configured(gpu_lib):
    om, cam, P, sensor, truth, frame = _scene("m1", 320, 240, seed=3)
    p = _params(**SMALL, seed=11)
    with sensor:
        with ObjectFinder(sensor, om, p) as plain:
            want_r = plain.find(frame)
            want = _all_stages(plain, p.rounds)
            with pytest.raises(RbSensorError) as e:                      # no find with the stage: no covariances
                plain.covariance(0)
            assert e.value.code == _capi.RBS_ERR_INVALID_ARGUMENT
        with ObjectFinder(sensor, om, p, refinement=RF(enabled=False)) as off:
            assert off.refinement is None
            r = off.find(frame)
            _assert_same_bits(_all_stages(off, p.rounds), want)
            _assert_same_bits([r.poses, r.scores], [want_r.poses, want_r.scores])
        with ObjectFinder(sensor, om, p) as toggled:
            toggled.set_refinement(RF())
            on = toggled.find(frame)
            assert on.found and len(toggled.covariance(p.rounds)) == len(on.poses)
            # round 0 draws through diag(sqrt(sigma^2)): step 6's children to rounding; from round 1 on it is another search
            k0, k1 = toggled.stage("children", 0)[0], toggled.stage("children", 1)[0]
            w0, w1 = want[4 * len(STAGES)], want[4 * len(STAGES) + 4]
            np.testing.assert_allclose(k0, w0, rtol=0, atol=1e-14)
            assert np.abs(k1 - w1).max() > 1e-6
            _assert_same_bits(_all_stages(toggled, 0)[: 4 * len(STAGES) - 4], want[: 4 * len(STAGES) - 4])   # steps 1-5 are the same
            toggled.set_refinement(None)
            r = toggled.find(frame)
            _assert_same_bits(_all_stages(toggled, p.rounds), want)
            _assert_same_bits([r.poses, r.scores], [want_r.poses, want_r.scores])
            with pytest.raises(RbSensorError):
                toggled.covariance(0)
            toggled.set_refinement(RF())
            toggled.set_refinement(RF(enabled=False))                     # enabled = 0 is off too
            toggled.find(frame)
            _assert_same_bits(_all_stages(toggled, p.rounds), want)


def test_bad_settings_are_refused_and_the_previous_one_stays(gpu_lib):
    om, cam, P, sensor, truth, frame = _scene("m1_l2", 160, 120, seed=4)
    p = _params(**TINY)
    nan, inf = float("nan"), float("inf")
    bad = (RF(elite=0), RF(elite=65), RF(elite=-1), RF(elite=p.children + 1), RF(mix=-0.1), RF(mix=1.5), RF(mix=nan), RF(shrink=0.0),
           RF(shrink=1.01), RF(shrink=nan), RF(jitter=-1e-12), RF(jitter=inf), RF(jitter=nan))
    first = RF(elite=min(4, p.children), mix=0.75, shrink=0.9, jitter=1e-9)
    with sensor:
        with ObjectFinder(sensor, om, p) as plain:
            off = plain.find(frame)
        with ObjectFinder(sensor, om, p, refinement=first) as fnd:
            on = fnd.find(frame)
            on_state = _covariances(fnd, p.rounds)
            for g in bad:
                with pytest.raises(RbSensorError) as e:
                    fnd.set_refinement(g)
                assert e.value.code == _capi.RBS_ERR_INVALID_ARGUMENT, g
                assert fnd.refinement == first
            again = fnd.find(frame)                                        # still the setting of before
            _assert_same_bits([again.poses, again.scores] + _covariances(fnd, p.rounds), [on.poses, on.scores] + on_state)
            fnd.set_refinement(None)
            for g in bad[:3]:
                with pytest.raises(RbSensorError):
                    fnd.set_refinement(g)
            still_off = fnd.find(frame)                                    # ... and off stays off
            _assert_same_bits([still_off.poses, still_off.scores], [off.poses, off.scores])
            fnd.set_refinement(first)
            fnd.find(frame)
            for bad_call in (lambda: fnd.covariance(p.rounds + 1), lambda: fnd.covariance(-1), lambda: fnd.perturbations(p.rounds)):
                with pytest.raises(RbSensorError) as e:                    # a round outside 0..rounds (0..rounds-1)
                    bad_call()
                assert e.value.code == _capi.RBS_ERR_INVALID_ARGUMENT
        with pytest.raises(RbSensorError) as e:
            ObjectFinder(sensor, om, p, refinement=bad[0])
        assert e.value.code == _capi.RBS_ERR_INVALID_ARGUMENT


def test_two_runs_and_any_batch_give_the_same_bits(gpu_lib):
    om, cam, P, sensor, truth, frame = _scene("m2", 320, 240, seed=7)
    with sensor:
        outs = []
        for batch in (4096, 4096, 65536, 2048):
            with ObjectFinder(sensor, om, _params(**dict(SMALL, batch=batch), **WIDE), foreground=FG(), refinement=RF()) as fnd:
                for _ in range(2):
                    r = fnd.find(frame)
                    outs.append([r.poses, r.scores] + _covariances(fnd, SMALL["rounds"]) +
                                [a for q in range(SMALL["rounds"]) for a in fnd.stage("children", q)[:2]])
        for o in outs[1:]:
            _assert_same_bits(o, outs[0])


@pytest.mark.parametrize("setting", [RF(), RF(elite=16, mix=1.0, shrink=0.9, jitter=0.0), RF(elite=1, mix=0.25)], ids=["default", "mix1", "elite1"])
def test_every_round_matches_the_twin(gpu_lib, setting):
    """As tests/test_gpu_finder.py::test_stages_match_the_twin does for step 6: each round from the device's own previous round.
    The covariances follow exactly from the device's perturbations and scores; the children follow from the covariances."""
    om, cam, P, sensor, truth, frame = _scene("m1", 320, 240, seed=3)
    p = _params(**SMALL, seed=11, **WIDE)
    g = setting
    with sensor, ObjectFinder(sensor, om, p, refinement=g) as fnd:
        res = fnd.find(frame)
        sp, _, _, _ = fnd.stage("survivors")
        S = len(sp)
        assert S > 1
        cur, prev = sp.copy(), None
        C = np.repeat(rt.initial_covariance(p.sigma_angle, p.sigma_translation)[None], S, 0)
        for r in range(p.rounds):
            got_c = fnd.covariance(r)
            assert got_c.shape == (S, 6, 6) and np.array_equal(_bits(got_c), _bits(C)), r          # the covariances entering round r
            L = np.stack([rt.factor(c, g.jitter) for c in C])
            kp, ks, _, _ = fnd.stage("children", r)
            kp, ks = kp.reshape(S, p.children, 12), ks.reshape(S, p.children)
            d = fnd.perturbations(r).reshape(S, p.children, 6)
            tp, td = rt.children(cur, L, p.children, r, p.seed)
            np.testing.assert_allclose(d, td, rtol=0, atol=1e-14)
            np.testing.assert_allclose(kp, tp, rtol=0, atol=1e-14)
            np.testing.assert_array_equal(kp[:, 0], cur)                   # child 0 is the survivor, bit for bit, and d = 0
            assert not d[:, 0].any()
            # the device's poses are its own perturbations' (the twin's rotation from the same d: to rounding)
            np.testing.assert_allclose(kp, rt.poses_from(cur, d), rtol=0, atol=1e-14)
            b = tw.best_child(ks)
            best = ks[np.arange(S), b]
            assert prev is None or np.all(best >= prev)
            prev, cur = best, kp[np.arange(S), b]
            C, _ = rt.update_all(C, ks, d, g.elite, g.mix, g.shrink, g.jitter)
        assert np.array_equal(_bits(fnd.covariance(p.rounds)), _bits(C))   # the final ones
        assert not np.array_equal(C[0], rt.initial_covariance(p.sigma_angle, p.sigma_translation))
        rp, rs, ri, _ = fnd.stage("result")
        o = tw.select_order(prev)
        np.testing.assert_array_equal(ri, o)
        np.testing.assert_array_equal(rp, cur[o])
        np.testing.assert_array_equal(rs, prev[o])
        np.testing.assert_array_equal(res.poses, rp)
        np.testing.assert_array_equal(res.scores, rs)
        # the scores are the sensor's own, as in step 6
        kp, ks, _, _ = fnd.stage("children", p.rounds - 1)
        pick = np.arange(0, len(kp), 3)
        np.testing.assert_array_equal(ks[pick], _reference_scores(om, cam.camera_matrix, cam.rows, cam.cols, P, frame, kp[pick]))


def test_rounds_zero_and_one_survivor(gpu_lib):
    om, cam, P, sensor, truth, frame = _scene("m1_l2", 160, 120, seed=4)
    with sensor:
        with ObjectFinder(sensor, om, _params(**dict(TINY, rounds=0)), refinement=RF()) as fnd, \
                ObjectFinder(sensor, om, _params(**dict(TINY, rounds=0))) as plain:
            r, w = fnd.find(frame), plain.find(frame)
            _assert_same_bits([r.poses, r.scores], [w.poses, w.scores])
            C0 = rt.initial_covariance(fnd.params.sigma_angle, fnd.params.sigma_translation)
            assert np.array_equal(fnd.covariance(0), np.repeat(C0[None], len(r.poses), 0))
        p = _params(**dict(TINY, n_survivors=1, children=1))               # one child: the survivor itself, C shrinks by 1 - mix
        with ObjectFinder(sensor, om, p, refinement=RF(elite=1, jitter=0.0)) as fnd:
            r = fnd.find(frame)
            assert len(r.poses) == 1 and np.array_equal(r.poses, fnd.stage("survivors")[0])
            C0 = rt.initial_covariance(p.sigma_angle, p.sigma_translation)
            for q in range(p.rounds + 1):
                assert np.array_equal(fnd.covariance(q)[0], C0 * 0.5 ** q)


def test_a_tracker_does_not_notice_a_refined_find(gpu_lib):
    from dbot_ros_amd.pose import matrix_to_rotvec
    from dbot_ros_amd.tracker import DeviceParticleTracker, ObjectTransitionBuilder, ParticleTrackerBuilder
    om, cam, P, probe, _, _ = _scene("m1", 320, 240, seed=1)
    rng = np.random.default_rng(4)
    truths = [synth.truth_pose(1, z=0.7, frame=k)[0] for k in range(8)]
    frames = []
    for tr in truths:
        d = probe.render_depth(tr)
        frames.append(synth.make_frame(np.where(np.isfinite(d), d, np.inf), cam.rows, cam.cols, rng))
    probe.close()

    def run(find_at=None, look_ahead=False, from_sensor=False):
        sensor = RbSensor(om, cam, RbSensorBuilder.Parameters(sample_count=200), max_particles=200)
        tr = DeviceParticleTracker(ObjectTransitionBuilder(ObjectTransitionBuilder.Parameters(
            0.002, 0.002, 0.002, 0.01, 0.01, 0.01, 0.8)).build(), sensor, om, ParticleTrackerBuilder.Parameters(evaluation_count=200),
            device_rng=True, seed=3)
        fnd = ObjectFinder(sensor, om, _params(**SMALL, **WIDE), foreground=FG(), refinement=RF())
        s0 = np.zeros(12)
        s0[:3] = truths[0][9:] - truths[0][:9].reshape(3, 3) @ om.centers[0]
        s0[3:6] = matrix_to_rotvec(truths[0][:9].reshape(3, 3))
        tr.initialize([s0])
        ests, found = [], None
        if look_ahead:
            tr.submit(frames[0])
            for k in range(1, len(frames)):
                tr.submit(frames[k])
                if find_at == k:
                    found = (fnd.find(None if from_sensor else frames[k]), fnd.covariance(SMALL["rounds"]))
                ests.append(tr.result())
            ests.append(tr.result())
        else:
            for k, fr in enumerate(frames):
                ests.append(tr.track(fr))
                if find_at == k:
                    found = (fnd.find(None if from_sensor else fr), fnd.covariance(SMALL["rounds"]))
        fnd.close()
        tr.close()
        sensor.close()
        return np.array(ests), found

    finds = []
    for la in (False, True):
        base, _ = run(look_ahead=la)
        for from_sensor in (False, True):
            got, (r, cov) = run(find_at=5, look_ahead=la, from_sensor=from_sensor)
            assert np.array_equal(_bits(got), _bits(base))
            assert r.found and len(cov) == len(r.poses)
            finds.append([r.poses, r.scores, cov])
    for f in finds[1:]:                                                    # the same frame: the same find, from a host frame or the sensor's
        _assert_same_bits(f, finds[0])


def test_the_node_passes_the_setting_through(tmp_path, gpu_lib):
    from dbot_ros_amd import node
    from test_node import _write
    tree = node.load_rosparams(*_write(tmp_path))
    K = synth.camera_matrix(640, 480)
    tree["object_finder"] = dict(TINY, refinement={"elite": 4, "mix": 0.75}, foreground={})
    finder, om, cam = node.build_object_finder(tree, K, str(tmp_path))
    try:
        assert finder.refinement == RF(elite=4, mix=0.75) and finder.foreground == FG() and finder.params.rounds == TINY["rounds"]
        frame = np.full((cam.rows, cam.cols), 1.0, dtype=np.float32)       # a plane with a block standing in front of it
        frame[cam.rows // 3: 2 * cam.rows // 3, cam.cols // 3: 2 * cam.cols // 3] = 0.7
        r = finder.find(frame)
        assert len(r.poses) > 0 and finder.covariance(TINY["rounds"]).shape == (len(r.poses), 6, 6)
    finally:
        finder.close()
        finder.sensor.close()
    tree["object_finder"] = dict(TINY)
    finder, _, _ = node.build_object_finder(tree, K, str(tmp_path))
    try:
        assert finder.refinement is None and finder.foreground is None
    finally:
        finder.close()
        finder.sensor.close()


def test_cpp_mirror_is_bit_identical_to_python(tmp_path, gpu_lib):
    om, cam, P, sensor, truth, frame = _scene("m1", 320, 240, seed=2)
    p = ObjectFinder.Parameters(max_seeds=64, n_rotations=256, n_candidates=256, n_survivors=8, rounds=3, children=32, batch=8192)
    with sensor, ObjectFinder(sensor, om, p, refinement=RF()) as fnd:
        want = fnd.find(frame)
        want_cov = fnd.covariance(p.rounds)
    exe = os.path.join(str(tmp_path), "find_refinement_check")
    lib_dir = os.path.dirname(_capi.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "find_refinement_check.cpp"), "-L" + lib_dir, "-lrbsensor_mi355x",
                           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"])
    inp, out = os.path.join(str(tmp_path), "in.bin"), os.path.join(str(tmp_path), "out.bin")
    drv.write_driver_input(inp, om.vertices[0], om.triangles[0], cam.camera_matrix, cam.cols, cam.rows, p, frame)
    r = subprocess.run([exe, inp, out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("OK"), (r.stdout, r.stderr)
    raw = open(out, "rb").read()
    found, n = np.frombuffer(raw[:8], dtype=np.int32)
    d = np.frombuffer(raw[8:], dtype=np.float64)
    assert bool(found) == want.found and n == len(want.poses) and len(d) == n * (12 + 1 + 12 + 36)
    _assert_same_bits([d[: 12 * n].reshape(n, 12), d[12 * n: 13 * n], d[25 * n:].reshape(n, 6, 6)], [want.poses, want.scores, want_cov])


# ---------------------------------------------------------------- the accuracy bar with the stage on
# The bar of tests/test_gpu_finder.py::test_accuracy_on_synthetic_scenes (translation < 1 cm, IoU >= 0.85, score >= 0.98 x the
# truth's) on its six scenes with the default foreground at seed_stride 4 and the default refinement from sigma (25 degrees,
# 1.5 cm).  ROUNDS is the smallest of {12, 16, 20, 24} at which the most scenes met the FULL bar on one MI355X: all six meet it
# at 16, 20 and 24; at 12 every pose is inside 1.9 mm at IoU >= 0.971 but only m1-1 and m3-1 have reached 0.98 of the truth's
# score.  MEASURED: (mesh, scene seed) -> rounds -> (|dt| mm, IoU, score / truth's); the rows at 12 are the CPU twin chain's
# (tests/test_find_refinement_cpu.py) to every printed digit.  So there is no expected failure here: the pose part and the
# score part are asserted on all six.
ROUNDS = 16
MEASURED = {
    ("m1", 1): {12: (1.89, 0.971, 0.9808), 16: (1.04, 0.981, 0.9924), 20: (0.31, 0.995, 0.9987), 24: (0.19, 0.996, 0.9997)},
    ("m1", 2): {12: (0.17, 0.983, 0.9793), 16: (0.82, 0.986, 0.9951), 20: (0.37, 0.990, 0.9987), 24: (0.38, 0.994, 1.0002)},
    ("m2", 1): {12: (1.43, 0.984, 0.9645), 16: (0.89, 0.993, 0.9880), 20: (0.17, 0.997, 0.9962), 24: (0.07, 0.998, 0.9987)},
    ("m2", 2): {12: (0.97, 0.974, 0.9681), 16: (0.38, 0.990, 0.9875), 20: (0.16, 0.995, 0.9963), 24: (0.25, 0.999, 0.9984)},
    ("m3", 1): {12: (0.48, 0.985, 0.9877), 16: (0.48, 0.985, 0.9877), 20: (0.14, 0.994, 0.9945), 24: (0.07, 0.997, 0.9970)},
    ("m3", 2): {12: (0.48, 0.984, 0.9757), 16: (0.39, 0.994, 0.9937), 20: (0.30, 0.997, 0.9973), 24: (0.07, 0.999, 0.9994)},
}


@pytest.mark.parametrize("mesh, seed", SCENES)
def test_accuracy_with_the_refinement_on(gpu_lib, mesh, seed):
    om, cam, P, sensor, truth, frame = _scene(mesh, 640, 480, seed=100 + seed)
    with sensor, ObjectFinder(sensor, om, _params(seed_stride=4, rounds=ROUNDS, **WIDE), foreground=FG(), refinement=RF()) as fnd:
        r = fnd.find(frame)
        ms = fnd.stage_ms()
        assert r.found
        best = r.poses[0]
        s_truth = _reference_scores(om, cam.camera_matrix, cam.rows, cam.cols, P, frame, truth[None])[0]
        dt = float(np.linalg.norm(best[9:] - truth[9:]))
        iou = _iou(sensor.render_depth(best), sensor.render_depth(truth))
        print(f"ACCURACY {mesh} seed {seed} rounds {ROUNDS}: |dt| {dt * 1e3:.2f} mm, IoU {iou:.3f}, score {r.scores[0]:.1f} vs truth "
              f"{s_truth:.1f} ({r.scores[0] / s_truth:.4f}; measured {MEASURED[(mesh, seed)][ROUNDS]}), find {ms[4]:.1f} ms "
              f"(stages {[round(x, 3) for x in ms[:4]]})")
        assert dt < 0.01 and iou >= 0.85, (dt, iou, r.scores[0], s_truth)                  # the pose part
        assert r.scores[0] >= s_truth - 0.02 * abs(s_truth), (dt, iou, r.scores[0], s_truth)   # ... and the score part: the full bar
