"""The object finder's step 1b, the foreground, through the release library (rbs_find_set_foreground, rbs_find_get_plane,
rbs_find_get_seed_frame; ObjectFinder.Foreground): off it changes no bit of a find, on it is the numpy twin
(tests/find_fg_twin.py) exactly and the later stages are the existing twin's fed its seeds; it takes the background plane of the
six synthetic scenes away and leaves the object; a find with it leaves the sensor and a tracker over it alone; and the
accuracy bar of tests/test_gpu_finder.py measured with the stage on."""
import numpy as np
import pytest

import find_fg_twin as fg
import find_twin as tw
from dbot_ros_amd import RbSensor, RbSensorBuilder, _capi, synth
from dbot_ros_amd.finder import ObjectFinder
from dbot_ros_amd.sensor import RbSensorError
from find_fg_twin import SCENES
from test_gpu_finder import SMALL, TINY, _iou, _params, _reference_scores, _scene

pytestmark = pytest.mark.gpu

STAGES = ("seeds", "coarse", "candidates", "survivors", "result")
FG = ObjectFinder.Foreground


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


def _twin_foreground(frame, cam, P, p, g):
    """The twin's record, seeding frame and seeds for this frame: (rec, seed frame, seeds, valid seed pixels, coarse, f)."""
    f = tw.coarse_factor(cam.cols, p.coarse_downsampling)
    coarse, cr, cc = tw.subsample(frame, cam.rows, cam.cols, f)
    rec, sf = fg.foreground(coarse, cr, cc, p.min_depth, p.max_depth, P.kinect.model_sigma, P.kinect.sigma_factor, p.seed, g.plane_trials,
                            g.ransac_sigmas, g.mask_sigmas, g.min_inlier_fraction)
    tseeds, nvalid = tw.seeds(sf, p.seed_stride, p.min_depth, p.max_depth, p.max_seeds)
    return rec, sf, tseeds, nvalid, coarse, f


def _assert_plane_and_seed_frame(fnd, rec, sf):
    pl = fnd.plane()
    got = np.array([float(pl.accepted), pl.a, pl.b, pl.c, pl.count, pl.n_valid, pl.trial, pl.masked])
    assert np.array_equal(_bits(got), _bits(rec)), (got, rec)
    out = fnd.seed_frame()
    assert out.shape == sf.shape and out.dtype == np.float32 and np.array_equal(_bits(out), _bits(sf))


def test_off_and_on_then_off_are_a_finder_never_configured(gpu_lib):
    om, cam, P, sensor, truth, frame = _scene("m1", 320, 240, seed=3)
    p = _params(**SMALL, seed=11)
    with sensor:
        with ObjectFinder(sensor, om, p) as plain:
            want_r = plain.find(frame)
            want = _all_stages(plain, p.rounds)
            want_ms = plain.stage_ms()
            assert plain.plane() == (False, 0.0, 0.0, 0.0, 0, 0, 0, 0)
            coarse, _, _ = tw.subsample(frame, cam.rows, cam.cols, 2)
            assert np.array_equal(_bits(plain.seed_frame()), _bits(coarse))          # the stage off: the coarse frame
        with ObjectFinder(sensor, om, p, foreground=FG(enabled=False)) as off:
            assert off.foreground is None
            r = off.find(frame)
            _assert_same_bits(_all_stages(off, p.rounds), want)
            _assert_same_bits([r.poses, r.scores], [want_r.poses, want_r.scores])
        with ObjectFinder(sensor, om, p) as toggled:
            toggled.set_foreground(FG())
            on = toggled.find(frame)
            assert toggled.plane().accepted and len(toggled.stage("seeds")[0]) != len(want[0])
            toggled.set_foreground(None)
            r = toggled.find(frame)
            _assert_same_bits(_all_stages(toggled, p.rounds), want)
            _assert_same_bits([r.poses, r.scores], [want_r.poses, want_r.scores])
            assert toggled.plane() == (False, 0.0, 0.0, 0.0, 0, 0, 0, 0) and on.found
            toggled.set_foreground(FG())
            toggled.set_foreground(FG(enabled=False))                       # enabled = 0 is off too
            toggled.find(frame)
            _assert_same_bits(_all_stages(toggled, p.rounds), want)
        assert len(want_ms) == 5


@pytest.mark.parametrize("stride, trials", [(4, 256), (1, 257), (3, 1)])
def test_stage_on_matches_the_twin_and_the_later_stages_follow_its_seeds(gpu_lib, stride, trials):
    om, cam, P, sensor, truth, frame = _scene("m1", 320, 240, seed=3)
    p = _params(**SMALL, seed=11, seed_stride=stride)
    g = FG(plane_trials=trials)
    with sensor, ObjectFinder(sensor, om, p, foreground=g) as fnd:
        res = fnd.find(frame)
        rec, sf, tseeds, nvalid, coarse, f = _twin_foreground(frame, cam, P, p, g)
        _assert_plane_and_seed_frame(fnd, rec, sf)
        if trials > 1:
            assert rec[0] == 1.0 and rec[7] > 0.5 * rec[5]
        seeds, _, _, info = fnd.stage("seeds")
        assert f == 2 and (info[0], info[1], info[2], info[4]) == (sf.shape[0], sf.shape[1], f, nvalid)      # info[4]: after masking
        np.testing.assert_array_equal(seeds, tseeds)
        assert len(tseeds) > 0 and (stride != 1 or nvalid > p.max_seeds)
        # from here on: tests/test_gpu_finder.py::test_stages_match_the_twin, fed these seeds
        Kc = tw.coarse_K(cam.camera_matrix, f)
        hp, hs, hi, _ = fnd.stage("coarse")
        assert len(hp) == len(tseeds) * p.n_rotations == info[3]
        np.testing.assert_allclose(hp, tw.hypotheses(tseeds, p.n_rotations, Kc, info[5]), rtol=0, atol=1e-15)
        # (scoring reads the WHOLE coarse frame, not the seeding frame)
        pick = np.unique(np.concatenate([np.arange(0, len(hp), 97), np.argsort(-np.nan_to_num(hs, nan=-np.inf))[:32]]))
        np.testing.assert_array_equal(hs[pick], _reference_scores(om, Kc, sf.shape[0], sf.shape[1], P, coarse, hp[pick]))
        cp, cs, ci, _ = fnd.stage("candidates")
        order = tw.select_order(hs)[: p.n_candidates]
        np.testing.assert_array_equal(ci, order)
        np.testing.assert_array_equal(cs, hs[order])
        np.testing.assert_array_equal(cp, hp[order])
        sp, ss, si, _ = fnd.stage("survivors")
        kept = tw.nms(cp, p.nms_translation, p.nms_angle, p.n_survivors)
        np.testing.assert_array_equal(si, ci[kept])
        np.testing.assert_array_equal(sp, cp[kept])
        S = len(sp)
        cur, prev = sp.copy(), None
        st, sa = p.sigma_translation, p.sigma_angle
        for r in range(p.rounds):
            kp, ks, _, _ = fnd.stage("children", r)
            kp, ks = kp.reshape(S, p.children, 12), ks.reshape(S, p.children)
            np.testing.assert_allclose(kp, tw.children(cur, p.children, r, p.seed, st, sa), rtol=0, atol=1e-14)
            np.testing.assert_array_equal(kp[:, 0], cur)
            b = tw.best_child(ks)
            best = ks[np.arange(S), b]
            assert prev is None or np.all(best >= prev)
            prev, cur = best, kp[np.arange(S), b]
            st, sa = st * p.decay, sa * p.decay
        rp, rs, ri, _ = fnd.stage("result")
        o = tw.select_order(prev)
        np.testing.assert_array_equal(ri, o)
        np.testing.assert_array_equal(rp, cur[o])
        np.testing.assert_array_equal(rs, prev[o])
        np.testing.assert_array_equal(res.poses, rp)
        np.testing.assert_array_equal(res.scores, rs)


@pytest.mark.parametrize("mesh, seed", SCENES)
def test_the_plane_goes_and_the_object_stays_on_the_six_scenes(gpu_lib, mesh, seed):
    om, cam, P, sensor, truth, frame = _scene(mesh, 640, 480, seed=100 + seed)
    p = _params(**SMALL)
    with sensor, ObjectFinder(sensor, om, p, foreground=FG()) as fnd:
        fnd.find(frame)
        depth = sensor.render_depth(truth)
        rec, sf, tseeds, nvalid, coarse, f = _twin_foreground(frame, cam, P, p, FG())
        _assert_plane_and_seed_frame(fnd, rec, sf)
        labels = fg.scene_labels(depth, cam.rows, cam.cols)[: sf.shape[0] * f: f, : sf.shape[1] * f: f]
        kp, ko = fg.check_caps(rec, fnd.seed_frame(), coarse, labels, p.min_depth, p.max_depth)
        print(f"{mesh} seed {seed}: kept {kp:.4%} of the plane's pixels, {ko:.2%} of the object's; plane {fnd.plane()}")


def test_frames_without_a_plane_pass_through(gpu_lib):
    om, cam, P, sensor, truth, frame = _scene("m1_l2", 160, 120, seed=4)
    p = _params(**TINY)
    nan = np.full(cam.rows * cam.cols, np.nan, dtype=np.float32)
    two = nan.copy()
    two[[8 * cam.cols + 12, 60 * cam.cols + 80]] = 0.7, 0.8            # two valid pixels, both on the seed grid
    with sensor, ObjectFinder(sensor, om, p, foreground=FG()) as fnd, ObjectFinder(sensor, om, p) as plain:
        for empty, n_valid in ((nan, 0), (two, 2)):
            r, w = fnd.find(empty), plain.find(empty)
            assert fnd.plane() == (False, 0.0, 0.0, 0.0, -1, n_valid, 0, 0)
            assert np.array_equal(_bits(fnd.seed_frame()), _bits(empty.reshape(cam.rows, cam.cols)))
            _assert_same_bits(_all_stages(fnd, p.rounds) if n_valid else [], _all_stages(plain, p.rounds) if n_valid else [])
            _assert_same_bits([r.poses, r.scores], [w.poses, w.scores])
            assert r.found == w.found == bool(n_valid) and fnd.stage("seeds")[3][4] == n_valid
        assert fnd.find(frame).found and fnd.plane().accepted            # ... and then a good frame


def test_two_runs_and_any_batch_give_the_same_bits(gpu_lib):
    om, cam, P, sensor, truth, frame = _scene("m2", 320, 240, seed=7)
    with sensor:
        outs = []
        for batch in (4096, 4096, 65536, 2048):
            with ObjectFinder(sensor, om, _params(**dict(SMALL, batch=batch)), foreground=FG()) as fnd:
                for _ in range(2):
                    r = fnd.find(frame)
                    hp, hs, _, _ = fnd.stage("coarse")
                    outs.append([r.poses, r.scores, hs, fnd.stage("seeds")[0], fnd.seed_frame(), np.array(fnd.plane(), dtype=np.float64)])
        assert outs[0][5][0] == 1.0
        for o in outs[1:]:
            _assert_same_bits(o, outs[0])


def test_a_find_on_the_sensors_own_observation(gpu_lib):
    om, cam, P, sensor, truth, frame = _scene("m1_l2", 160, 120, seed=4)
    with sensor, ObjectFinder(sensor, om, _params(**TINY), foreground=FG()) as fnd:
        want = fnd.find(frame)
        plane, sf = fnd.plane(), fnd.seed_frame()
        sensor.set_observation(np.asarray(frame, dtype=np.float32).ravel())
        got = fnd.find(None)
        _assert_same_bits([got.poses, got.scores, fnd.seed_frame()], [want.poses, want.scores, sf])
        assert got.found == want.found and fnd.plane() == plane and plane.accepted


def test_a_tracker_does_not_notice_a_foreground_find(gpu_lib):
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
        fnd = ObjectFinder(sensor, om, _params(**SMALL), foreground=FG())
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
                    found = (fnd.find(None if from_sensor else frames[k]), fnd.plane())
                ests.append(tr.result())
            ests.append(tr.result())
        else:
            for k, fr in enumerate(frames):
                ests.append(tr.track(fr))
                if find_at == k:
                    found = (fnd.find(None if from_sensor else fr), fnd.plane())
        fnd.close()
        tr.close()
        sensor.close()
        return np.array(ests), found

    for la in (False, True):
        base, _ = run(look_ahead=la)
        for from_sensor in (False, True):
            got, (r, plane) = run(find_at=5, look_ahead=la, from_sensor=from_sensor)
            assert np.array_equal(_bits(got), _bits(base))
            assert r.found and plane.accepted


def test_bad_settings_are_refused_and_the_previous_one_stays(gpu_lib):
    om, cam, P, sensor, truth, frame = _scene("m1_l2", 160, 120, seed=4)
    p = _params(**TINY)
    bad = (FG(plane_trials=0), FG(plane_trials=4097), FG(plane_trials=-3), FG(ransac_sigmas=-1.0), FG(ransac_sigmas=float("nan")),
           FG(mask_sigmas=float("inf")), FG(mask_sigmas=-0.5), FG(min_inlier_fraction=1.5), FG(min_inlier_fraction=-0.1),
           FG(min_inlier_fraction=float("nan")))
    with sensor:
        with ObjectFinder(sensor, om, p) as plain:
            off = plain.find(frame)
            off_seeds = plain.stage("seeds")[0]
        with ObjectFinder(sensor, om, p, foreground=FG(plane_trials=64, mask_sigmas=4.0)) as fnd:
            on = fnd.find(frame)
            on_state = (fnd.plane(), fnd.seed_frame(), fnd.stage("seeds")[0])
            assert on_state[0].accepted and len(on_state[2]) != len(off_seeds)
            for g in bad:
                with pytest.raises(RbSensorError) as e:
                    fnd.set_foreground(g)
                assert e.value.code == _capi.RBS_ERR_INVALID_ARGUMENT, g
                assert fnd.foreground == FG(plane_trials=64, mask_sigmas=4.0)
            again = fnd.find(frame)                                        # still the setting of before
            assert fnd.plane() == on_state[0]
            _assert_same_bits([again.poses, again.scores, fnd.seed_frame(), fnd.stage("seeds")[0]], [on.poses, on.scores, on_state[1], on_state[2]])
            fnd.set_foreground(None)
            for g in bad[:3]:
                with pytest.raises(RbSensorError):
                    fnd.set_foreground(g)
            still_off = fnd.find(frame)                                    # ... and off stays off
            _assert_same_bits([still_off.poses, still_off.scores, fnd.stage("seeds")[0]], [off.poses, off.scores, off_seeds])
        with pytest.raises(RbSensorError) as e:
            ObjectFinder(sensor, om, p, foreground=bad[0])
        assert e.value.code == _capi.RBS_ERR_INVALID_ARGUMENT


# ---------------------------------------------------------------- the accuracy bar with the stage on: a measurement
# The bar of tests/test_gpu_finder.py::test_accuracy_on_synthetic_scenes (translation < 1 cm, IoU >= 0.85, score >= 0.98 x the
# truth's) on its six scenes with the header's default search and the default foreground, at seed_stride 4 and 1.
# MEASURED: (mesh, scene seed, seed_stride) -> (|dt| mm, IoU, score, truth's score, nearest coarse candidate mm, seeds on the
# object / on the occluder), on one MI355X (the last three from tools/find_object_timing.py --foreground).  Six of the twelve
# meet the bar (without the stage: none) and are plain assertions.  NOT_MET are strict expected failures, with the cause the
# timing tool shows:
#   m1-1, both strides   the pose is within 0.5 mm and IoU 0.96, but the score stays 4-5 % under the truth's (the bar allows 2 %)
#   m1-2, stride 4       6 seeds on the object: 1.6 mm, IoU 0.93, score 5.7 % under; stride 1 (126 seeds) meets the bar
#   m2-1, stride 4       as without the stage (12 mm, IoU 0.70): the nearest candidate is 13 mm and 171 degrees off, a flipped
#                        fit the refinement does not leave; stride 1 (251 seeds) meets the bar
#   m3-1, both strides   109 mm off at half the truth's score; the nearest candidate is 25 mm (stride 4) and 40 mm (stride 1)
#                        away, so the object's own fits are not among the candidates: with the plane gone, as many seeds sit
#                        on the occluder (220) as on the object (229); that the occluder's fits take the top-k is the likely reading
#                        (the tool does not say where each candidate lies).
#                        A second plane / clustering is the next step.
MEASURED = {
    ("m1", 1, 4): (0.50, 0.963, 15177.7, 15925.5, 9.05, 14, 9), ("m1", 1, 1): (0.27, 0.964, 15298.7, 15925.5, 3.34, 215, 176),
    ("m1", 2, 4): (1.57, 0.931, 8498.1, 9010.7, 11.63, 6, 5), ("m1", 2, 1): (0.80, 0.986, 8975.1, 9010.7, 5.10, 126, 124),
    ("m2", 1, 4): (12.28, 0.703, 12272.5, 18750.6, 13.17, 14, 10), ("m2", 1, 1): (0.23, 0.997, 18689.0, 18750.6, 8.28, 251, 212),
    ("m2", 2, 4): (0.28, 0.985, 10082.8, 10195.0, 15.68, 7, 12), ("m2", 2, 1): (0.42, 0.990, 10122.4, 10195.0, 3.84, 138, 158),
    ("m3", 1, 4): (108.57, 0.189, 8336.8, 17013.4, 24.75, 15, 12), ("m3", 1, 1): (108.53, 0.189, 8367.2, 17013.4, 40.29, 229, 220),
    ("m3", 2, 4): (0.26, 0.995, 11042.2, 11065.8, 14.92, 7, 12), ("m3", 2, 1): (0.27, 0.995, 10995.8, 11065.8, 14.92, 151, 158),
}
NOT_MET = {("m1", 1, 4), ("m1", 1, 1), ("m1", 2, 4), ("m2", 1, 4), ("m3", 1, 4), ("m3", 1, 1)}


def _accuracy_cases():
    for mesh, seed in SCENES:
        for stride in (4, 1):
            marks = [pytest.mark.xfail(reason=f"accuracy bar not met with the foreground on: measured {MEASURED.get((mesh, seed, stride))}",
                                       strict=True)] if (mesh, seed, stride) in NOT_MET else []
            yield pytest.param(mesh, seed, stride, marks=marks, id=f"{mesh}-{seed}-stride{stride}")


@pytest.mark.parametrize("mesh, seed, stride", list(_accuracy_cases()))
def test_accuracy_with_the_foreground_on(gpu_lib, mesh, seed, stride):
    om, cam, P, sensor, truth, frame = _scene(mesh, 640, 480, seed=100 + seed)
    with sensor, ObjectFinder(sensor, om, _params(seed_stride=stride), foreground=FG()) as fnd:
        r = fnd.find(frame)
        ms = fnd.stage_ms()
        assert r.found
        best = r.poses[0]
        s_truth = _reference_scores(om, cam.camera_matrix, cam.rows, cam.cols, P, frame, truth[None])[0]
        dt = float(np.linalg.norm(best[9:] - truth[9:]))
        iou = _iou(sensor.render_depth(best), sensor.render_depth(truth))
        print(f"ACCURACY {mesh} seed {seed} stride {stride}: |dt| {dt * 1e3:.2f} mm, IoU {iou:.3f}, score {r.scores[0]:.1f} vs truth "
              f"{s_truth:.1f}, find {ms[4]:.1f} ms (stages {[round(x, 3) for x in ms[:4]]}), seeds {len(fnd.stage('seeds')[0])}")
        assert dt < 0.01 and iou >= 0.85 and r.scores[0] >= s_truth - 0.02 * abs(s_truth), (dt, iou, r.scores[0], s_truth)
