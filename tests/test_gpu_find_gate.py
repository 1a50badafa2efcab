"""The finder's silhouette gate through the release library (rbs_find_set_gate, rbs_find_get_evidence; ObjectFinder.Gate,
SceneFinder(gate=)): off after having been on it changes no bit of a find; on, every stage's order is the numpy twin's
(tests/find_gate_twin.py) from the device's own scores and records, the records are rbs_contour_poses' of the same poses and
frame, and `found` follows require_confirmed; the outcome on the two-body scene of DESIGN.md Appendix K; and a tracker over
the sensor is left alone."""
import math

import numpy as np
import pytest

import find_gate_scenes as gs
import find_gate_twin as gt
import find_twin as ft
import scene_find_scenes as ss
from dbot_ros_amd import RbSensor, RbSensorBuilder, _capi, synth
from dbot_ros_amd.assess import PoseAssessor
from dbot_ros_amd.finder import ObjectFinder, SceneFinder
from dbot_ros_amd.sensor import RbSensorError
from test_gpu_finder import _iou, _params, _scene

pytestmark = pytest.mark.gpu

STAGES = ("seeds", "coarse", "candidates", "survivors", "result")
GATE = ObjectFinder.Gate
SMALL = dict(ss.SMALL, batch=1024)             # 6 144 hypotheses in six scoring calls


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


def test_off_after_on_is_a_finder_never_configured(gpu_lib):
    om, cam, P, sensor, truth, frame = _scene("m1", 160, 120, seed=3)
    p = _params(**SMALL, seed=11)
    with sensor:
        with ObjectFinder(sensor, om, p) as plain:
            want_r = plain.find(frame)
            want = _all_stages(plain, p.rounds)
            assert want_r.classes is None
            for call in (lambda: plain.evidence("coarse"), plain.gate_ms):   # no find with the stage: no evidence
                with pytest.raises(RbSensorError) as e:
                    call()
                assert e.value.code == _capi.RBS_ERR_INVALID_ARGUMENT
        with ObjectFinder(sensor, om, p, gate=GATE(enabled=False)) as off:
            assert off.gate is None
            r = off.find(frame)
            _assert_same_bits(_all_stages(off, p.rounds) + [r.poses, r.scores], want + [want_r.poses, want_r.scores])
        with ObjectFinder(sensor, om, p) as toggled:
            toggled.set_gate(GATE())
            on = toggled.find(frame)
            assert on.classes is not None and len(on.classes) == len(on.poses)
            _assert_same_bits(_all_stages(toggled, 0)[:8], want[:8])          # seeds and coarse scores are the same
            toggled.set_gate(None)
            r = toggled.find(frame)
            assert r.classes is None and r.found == want_r.found
            _assert_same_bits(_all_stages(toggled, p.rounds) + [r.poses, r.scores], want + [want_r.poses, want_r.scores])
            with pytest.raises(RbSensorError):
                toggled.evidence("result")
            toggled.set_gate(GATE())
            toggled.set_gate(GATE(enabled=False))                              # enabled = 0 is off too
            toggled.find(frame)
            _assert_same_bits(_all_stages(toggled, p.rounds), want)


def test_bad_settings_are_refused_and_the_previous_one_stays(gpu_lib):
    om, cam, P, sensor, truth, frame = _scene("m1_l2", 160, 120, seed=4)
    p = _params(**ss.TINY)
    nan = float("nan")
    bad = (GATE(radius=0), GATE(radius=9), GATE(min_rim_pixels=0), GATE(min_pixels=0), GATE(sigmas=0.0), GATE(sigmas=nan),
           GATE(min_support_fraction=1.5), GATE(min_visible_fraction=-0.1), GATE(min_valid_fraction=nan), GATE(min_contour_fraction=1.01),
           GATE(min_flush_fraction=-1.0))
    first = GATE(radius=3, min_contour_fraction=0.25)
    with sensor, ObjectFinder(sensor, om, p, gate=first) as fnd:
        on = fnd.find(frame)
        ev = fnd.evidence("coarse")
        for g in bad:
            with pytest.raises(RbSensorError) as e:
                fnd.set_gate(g)
            assert e.value.code == _capi.RBS_ERR_INVALID_ARGUMENT, g
            assert fnd.gate == first
        again = fnd.find(frame)                                               # still the setting of before, and the same bits
        _assert_same_bits([again.poses, again.scores, again.classes, *fnd.evidence("coarse")], [on.poses, on.scores, on.classes, *ev])
        with pytest.raises(RbSensorError):
            fnd.evidence(_capi.RBS_FIND_SEEDS)
        with pytest.raises(RbSensorError):
            fnd.evidence(_capi.RBS_FIND_CHILDREN)


def _check_find_against_the_twin(fnd, p, gate, assessor, frame, found, classes):
    """Every stage of fnd's last find: the orders from the device's own scores and records, the records from rbs_contour_poses."""
    params = {k: getattr(gate, k) for k in gt.DEFAULTS}
    hyp, hs, hidx, info = fnd.stage("coarse")
    rec, cls = fnd.evidence("coarse")
    H = len(hs)
    assert rec.shape == (H, 10) and cls.shape == (H,) and H > p.batch
    assert np.array_equal(cls, [gt.class_of(r, **params) for r in rec])
    n0 = int((cls == 0).sum())
    # a sample across the scoring calls: the records are the assessor's of the same pose and (coarse = full here) frame
    rng = np.random.default_rng(0)
    pick = np.unique(np.concatenate([[0, p.batch - 1, p.batch, H - 1], rng.choice(H, 44, replace=False), np.nonzero(cls == 0)[0][:12]]))
    a = assessor.assess(hyp[pick][:, None, :], frame)
    assert np.array_equal(rec[pick, :5], a.counts[:, 0]) and np.array_equal(rec[pick, 5:], a.contour_counts[:, 0])
    assert np.array_equal(cls[pick] == 0, a.confirmed_mask())
    # step 5
    cp, cscore, cidx, _ = fnd.stage("candidates")
    ws, wi = gt.gated_topk(hs, cls, p.n_candidates)
    assert np.array_equal(cidx, wi) and np.array_equal(_bits(cscore), _bits(ws))
    crec, ccls = fnd.evidence("candidates")
    assert np.array_equal(crec, rec[cidx]) and np.array_equal(ccls, cls[cidx])
    assert (ccls[:min(n0, p.n_candidates)] == 0).all() and (ccls[n0:] == 1).all()
    sp, sscore, sidx, _ = fnd.stage("survivors")
    kept = ft.nms(cp, p.nms_translation, p.nms_angle, p.n_survivors, cscore)
    assert np.array_equal(sidx, cidx[kept]) and np.array_equal(_bits(sp), _bits(cp[kept]))
    srec, scls = fnd.evidence("survivors")
    assert np.array_equal(srec, rec[sidx]) and np.array_equal(scls, cls[sidx])
    # step 7
    fp, fs, fk, _ = fnd.stage("result")
    frec, fcls = fnd.evidence("result")
    S = len(fs)
    assert S == len(sidx) and sorted(fk.tolist()) == list(range(S))
    by_k_s, by_k_c = np.empty(S), np.empty(S, dtype=np.int64)
    by_k_s[fk], by_k_c[fk] = fs, fcls
    order = gt.result_order(by_k_s, by_k_c)
    assert np.array_equal(fk, order)
    assert np.array_equal(fcls, [gt.class_of(r, **params) for r in frec])
    a = assessor.assess(fp[:, None, :], frame)
    assert np.array_equal(frec[:, :5], a.counts[:, 0]) and np.array_equal(frec[:, 5:], a.contour_counts[:, 0])
    assert found == gt.found(by_k_s, by_k_c, order, p.min_score, gate.require_confirmed)
    if classes is not None:
        assert np.array_equal(classes, fcls[:len(classes)])
    ms = fnd.gate_ms()
    assert len(ms) == 2 and ms[0] > 0.0 and ms[1] > 0.0
    return cls, ccls, fcls


def _assessor(sensor, gate):
    return PoseAssessor(sensor, PoseAssessor.Parameters(**{k: getattr(gate, k) for k in gt.ASSESS_KEYS}),
                        PoseAssessor.ContourParameters(**{k: getattr(gate, k) for k in gt.CONTOUR_KEYS}))


@pytest.mark.parametrize("gate", [GATE(), GATE(require_confirmed=True, radius=1), GATE(radius=8, min_contour_fraction=0.9)],
                         ids=["default", "require_r1", "r8_strict"])
def test_every_stage_is_the_twins_from_the_devices_scores_and_records(gpu_lib, gate):
    om, cam, P, sensor, truth, frame = _scene("m1", 160, 120, seed=3)
    p = _params(**SMALL, seed=11)
    with sensor, ObjectFinder(sensor, om, p, gate=gate) as fnd:
        r = fnd.find(frame)
        cls, ccls, fcls = _check_find_against_the_twin(fnd, p, gate, _assessor(sensor, gate), frame, r.found, r.classes)
        print(gate, "confirmed hypotheses", int((cls == 0).sum()), "of", len(cls), "candidates", int((ccls == 0).sum()), "finals",
              int((fcls == 0).sum()), "found", r.found, "|dt| mm", round(1e3 * float(np.linalg.norm(r.poses[0, 9:] - truth[9:])), 2))
        again = fnd.find(frame)
        _assert_same_bits([again.poses, again.scores, again.classes], [r.poses, r.scores, r.classes])
        if gate.require_confirmed:
            assert r.found == bool(fcls[0] == 0)


def test_a_body_of_a_two_body_sensor_through_the_scene_finder(gpu_lib):
    s = ss.Scene(("m1", "m2"), 160, 120, 3)
    p = _params(**SMALL, seed=11)
    gate = GATE()
    with RbSensor(s.om, s.cam, s.P, max_particles=1) as sensor, SceneFinder(sensor, s.om, p, gate=gate) as fnd:
        res = fnd.find(s.frame)
        order, _ = fnd.order()
        for b in order:
            om1 = s.part_model(b)
            with RbSensor(om1, s.cam, s.P, max_particles=1) as one:
                body = fnd.body_finder(b)
                assert body.gate == gate
                _check_find_against_the_twin(body, p, gate, _assessor(one, gate), fnd.residual(b), bool(res.found[b]), None)
        with pytest.raises(RbSensorError) as e:
            fnd.set_gate(GATE(radius=0))
        assert e.value.code == _capi.RBS_ERR_INVALID_ARGUMENT and fnd.gate == gate
        fnd.set_gate(None)
        fnd.find(s.frame)
        with pytest.raises(RbSensorError):
            fnd.body_finder(order[0]).evidence("coarse")


def _planes(assessor, poses, frame):
    assessor.assess(poses[None], frame)
    return np.stack([assessor.plane(0, b) for b in range(len(poses))])


@pytest.fixture(scope="module")
def outcome(gpu_lib):
    """The scene of tests/find_gate_scenes.py at the settings of tests/test_gpu_scene_find.py's accuracy test, found with the
    gate off, on, and on with require_confirmed: {name: (SceneFindResult, |dt| [B], IoU [B], confirmed finals per body)}."""
    s = gs.scene()
    p = _params(**gs.FIND)
    out = {"scene": s}
    with RbSensor(s.om, s.cam, s.P, max_particles=1) as sensor:
        a = PoseAssessor(sensor)
        true_planes = _planes(a, s.truth, s.frame).reshape(s.B, -1)
        for name, gate in (("off", None), ("on", GATE()), ("require", GATE(require_confirmed=True))):
            with SceneFinder(sensor, s.om, p, foreground=ObjectFinder.Foreground(), refinement=ObjectFinder.Refinement(), gate=gate) as fnd:
                r = fnd.find(s.frame)
                conf = [int((fnd.body_finder(b).evidence("result")[1] == 0).sum()) if gate else None for b in range(s.B)]
                hyp = [int((fnd.body_finder(b).evidence("coarse")[1] == 0).sum()) if gate else None for b in range(s.B)]
                ms = [fnd.body_finder(b).gate_ms() + fnd.body_finder(b).stage_ms() if gate else fnd.body_finder(b).stage_ms() for b in range(s.B)]
            got = _planes(a, np.where(np.isfinite(r.poses), r.poses, s.truth), s.frame).reshape(s.B, -1)
            dts = [float(np.linalg.norm(r.poses[b, 9:] - s.truth[b, 9:])) for b in range(s.B)]
            ious = [float(_iou(got[b], true_planes[b])) for b in range(s.B)]
            print(f"gate {name}: |dt| mm {[round(1e3 * d, 2) for d in dts]}, IoU {[round(i, 3) for i in ious]}, found {r.found.tolist()}, "
                  f"scores {r.scores.tolist()}, joint {r.joint_score:.1f}, confirmed finals {conf}, confirmed hypotheses {hyp}, "
                  f"ms (gate 4b, gate 7, stages) {[[round(float(x), 2) for x in m] for m in ms]}")
            out[name] = (r, dts, ious, conf)
    return out


def test_the_gate_finds_the_visible_body_of_the_two_body_scene(outcome):
    """Without the gate body m1 ends in the slab, 0.4 m off; with it m1 is found."""
    r, dts, ious, conf = outcome["on"]
    assert r.found[0] and dts[0] < 0.010 and ious[0] >= 0.85, (dts, ious)
    assert conf[0] >= 1
    off = outcome["off"]
    assert off[1][0] > 0.3, off[1]


def test_require_confirmed_leaves_the_hidden_body_unplaced(outcome):
    r, dts, ious, conf = outcome["require"]
    assert not r.found[1], (dts, ious, conf)
    assert r.found[0] and dts[0] < 0.010 and ious[0] >= 0.85, (dts, ious)


def test_a_gated_find_leaves_a_tracker_alone(gpu_lib):
    from assess_scenes import truth_state
    from dbot_ros_amd.tracker import DeviceParticleTracker, ObjectTransitionBuilder, ParticleTrackerBuilder
    s = ss.Scene(("m1",), 80, 60, 3)
    rng = np.random.default_rng(4)
    truths = [synth.truth_pose(1, z=0.7, frame=k) for k in range(5)]
    orc = s.oracle()
    frames = [synth.make_frame(orc.render_depth(t), s.rows, s.cols, rng) for t in truths]
    p = _params(**ss.TINY)

    def run(find):
        sensor = RbSensor(s.om, s.cam, RbSensorBuilder.Parameters(sample_count=200), max_particles=200)
        tr = DeviceParticleTracker(ObjectTransitionBuilder(ObjectTransitionBuilder.Parameters(
            0.002, 0.002, 0.002, 0.01, 0.01, 0.01, 0.8, 1)).build(), sensor, s.om, ParticleTrackerBuilder.Parameters(evaluation_count=200),
            device_rng=True, seed=3)
        fnd = ObjectFinder(sensor, s.om, p, gate=GATE(require_confirmed=True)) if find else None
        tr.initialize([truth_state(s.om, truths[0])])
        ests, finds = [], []
        for fr in frames:
            ests.append(tr.track(fr))
            if find:
                given, held = fnd.find(fr), fnd.find()                     # frame=None: the sensor's observation IS this frame
                _assert_same_bits([given.poses, given.scores, given.classes], [held.poses, held.scores, held.classes])
                finds.append(given)
        if fnd is not None:
            fnd.close()
        tr.close()
        sensor.close()
        return np.array(ests), finds

    base, _ = run(False)
    got, finds = run(True)
    assert np.array_equal(got, base)
    assert all(f.classes is not None for f in finds)
