"""The pose assessor on the device (rbs_assess_*, dbot_ros_amd/assess.py): every per-body plane against the one-body
oracle render bit for bit, every count and verdict against the numpy twin (tests/assess_twin.py) exactly, batching and
frame sources, no side effects on a tracker over the same sensor, what the verdicts mean on the synthetic scenes, and
the supervisor's loop over a sequence whose object jumps."""
import numpy as np
import pytest

import assess_scenes as asc
import assess_twin as tw
from dbot_ros_amd import RbSensor, RbSensorBuilder, _capi, synth
from dbot_ros_amd.assess import LOST, OCCLUDED, OUT_OF_VIEW, SUPPORTED, PoseAssessor
from dbot_ros_amd.sensor import RbSensorError

pytestmark = pytest.mark.gpu

PARAMS = PoseAssessor.Parameters(**asc.PARAMS)


@pytest.fixture(scope="module")
def scenes():
    """name -> (Scene, sensor, assessor, pose names, Assessment of all the scene's poses in one call): shared, read-only."""
    out = {}
    for name, (meshes, cols, rows) in asc.SCENES.items():
        s = asc.Scene(meshes, cols, rows)
        sensor = RbSensor(s.om, s.cam, s.P, max_particles=1)
        a = PoseAssessor(sensor, PARAMS)
        poses = s.poses()
        assert len(poses) * s.B <= 64
        out[name] = (s, sensor, a, list(poses), a.assess(np.stack(list(poses.values())), s.frame))
    yield out
    for s, sensor, *_ in out.values():
        sensor.close()
        s.close()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("name", list(asc.SCENES))
def test_planes_equal_the_one_body_oracle_and_their_minimum_the_render(gpu_lib, scenes, name):
    s, sensor, a, names, _ = scenes[name]
    poses = s.poses()
    a.assess(np.stack([poses[n] for n in names]), s.frame)       # (the planes of THIS scene's last call)
    for k, pn in enumerate(names):
        want = s.planes(poses[pn])
        got = np.stack([a.plane(k, b) for b in range(s.B)])
        for b in range(s.B):
            assert np.array_equal(bits(got[b]), bits(want[b])), (name, pn, b, int((bits(got[b]) != bits(want[b])).sum()))
        assert np.array_equal(bits(got.min(axis=0)), bits(sensor.render_depth(poses[pn]))), (name, pn)
    with pytest.raises(RbSensorError):
        a.plane(len(names), 0)
    with pytest.raises(RbSensorError):
        a.plane(0, s.B)
    with pytest.raises(RbSensorError):
        a.plane(-1, 0)


@pytest.mark.parametrize("name", list(asc.SCENES))
def test_counts_and_verdicts_equal_the_twin(gpu_lib, scenes, name):
    s, sensor, a, names, got = scenes[name]
    poses = s.poses()
    for k, pn in enumerate(names):
        c, v = s.expect(poses[pn])
        print(name, pn, "device", got.counts[k].tolist(), got.verdicts[k].tolist(), "twin", c.tolist(), v.tolist())
        assert np.array_equal(got.counts[k], c) and np.array_equal(got.verdicts[k], v), (name, pn)
        assert (got.counts[k][:, 1] == got.counts[k][:, 2:5].sum(axis=1)).all() and (got.counts[k][:, 1] <= got.counts[k][:, 0]).all()
    for pn in ("off screen", "behind the camera"):
        k = names.index(pn)
        assert not got.counts[k].any() and (got.verdicts[k] == OUT_OF_VIEW).all(), pn
    k = names.index("fills the image")
    assert got.counts[k][:, 0].sum() >= 0.5 * s.rows * s.cols, got.counts[k].tolist()
    for pn in ("left border", "right border", "top border", "bottom border", "corner"):   # they do straddle the border
        k = names.index(pn)
        full = s.expect(s.at(0.0, 0.0, 0.7))[0][:, 0]
        assert (got.counts[k][:, 0] > 0).all() and (got.counts[k][:, 0] < full).any(), (pn, got.counts[k].tolist(), full.tolist())
    # an all-NaN frame: every owned pixel without a reading
    nan = np.full(s.rows * s.cols, np.nan, dtype=np.float32)
    r = a.assess(s.truth, nan)
    c, v = s.expect(s.truth, nan)
    assert np.array_equal(r.counts[0], c) and np.array_equal(r.verdicts[0], v)
    assert (r.counts[0][:, 0] == got.counts[0][:, 0]).all() and not r.counts[0][:, 1:].any() and (r.verdicts[0] == OCCLUDED).all()


def test_a_duplicate_body_owns_nothing(gpu_lib):
    s = asc.Scene(("m1", "m1"), 80, 60)
    pose = np.stack([s.truth[0], s.truth[0]])
    with RbSensor(s.om, s.cam, s.P, max_particles=1) as sensor:
        a = PoseAssessor(sensor, PARAMS)
        for inspect in (lambda: a.plane(0, 0), a.kernel_ms):           # before the first call there is nothing to inspect
            with pytest.raises(RbSensorError) as e:
                inspect()
            assert e.value.code == _capi.RBS_ERR_INVALID_ARGUMENT
        r = a.assess(pose, s.frame)
        c, v = s.expect(pose)
        assert np.array_equal(r.counts[0], c) and np.array_equal(r.verdicts[0], v)
        assert r.counts[0][0, 0] > 16 and not r.counts[0][1].any() and r.verdicts[0][1] == OUT_OF_VIEW
        assert np.array_equal(bits(a.plane(0, 0)), bits(a.plane(0, 1)))       # the same plane twice: every pixel a tie
    s.close()


@pytest.mark.parametrize("name", ["m1m2_161", "m1_80"])
def test_a_record_does_not_depend_on_its_batch_or_the_frame_source(gpu_lib, scenes, name):
    s, _, _, names, ref = scenes[name]
    poses = s.poses()
    n = 64 // s.B
    rng = np.random.default_rng(8)
    batch = np.stack([poses[names[i]] if i < len(names) else synth.particle_poses(poses[names[i % len(names)]], 1, rng, scale=3.0)[0]
                      for i in range(n)])
    with RbSensor(s.om, s.cam, s.P, max_particles=1) as sensor:
        a = PoseAssessor(sensor, PARAMS)
        alone = {k: a.assess(batch[k], s.frame) for k in (0, 1, n // 2, n - 1)}      # n = 1 first: the buffers grow afterwards
        full = a.assess(batch, s.frame)
        for k, r in alone.items():
            assert np.array_equal(r.counts[0], full.counts[k]) and np.array_equal(r.verdicts[0], full.verdicts[k]), k
        assert np.array_equal(full.counts[:len(names)], ref.counts) and np.array_equal(full.verdicts[:len(names)], ref.verdicts)
        for k in (len(names), n - 1):                                              # the perturbed poses: the twin again
            c, v = s.expect(batch[k])
            assert np.array_equal(full.counts[k], c) and np.array_equal(full.verdicts[k], v), k
        again = a.assess(batch, s.frame)
        assert np.array_equal(again.counts, full.counts)                           # run after run
        sensor.set_observation(s.frame)
        held = a.assess(batch)                                                     # frame = NULL: the sensor's observation
        assert np.array_equal(held.counts, full.counts) and np.array_equal(held.verdicts, full.verdicts)
        assert np.array_equal(sensor.get_observation(), s.frame, equal_nan=True)
        ms = a.kernel_ms()
        assert len(ms) == 2 and all(0.0 < m < 1000.0 for m in ms), ms
        # refusals on a live handle
        with pytest.raises(RbSensorError) as e:
            a.assess(np.concatenate([batch, batch[:1]]), s.frame)
        assert e.value.code == _capi.RBS_ERR_INVALID_ARGUMENT and "exceeds 64" in str(e.value)
        bad = batch[:2].copy()
        bad[1, s.B - 1, 4] = np.nan
        with pytest.raises(RbSensorError) as e:
            a.assess(bad, s.frame)
        assert e.value.code == _capi.RBS_ERR_INVALID_ARGUMENT and "not finite" in str(e.value)
        with pytest.raises(RbSensorError):
            PoseAssessor(sensor, PoseAssessor.Parameters(sigmas=0.0)).assess(batch[:1], s.frame)
        assert np.array_equal(a.assess(batch, s.frame).counts, full.counts)         # a refused call changes nothing


@pytest.mark.parametrize("kw", [dict(state_layout="dense"), dict(precision="f32"), dict(state_layout="window")],
                         ids=["dense", "f32", "windowed"])
def test_layouts_and_precisions_count_alike(gpu_lib, scenes, kw):
    s, _, _, names, ref = scenes["m1m2_161" if "precision" not in kw else "m1_80"]
    poses = s.poses()
    with RbSensor(s.om, s.cam, s.P, max_particles=1, **kw) as sensor:
        r = PoseAssessor(sensor, PARAMS).assess(np.stack([poses[n] for n in names]), s.frame)
    assert np.array_equal(r.counts, ref.counts) and np.array_equal(r.verdicts, ref.verdicts)


def test_assessing_leaves_a_tracker_alone(gpu_lib):
    from dbot_ros_amd.tracker import DeviceParticleTracker, ObjectTransitionBuilder, ParticleTrackerBuilder
    s = asc.Scene(("m1",), 80, 60)
    rng = np.random.default_rng(4)
    truths = [synth.truth_pose(1, z=0.7, frame=k) for k in range(8)]
    frames = [synth.make_frame(s.orc.render_depth(t), s.rows, s.cols, rng) for t in truths]

    def run(assess, look_ahead):
        sensor = RbSensor(s.om, s.cam, RbSensorBuilder.Parameters(sample_count=200), max_particles=200)
        tr = DeviceParticleTracker(ObjectTransitionBuilder(ObjectTransitionBuilder.Parameters(
            0.002, 0.002, 0.002, 0.01, 0.01, 0.01, 0.8)).build(), sensor, s.om, ParticleTrackerBuilder.Parameters(evaluation_count=200),
            device_rng=True, seed=3)
        a = PoseAssessor(sensor, PARAMS)
        tr.initialize([asc.truth_state(s.om, truths[0][0])])
        ests, verdicts = [], []
        if look_ahead:
            tr.submit(frames[0])
            for k in range(1, len(frames)):
                tr.submit(frames[k])
                ests.append(tr.result())
                if assess:
                    with pytest.raises(ValueError):
                        tr.assess(assessor=a)                       # a frame in flight: whose observation?
                    verdicts.append(int(tr.assess(frames[k - 1], assessor=a).verdicts[0, 0]))
            ests.append(tr.result())
            if assess:
                verdicts.append(int(tr.assess(frames[-1], assessor=a).verdicts[0, 0]))
        else:
            for k, fr in enumerate(frames):
                ests.append(tr.track(fr))
                if assess:
                    given = tr.assess(fr, assessor=a)
                    held = tr.assess(assessor=a)                    # the sensor's observation IS this frame
                    assert np.array_equal(given.counts, held.counts)
                    verdicts.append(int(given.verdicts[0, 0]))
        tr.close()
        sensor.close()
        return np.array(ests), verdicts

    for la in (False, True):
        base, _ = run(False, la)
        got, verdicts = run(True, la)
        assert np.array_equal(got, base), la
        assert verdicts == [SUPPORTED] * len(frames), (la, verdicts)    # and a healthy track reads SUPPORTED throughout
    s.close()


def test_what_the_verdicts_mean_on_the_synthetic_scenes(gpu_lib, scenes):
    """Explicit parameters (3.0, 0.5, 0.25, 16).  At the truth every body that is visible enough is SUPPORTED with
    support >= 0.95 u; at +8 cm in x body 0 of the two- and three-body scenes is LOST.  (The reference alone: 44/44,
    246/246, 84/84, 1003/1005, 902/904 supported, the slab-covered third body 50 of 973 OCCLUDED; 12 of 230 and 69 of 959.)"""
    assert (PARAMS.sigmas, PARAMS.min_support_fraction, PARAMS.min_visible_fraction, PARAMS.min_pixels) == (3.0, 0.5, 0.25, 16)
    decided = 0
    for name, (s, _, _, names, got) in scenes.items():
        c, v = got.counts[names.index("truth")], got.verdicts[names.index("truth")]
        for b in range(s.B):
            rendered, support, behind = int(c[b, 0]), int(c[b, 2]), int(c[b, 4])
            u = support + behind
            print(name, "truth body", b, "support / u =", support, "/", u, "of", rendered, tw.verdict(c[b]))
            if u >= 0.25 * rendered:
                assert v[b] == SUPPORTED and support >= 0.95 * u, (name, b, c[b].tolist())
                decided += 1
            else:
                assert v[b] == OCCLUDED, (name, b, c[b].tolist())
    assert decided >= 6
    assert scenes["m1m2m3_322"][4].verdicts[0][2] == OCCLUDED          # the slab covers the third body
    for name in ("m1m2_161", "m1m2m3_322"):
        s, _, _, names, got = scenes[name]
        k = names.index("x+8cm")
        print(name, "x+8cm body 0", got.counts[k][0].tolist())
        assert got.verdicts[k][0] == LOST, (name, got.counts[k].tolist())
        k = names.index("z+2cm")                                       # the documented blind spot: pushed back reads OCCLUDED
        assert (got.verdicts[k] == OCCLUDED).all(), (name, got.counts[k].tolist())


def test_supervisor_reacquires_an_object_that_jumped(gpu_lib):
    from dbot_ros_amd.supervisor import TrackSupervisor
    from dbot_ros_amd.tracker import DeviceParticleTracker, ObjectTransitionBuilder, ParticleTrackerBuilder
    s = asc.Scene(("m1",), 80, 60)
    rng = np.random.default_rng(6)
    n_frames, jump_at = 16, 5
    truths = []
    for k in range(n_frames):
        t = synth.truth_pose(1, z=0.7, frame=k)
        if k >= jump_at:
            t[:, 9] += 0.10                                            # the object jumps 10 cm between two frames
        truths.append(t)
    frames = [synth.make_frame(s.orc.render_depth(t), s.rows, s.cols, rng, occluder=False) for t in truths]
    states = [asc.truth_state(s.om, t[0]) for t in truths]
    index = {fr.tobytes(): k for k, fr in enumerate(frames)}
    with RbSensor(s.om, s.cam, RbSensorBuilder.Parameters(sample_count=400), max_particles=400) as sensor:
        tr = DeviceParticleTracker(ObjectTransitionBuilder(ObjectTransitionBuilder.Parameters(
            0.002, 0.002, 0.002, 0.01, 0.01, 0.01, 0.8)).build(), sensor, s.om, ParticleTrackerBuilder.Parameters(evaluation_count=400),
            device_rng=True, seed=3)
        sup = TrackSupervisor(tr, PoseAssessor(sensor, PARAMS), find=lambda fr: states[index[np.asarray(fr).tobytes()]],
                              lost_frames=3)
        tr.initialize([states[0]])
        events, errs = [], []
        for k, fr in enumerate(frames):
            est, verdicts, ev = sup.step(fr)
            events.append(ev)
            errs.append(float(np.linalg.norm(est[0:3] - states[k][0:3])))
            print(k, ev, verdicts.tolist(), sup.last.counts[0].tolist(), round(errs[-1], 4))
        tr.close()
    s.close()
    assert events[:jump_at] == [None] * jump_at, events
    seen = [e for e in events if e is not None]
    assert seen == ["lost", "reacquired"], events
    at = events.index("reacquired")
    assert at == jump_at + 3 and errs[jump_at] > 0.08                  # three LOST frames, then the search on the next one
    assert max(errs[at:]) < 0.025, errs                                # 80x60: one pixel is 8.8 mm at 0.7 m -> a few pixels


def test_every_tracker_assesses_its_last_estimate(gpu_lib):
    """GaussianTracker and the host ParticleTracker over the device sensor: assess(frame) is the assessor's record of the
    estimate's absolute pose, and both read SUPPORTED while they follow the object."""
    from dbot_ros_amd.assess import state_poses
    from dbot_ros_amd.gaussian import GaussianTracker, GaussianTrackerBuilder
    from dbot_ros_amd.tracker import ObjectTransitionBuilder, ParticleTracker, ParticleTrackerBuilder
    s = asc.Scene(("m1", "m2"), 161, 121)
    rng = np.random.default_rng(9)
    truths = [synth.truth_pose(2, z=0.7, frame=k) for k in range(3)]
    frames = [synth.make_frame(s.orc.render_depth(t), s.rows, s.cols, rng, occluder=False) for t in truths]
    s0 = np.zeros(24)
    for b in range(2):
        s0[12 * b:12 * b + 12] = asc.truth_state(ObjectModelPart(s.om, b), truths[0][b])
    with RbSensor(s.om, s.cam, RbSensorBuilder.Parameters(sample_count=100), max_particles=100) as sensor:
        gp = GaussianTrackerBuilder.Parameters()
        gp.object_transition.part_count = 2
        tp = ObjectTransitionBuilder.Parameters(0.002, 0.002, 0.002, 0.01, 0.01, 0.01, 0.8, part_count=2)
        trackers = [GaussianTracker(sensor, s.om, gp),
                    ParticleTracker(ObjectTransitionBuilder(tp).build(), sensor, s.om, ParticleTrackerBuilder.Parameters(evaluation_count=200),
                                    np.random.default_rng(1))]
        a = PoseAssessor(sensor, PARAMS)
        for tr in trackers:
            with pytest.raises(ValueError):
                tr.assess(frames[0], assessor=a)                        # nothing tracked yet
            tr.initialize([s0])
            for fr in frames:
                est = tr.track(fr.astype(np.float64) if isinstance(tr, GaussianTracker) else fr)
                got = tr.assess(fr, assessor=a)
                ref = a.assess(state_poses(tr, est), fr)
                assert np.array_equal(got.counts, ref.counts) and got.counts.shape == (1, 2, 5)
                c, v = s.expect(state_poses(tr, est)[0], fr)
                assert np.array_equal(got.counts[0], c) and np.array_equal(got.verdicts[0], v)
                assert (got.verdicts == SUPPORTED).all(), (type(tr).__name__, got.counts.tolist())
            assert tr.assess(fr).verdicts.shape == (1, 2)               # its own assessor, the library's defaults
        trackers[0].close()
    s.close()


class ObjectModelPart:
    """One part of an object model, as asc.truth_state reads it."""

    def __init__(self, om, b):
        self.centers = [om.centers[b]]


def test_the_finder_confirms_its_find(gpu_lib):
    from dbot_ros_amd.finder import ObjectFinder
    s = asc.Scene(("m1",), 320, 240)
    p = ObjectFinder.Parameters()
    for k, v in dict(max_seeds=48, n_rotations=128, n_candidates=256, n_survivors=8, rounds=3, children=16, batch=4096, seed=11).items():
        setattr(p, k, v)
    with RbSensor(s.om, s.cam, s.P, max_particles=1) as sensor, ObjectFinder(sensor, s.om, p) as fnd:
        a = PoseAssessor(sensor, PARAMS)
        plain = fnd.find(s.frame)
        assert plain.assessment is None and plain.confirmed is None     # the defaults leave a find as it was
        r = fnd.find(s.frame, assess=a)
        assert r.found == plain.found and np.array_equal(r.poses, plain.poses) and np.array_equal(r.scores, plain.scores)
        K = len(r.poses)
        assert K >= 1 and r.assessment.counts.shape == (K, 1, 5)
        for k in range(K):
            c, v = s.expect(r.poses[k])
            assert np.array_equal(r.assessment.counts[k], c) and np.array_equal(r.assessment.verdicts[k], v), k
        hits = np.nonzero(r.assessment.verdicts[:, 0] == SUPPORTED)[0]
        assert r.confirmed == (int(hits[0]) if hits.size else -1)
        nan = np.full(s.rows * s.cols, np.nan, dtype=np.float32)
        none = fnd.find(nan, assess=a)                                  # no seed, no pose: nothing to confirm
        assert len(none.poses) == 0 and none.confirmed == -1 and none.assessment is None
    s.close()
