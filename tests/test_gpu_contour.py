"""The contour rule on the device (rbs_contour_*, dbot_ros_amd/assess.py): every count and verdict against the numpy
twin (tests/contour_twin.py) exactly at radius 1, 2 and 8, the assess records and planes beside it unchanged, batching and
frame sources, no side effects on a tracker over the same sensor, what the verdicts mean on the synthetic scenes and on
poses planted in the background plane, the supervisor's loop with the rule on, and the finder's finds."""
import ctypes as C

import numpy as np
import pytest

import assess_scenes as asc
import contour_scenes as cs
import contour_twin as ct
from dbot_ros_amd import RbSensor, RbSensorBuilder, _capi, synth
from dbot_ros_amd.assess import (CONTOUR_ABSENT, CONTOUR_NO_RIM, CONTOUR_PRESENT, CONTOUR_UNDECIDED, CONTOUR_VERDICTS, OCCLUDED,
                                 SUPPORTED, VERDICTS, PoseAssessor)
from dbot_ros_amd.sensor import RbSensorError

pytestmark = pytest.mark.gpu

PARAMS = PoseAssessor.Parameters(**asc.PARAMS)
RADII = (1, 2, 8)


def contour_params(radius=2):
    return PoseAssessor.ContourParameters(**dict(cs.PARAMS, radius=radius))


@pytest.fixture(scope="module")
def scenes():
    """name -> (Scene, sensor, pose names, poses [n, B, 12], {radius: Assessment of all poses in one call}): shared, read-only."""
    out = {}
    for name, (meshes, cols, rows) in asc.SCENES.items():
        s = asc.Scene(meshes, cols, rows)
        sensor = RbSensor(s.om, s.cam, s.P, max_particles=1)
        poses = cs.poses(s)
        assert len(poses) * s.B <= 64
        stack = np.stack(list(poses.values()))
        got = {r: PoseAssessor(sensor, PARAMS, contour_params(r)).assess(stack, s.frame) for r in RADII}
        out[name] = (s, sensor, list(poses), stack, got)
    yield out
    for s, sensor, *_ in out.values():
        sensor.close()
        s.close()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def sane(c):
    """valid == flush + in_front + beyond <= rim, everywhere."""
    c = np.asarray(c).reshape(-1, 5)
    return bool((c[:, 1] == c[:, 2:5].sum(axis=1)).all() and (c[:, 1] <= c[:, 0]).all() and (c >= 0).all())


@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("name", list(asc.SCENES))
def test_counts_and_verdicts_equal_the_twin(gpu_lib, scenes, name, radius):
    s, sensor, names, stack, results = scenes[name]
    got = results[radius]
    assert got.contour_counts.shape == (len(names), s.B, 5) and got.contour_verdicts.shape == (len(names), s.B)
    for k, pn in enumerate(names):
        c, v = cs.expect(s, stack[k], radius=radius)
        print(name, "r", radius, pn, "device", got.contour_counts[k].tolist(), got.contour_verdicts[k].tolist(), "twin", c.tolist(), v.tolist())
        assert np.array_equal(got.contour_counts[k], c) and np.array_equal(got.contour_verdicts[k], v), (name, radius, pn)
    assert sane(got.contour_counts)
    for pn in ("off screen", "behind the camera"):
        k = names.index(pn)
        assert not got.contour_counts[k].any() and (got.contour_verdicts[k] == CONTOUR_NO_RIM).all(), pn
    for pn in ("left border", "right border", "top border", "bottom border", "corner", "truth"):
        assert (got.contour_counts[names.index(pn)][:, 0] > 0).any(), pn
    # an all-NaN frame: every rim pixel without a reading
    nan = np.full(s.rows * s.cols, np.nan, dtype=np.float32)
    a = PoseAssessor(sensor, PARAMS, contour_params(radius))
    r = a.assess(s.truth, nan)
    c, v = cs.expect(s, s.truth, nan, radius=radius)
    assert np.array_equal(r.contour_counts[0], c) and np.array_equal(r.contour_verdicts[0], v)
    k = names.index("truth")
    assert (r.contour_counts[0][:, 0] == got.contour_counts[k][:, 0]).all() and not r.contour_counts[0][:, 1:].any()
    assert set(r.contour_verdicts[0].tolist()) <= {CONTOUR_UNDECIDED, CONTOUR_NO_RIM}
    for counts, verdicts in ((got.contour_counts, got.contour_verdicts), (r.contour_counts, r.contour_verdicts)):
        for row, vv in zip(counts.reshape(-1, 5), verdicts.reshape(-1)):   # the host verdict, through the Python wrapper
            assert a.contour_verdict(row) == vv


@pytest.mark.parametrize("name", list(asc.SCENES))
def test_the_assess_records_and_planes_beside_it_are_rbs_assess_poses(gpu_lib, scenes, name):
    s, sensor, names, stack, results = scenes[name]
    plain = PoseAssessor(sensor, PARAMS).assess(stack, s.frame)
    assert plain.contour_counts is None and plain.contour_verdicts is None
    for r in RADII:
        assert np.array_equal(results[r].counts, plain.counts) and np.array_equal(results[r].verdicts, plain.verdicts), r
    for k in range(len(names)):
        c, v = s.expect(stack[k])
        assert np.array_equal(plain.counts[k], c) and np.array_equal(plain.verdicts[k], v)
    a = PoseAssessor(sensor, PARAMS, contour_params(2))
    again = a.assess(stack, s.frame)
    for k, pn in enumerate(names):                                       # the planes of THIS call
        want = s.planes(stack[k])
        for b in range(s.B):
            got = a.plane(k, b)
            assert np.array_equal(bits(got), bits(want[b])), (name, pn, b)
    # out_assess = NULL: the contour records alone, the same
    lib = _capi.load()
    n = len(names)
    cout = (_capi.RbsContourBody * (n * s.B))()
    cp, cc = PARAMS.c_params(), contour_params(2).c_params()
    P = np.ascontiguousarray(stack, dtype=np.float64)
    sensor._check(lib.rbs_contour_poses(sensor._h, C.byref(cp), C.byref(cc), s.frame.ctypes.data_as(C.POINTER(C.c_float)),
                                        P.ctypes.data_as(C.POINTER(C.c_double)), n, None, cout))
    rec = np.frombuffer(cout, dtype=np.int32).reshape(n, s.B, 8)
    assert np.array_equal(rec[:, :, :5], again.contour_counts) and np.array_equal(rec[:, :, 5], again.contour_verdicts)
    assert not rec[:, :, 6:].any()
    # NULL parameters are the defaults (here: the stated ones)
    sensor._check(lib.rbs_contour_poses(sensor._h, None, None, s.frame.ctypes.data_as(C.POINTER(C.c_float)),
                                        P.ctypes.data_as(C.POINTER(C.c_double)), n, None, cout))
    assert np.array_equal(np.frombuffer(cout, dtype=np.int32).reshape(n, s.B, 8)[:, :, :6], rec[:, :, :6])


def test_a_duplicate_body_has_no_rim(gpu_lib):
    s = asc.Scene(("m1", "m1"), 80, 60)
    pose = np.stack([s.truth[0], s.truth[0]])
    with RbSensor(s.om, s.cam, s.P, max_particles=1) as sensor:
        a = PoseAssessor(sensor, PARAMS, contour_params(2))
        with pytest.raises(RbSensorError) as e:                            # before the first call there is nothing to time
            a.kernel_ms()
        assert e.value.code == _capi.RBS_ERR_INVALID_ARGUMENT
        r = a.assess(pose, s.frame)
        c, v = cs.expect(s, pose)
        assert np.array_equal(r.contour_counts[0], c) and np.array_equal(r.contour_verdicts[0], v)
        assert r.contour_counts[0][0, 0] > 16 and not r.contour_counts[0][1].any() and r.contour_verdicts[0][1] == CONTOUR_NO_RIM
        assert not r.counts[0][1].any()
        PoseAssessor(sensor, PARAMS).assess(pose, s.frame)                 # a plain call: the contour kernel's time is gone
        with pytest.raises(RbSensorError):
            a.kernel_ms()
    s.close()


@pytest.mark.parametrize("name", ["m1m2_161", "m1_80"])
def test_a_record_does_not_depend_on_its_batch_or_the_frame_source(gpu_lib, scenes, name):
    s, _, names, stack, results = scenes[name]
    ref = results[2]
    n = 64 // s.B
    rng = np.random.default_rng(8)
    batch = np.stack([stack[i] if i < len(names) else synth.particle_poses(stack[i % len(names)], 1, rng, scale=3.0)[0] for i in range(n)])
    with RbSensor(s.om, s.cam, s.P, max_particles=1) as sensor:
        a = PoseAssessor(sensor, PARAMS, contour_params(2))
        alone = {k: a.assess(batch[k], s.frame) for k in (0, 1, n // 2, n - 1)}      # n = 1 first: the buffers grow afterwards
        full = a.assess(batch, s.frame)
        for k, r in alone.items():
            assert np.array_equal(r.contour_counts[0], full.contour_counts[k]) and np.array_equal(r.contour_verdicts[0], full.contour_verdicts[k]), k
            assert np.array_equal(r.counts[0], full.counts[k])
        assert np.array_equal(full.contour_counts[:len(names)], ref.contour_counts)
        assert np.array_equal(full.contour_verdicts[:len(names)], ref.contour_verdicts)
        for k in (len(names), n - 1):                                              # the perturbed poses: the twin again
            c, v = cs.expect(s, batch[k])
            assert np.array_equal(full.contour_counts[k], c) and np.array_equal(full.contour_verdicts[k], v), k
        again = a.assess(batch, s.frame)                                           # run after run
        assert np.array_equal(again.contour_counts, full.contour_counts) and np.array_equal(again.counts, full.counts)
        sensor.set_observation(s.frame)
        held = a.assess(batch)                                                     # frame = NULL: the sensor's observation
        assert np.array_equal(held.contour_counts, full.contour_counts) and np.array_equal(held.contour_verdicts, full.contour_verdicts)
        assert np.array_equal(held.counts, full.counts)
        assert np.array_equal(sensor.get_observation(), s.frame, equal_nan=True)
        ms = a.kernel_ms()
        assert len(ms) == 3 and all(0.0 < m < 1000.0 for m in ms), ms
        # refusals on a live handle
        with pytest.raises(RbSensorError) as e:
            a.assess(np.concatenate([batch, batch[:1]]), s.frame)
        assert e.value.code == _capi.RBS_ERR_INVALID_ARGUMENT and "exceeds 64" in str(e.value)
        for bad in (dict(radius=0), dict(radius=9), dict(min_rim_pixels=0), dict(min_flush_fraction=1.5)):
            with pytest.raises(RbSensorError) as e:
                PoseAssessor(sensor, PARAMS, PoseAssessor.ContourParameters(**bad)).assess(batch[:1], s.frame)
            assert e.value.code == _capi.RBS_ERR_INVALID_ARGUMENT and "contour" in str(e.value)
        assert np.array_equal(a.assess(batch, s.frame).contour_counts, full.contour_counts)   # a refused call changes nothing


@pytest.mark.parametrize("kw", [dict(state_layout="dense"), dict(precision="f32"), dict(state_layout="window")],
                         ids=["dense", "f32", "windowed"])
def test_layouts_and_precisions_count_alike(gpu_lib, scenes, kw):
    s, _, names, stack, results = scenes["m1m2_161" if "precision" not in kw else "m1_80"]
    with RbSensor(s.om, s.cam, s.P, max_particles=1, **kw) as sensor:
        r = PoseAssessor(sensor, PARAMS, contour_params(2)).assess(stack, s.frame)
    assert np.array_equal(r.contour_counts, results[2].contour_counts) and np.array_equal(r.contour_verdicts, results[2].contour_verdicts)
    assert np.array_equal(r.counts, results[2].counts)


def test_a_contour_assessment_leaves_a_tracker_alone(gpu_lib):
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
        a = PoseAssessor(sensor, PARAMS, contour_params(2))
        tr.initialize([asc.truth_state(s.om, truths[0][0])])
        ests, ok = [], []
        if look_ahead:
            tr.submit(frames[0])
            for k in range(1, len(frames)):
                tr.submit(frames[k])
                ests.append(tr.result())
                if assess:
                    ok.append(bool(tr.assess(frames[k - 1], assessor=a).confirmed_mask()[0]))
            ests.append(tr.result())
            if assess:
                ok.append(bool(tr.assess(frames[-1], assessor=a).confirmed_mask()[0]))
        else:
            for fr in frames:
                ests.append(tr.track(fr))
                if assess:
                    given = tr.assess(fr, assessor=a)
                    held = tr.assess(assessor=a)                    # the sensor's observation IS this frame
                    assert np.array_equal(given.contour_counts, held.contour_counts)
                    ok.append(bool(given.confirmed_mask()[0]))
        tr.close()
        sensor.close()
        return np.array(ests), ok

    for la in (False, True):
        base, _ = run(False, la)
        got, ok = run(True, la)
        assert np.array_equal(got, base), la
        print("look ahead", la, "confirmed", ok)
        assert ok == [True] * len(frames), (la, ok)                 # a healthy track reads SUPPORTED and PRESENT throughout
    s.close()


# The planted in-wall bodies that the plain rule confirms, with the twin's contour verdict (computed on the CPU from
# the one-body oracle's planes; the counts: DESIGN.md Appendix J).  m1_80's in-wall pose has 16 rendered pixels and
# sits at the edge of every threshold: it is held to the twin above and left out here.
IN_WALL = {("m1_640", 10, 0): CONTOUR_ABSENT, ("m1_640", 20, 0): CONTOUR_ABSENT, ("m1_640", 30, 0): CONTOUR_UNDECIDED,
           ("m1m2_161", 10, 0): CONTOUR_ABSENT, ("m1m2_161", 20, 0): CONTOUR_ABSENT, ("m1m2_161", 30, 0): CONTOUR_UNDECIDED,
           ("m1m2m3_322", 10, 1): CONTOUR_ABSENT, ("m1m2m3_322", 20, 1): CONTOUR_ABSENT, ("m1m2m3_322", 30, 1): CONTOUR_ABSENT}


def test_what_the_contour_verdicts_mean_on_the_synthetic_scenes(gpu_lib, scenes):
    """Stated parameters (radius 2, 16, 0.5, 0.3, 0.5).  At the truth every body that reads SUPPORTED reads PRESENT; a
    body planted in the background plane that reads SUPPORTED does not, and confirmed_mask() refuses the pose the plain
    verdict alone would confirm."""
    assert cs.PARAMS == dict(radius=2, min_rim_pixels=16, min_valid_fraction=0.5, min_contour_fraction=0.3, min_flush_fraction=0.5)
    decided = 0
    for name, (s, _, names, stack, results) in scenes.items():
        got = results[2]
        k = names.index("truth")
        for b in range(s.B):
            print(name, "truth body", b, VERDICTS[got.verdicts[k, b]], got.contour_counts[k, b].tolist(), CONTOUR_VERDICTS[got.contour_verdicts[k, b]])
            if got.verdicts[k, b] == SUPPORTED:
                assert got.contour_verdicts[k, b] == CONTOUR_PRESENT, (name, b, got.contour_counts[k, b].tolist())
                decided += 1
        assert bool(got.confirmed_mask()[k]) == bool((got.verdicts[k] == SUPPORTED).all())
    assert decided == 6
    assert scenes["m1m2m3_322"][4][2].verdicts[0][2] == OCCLUDED           # the slab covers the third body
    assert scenes["m1m2m3_322"][4][2].contour_verdicts[0][2] == CONTOUR_UNDECIDED
    seen = set()
    for name, (s, _, names, stack, results) in scenes.items():
        if name == "m1_80":
            continue
        got = results[2]
        for off in cs.OFFSETS_MM:
            k = names.index("in wall +%d mm" % off)
            ca, va = s.expect(stack[k])                                    # the twin, on the CPU
            cc, vc = cs.expect(s, stack[k])
            for b in range(s.B):
                print(name, "in wall +%d mm body" % off, b, ca[b].tolist(), VERDICTS[va[b]], cc[b].tolist(), CONTOUR_VERDICTS[vc[b]])
                if va[b] != SUPPORTED:
                    continue
                assert vc[b] == IN_WALL[(name, off, b)]                     # the planted case is what it was chosen for
                seen.add((name, off, b))
                assert got.verdicts[k, b] == SUPPORTED and got.contour_verdicts[k, b] == vc[b] != CONTOUR_PRESENT
            if (va == SUPPORTED).all():                                    # the plain verdict alone would confirm it
                assert not got.confirmed_mask()[k], (name, off)
                plain = PoseAssessor(scenes[name][1], PARAMS).assess(stack[k], s.frame)
                assert plain.confirmed_mask()[0]
    assert seen == set(IN_WALL)


def _jump_sequence(s, n_frames, jump_at, seed):
    rng = np.random.default_rng(seed)
    truths = []
    for k in range(n_frames):
        t = synth.truth_pose(1, z=0.7, frame=k)
        if k >= jump_at:
            t[:, 9] += 0.10                                            # the object jumps 10 cm between two frames
        truths.append(t)
    frames = [synth.make_frame(s.orc.render_depth(t), s.rows, s.cols, rng, occluder=False) for t in truths]
    return truths, frames, [asc.truth_state(s.om, t[0]) for t in truths]


@pytest.mark.parametrize("stub", ["truth", "in wall"])
def test_supervisor_with_the_contour_rule_on(gpu_lib, stub):
    """tests/test_gpu_assess.py's jump at 161 x 121 with the contour rule on: the finder stubbed with the truth reacquires;
    stubbed with a pose in the background plane that the plain rule confirms, the find fails."""
    from dbot_ros_amd.supervisor import TrackSupervisor
    from dbot_ros_amd.tracker import DeviceParticleTracker, ObjectTransitionBuilder, ParticleTrackerBuilder
    s = asc.Scene(("m1",), 161, 121)
    n_frames, jump_at = 12, 4
    truths, frames, states = _jump_sequence(s, n_frames, jump_at, seed=6)
    index = {fr.tobytes(): k for k, fr in enumerate(frames)}
    wall = cs.in_wall(s, 20)
    searched = []

    def find(fr):
        k = index[np.asarray(fr).tobytes()]
        searched.append(k)
        return states[k] if stub == "truth" else asc.truth_state(s.om, wall[0])

    with RbSensor(s.om, s.cam, RbSensorBuilder.Parameters(sample_count=400), max_particles=400) as sensor:
        tr = DeviceParticleTracker(ObjectTransitionBuilder(ObjectTransitionBuilder.Parameters(
            0.002, 0.002, 0.002, 0.01, 0.01, 0.01, 0.8)).build(), sensor, s.om, ParticleTrackerBuilder.Parameters(evaluation_count=400),
            device_rng=True, seed=3)
        sup = TrackSupervisor(tr, PoseAssessor(sensor, PARAMS, contour_params(2)), find=find, lost_frames=3)
        tr.initialize([states[0]])
        events, errs = [], []
        for k, fr in enumerate(frames):
            est, verdicts, ev = sup.step(fr)
            events.append(ev)
            errs.append(float(np.linalg.norm(est[0:3] - states[k][0:3])))
            print(k, ev, verdicts.tolist(), sup.last.counts[0].tolist(), sup.last.contour_counts[0].tolist(), round(errs[-1], 4))
        tr.close()
    assert events[:jump_at] == [None] * jump_at, events
    seen = [e for e in events if e is not None]
    at = jump_at + 3
    if stub == "truth":
        assert seen == ["lost", "reacquired"] and events.index("reacquired") == at, events
        assert max(errs[at:]) < 0.015, errs                            # 161 x 121: one pixel is 4.4 mm at 0.7 m
    else:
        assert searched and searched[0] == at
        for k in searched:                                             # the twin, on the CPU: the plain rule confirms the stub, the contour does not
            assert s.expect(wall, frames[k])[1].tolist() == [SUPPORTED], k
            assert cs.expect(s, wall, frames[k])[1][0] != CONTOUR_PRESENT, k
        assert seen[:2] == ["lost", "find_failed"] and "reacquired" not in seen and events[at] == "find_failed", events
    s.close()


def _finder_scene(s, seed):
    """tools/find_object_timing.py's scene (DESIGN.md Appendices F and J) over Scene s's camera: truth [12] and frame."""
    from dbot_ros_amd.pose import quat_to_matrix
    rng = np.random.default_rng(seed)
    q = rng.normal(size=4)
    R = quat_to_matrix(q / np.linalg.norm(q))
    z = rng.uniform(0.55, 0.9)
    K = s.cam.camera_matrix
    u, v = rng.uniform(0.3, 0.7) * s.cols, rng.uniform(0.3, 0.7) * s.rows
    truth = np.concatenate([R.ravel(), [(u - K[0, 2]) / K[0, 0] * z, (v - K[1, 2]) / K[1, 1] * z, z]])
    d = s.parts[0].render_depth(truth)
    return truth, synth.make_frame(np.where(np.isfinite(d), d, np.inf), s.rows, s.cols, rng)


@pytest.mark.parametrize("mesh", ["m1", "m2", "m3"])
def test_the_finder_confirms_by_both_rules(gpu_lib, mesh):
    """The finder's default search on Appendix J's scenes: the found poses' records equal the twin's and a confirmed find
    is SUPPORTED and PRESENT.  Whether each find is confirmed is a measurement (printed), not asserted."""
    from dbot_ros_amd.finder import ObjectFinder
    s = asc.Scene((mesh,), 640, 480)
    with RbSensor(s.om, s.cam, s.P, max_particles=1) as sensor, ObjectFinder(sensor, s.om, ObjectFinder.Parameters()) as fnd:
        a = PoseAssessor(sensor, PARAMS, contour_params(2))
        for seed in (101, 102):
            truth, frame = _finder_scene(s, seed)
            r = fnd.find(frame, assess=a)
            plain = fnd.find(frame, assess=PoseAssessor(sensor, PARAMS))
            assert np.array_equal(r.poses, plain.poses) and np.array_equal(r.assessment.counts, plain.assessment.counts)
            t = a.assess(truth, frame)
            ct_, vt = cs.expect(s, truth[None], frame)
            assert np.array_equal(t.contour_counts[0], ct_) and np.array_equal(t.contour_verdicts[0], vt)
            print("FIND", mesh, seed, "truth", t.counts[0, 0].tolist(), VERDICTS[t.verdicts[0, 0]], t.contour_counts[0, 0].tolist(),
                  CONTOUR_VERDICTS[t.contour_verdicts[0, 0]], "confirmed", r.confirmed, "plain rule alone", plain.confirmed)
            K = len(r.poses)
            assert K >= 1 and r.assessment.contour_counts.shape == (K, 1, 5)
            for k in range(K):
                c, v = cs.expect(s, r.poses[k][None], frame)
                assert np.array_equal(r.assessment.contour_counts[k], c) and np.array_equal(r.assessment.contour_verdicts[k], v), k
                print("FIND", mesh, seed, "pose", k, "off by %.1f mm" % (1e3 * float(np.linalg.norm(r.poses[k, 9:] - truth[9:]))),
                      r.assessment.counts[k, 0].tolist(), VERDICTS[r.assessment.verdicts[k, 0]], r.assessment.contour_counts[k, 0].tolist(),
                      CONTOUR_VERDICTS[r.assessment.contour_verdicts[k, 0]])
            mask = r.assessment.confirmed_mask()
            assert r.confirmed == (int(np.nonzero(mask)[0][0]) if mask.any() else -1)
            if r.confirmed >= 0:
                assert r.assessment.verdicts[r.confirmed, 0] == SUPPORTED and r.assessment.contour_verdicts[r.confirmed, 0] == CONTOUR_PRESENT
    s.close()
