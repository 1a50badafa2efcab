"""The scene finder on the device (rbs_find_scene_*, dbot_ros_amd/finder.py SceneFinder): the residual
frame against the numpy twin bit for bit, every body's find against the single-object finder on the twin's residual frame,
the polish against the twin and the B-body sensor's own log-likelihoods, masks and refusals, explain-away on two copies of
one mesh, and that a scene find leaves the sensor and a tracker over it alone."""
import math

import numpy as np
import pytest

import find_twin as tw
import scene_find_scenes as ss
import scene_find_twin as st
from dbot_ros_amd import RbSensor, RbSensorBuilder, _capi, synth
from dbot_ros_amd.assess import PoseAssessor
from dbot_ros_amd.finder import ObjectFinder, SceneFinder
from dbot_ros_amd.pose import matrix_to_rotvec
from dbot_ros_amd.sensor import RbSensorError

pytestmark = pytest.mark.gpu

SMALL, TINY = ss.SMALL, ss.TINY
FG = ObjectFinder.Foreground(**ss.FOREGROUND)


def _params(**kw):
    p = ObjectFinder.Parameters()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def device_planes(assessor, poses):
    """The assess rule's planes of poses [B][12]: [B][npx] float32, +inf where a body covers nothing."""
    B = len(poses)
    assessor.assess(np.asarray(poses)[None])
    return np.stack([assessor.plane(0, b).ravel() for b in range(B)])


def twin_residual(s, planes, placed, frame, radius, sigmas=3.0):
    return st.residual(planes, placed, frame, s.rows, s.cols, s.ms, s.sf, sigmas, radius)


def assert_same_bits(got, want, what):
    g, w = bits(np.asarray(got).ravel()), bits(np.asarray(want).ravel())
    assert np.array_equal(g, w), (what, int((g != w).sum()), np.nonzero(g != w)[0][:8].tolist())


# ---------------------------------------------------------------- 1. the residual frame
def _residual_case(s, frame, poses, search, radius, what):
    """Body `search` searched, the others given at `poses`: the device's residual frame against the twin's."""
    with RbSensor(s.om, s.cam, s.P, max_particles=1) as sensor:
        a = PoseAssessor(sensor)
        with SceneFinder(sensor, s.om, _params(**TINY), SceneFinder.Parameters(explain_radius=radius, polish_sweeps=0)) as fnd:
            for poses_k, frame_k, tag in zip(poses, frame, what):
                r = fnd.find(frame_k, search=[search], given_poses=poses_k)
                placed = [b for b in range(s.B) if b != search]
                planes = device_planes(a, poses_k)
                want = twin_residual(s, planes, placed, frame_k, radius)
                assert_same_bits(fnd.residual(search), want, (tag, radius))
                for b in placed:
                    assert np.array_equal(r.poses[b], poses_k[b]), tag        # given bodies come back bit for bit
                yield tag, want, frame_k


@pytest.mark.parametrize("cols, rows", [(160, 120), (161, 121)])
@pytest.mark.parametrize("radius", [0, 2, 8])
def test_residual_equals_the_twin_with_one_placed_body(gpu_lib, cols, rows, radius):
    s = ss.Scene(("m1", "m2"), cols, rows, 3)
    T = s.truth
    over_border = T.copy()
    over_border[0, 9] = (0.0 - s.K[0, 2]) / s.K[0, 0] * T[0, 11]                 # body 0's centre on the left border
    off_screen = T.copy()
    off_screen[0, 9] = -5.0
    behind = T.copy()
    behind[0, 11] = -0.7
    close = T.copy()
    close[0, 9:] = [0.0, 0.0, 0.11]                                              # 11 cm from the camera: it fills the image
    near_frame = synth.make_frame(np.where(np.isfinite(s.plane(0, close[0])), s.plane(0, close[0]), np.inf), rows, cols,
                                  np.random.default_rng(5), occluder=False)
    all_nan = np.full(rows * cols, np.nan, dtype=np.float32)
    cases = [("truth", T, s.frame), ("over the border", over_border, s.frame), ("off screen", off_screen, s.frame),
             ("behind the camera", behind, s.frame), ("all-NaN frame", T, all_nan), ("11 cm", close, near_frame)]
    seen = {}
    for tag, want, frame in _residual_case(s, [c[2] for c in cases], [c[1] for c in cases], 1, radius, [c[0] for c in cases]):
        seen[tag] = int((bits(want) != bits(frame)).sum())
    print(cols, rows, radius, seen)
    assert seen["truth"] > 0 and seen["11 cm"] > seen["truth"]
    assert seen["off screen"] == seen["behind the camera"] == seen["all-NaN frame"] == 0


@pytest.mark.parametrize("radius", [0, 2, 8])
def test_residual_equals_the_twin_with_two_placed_bodies(gpu_lib, radius):
    s = ss.Scene(("m1", "m2", "m3"), 322, 241, 4)
    T = s.truth
    overlap = T.copy()
    overlap[1, 9:] = T[0, 9:] + [0.02, 0.0, 0.05]                                # body 1 behind body 0 on screen
    depth = np.minimum(s.plane(0, overlap[0]), s.plane(1, overlap[1]))
    overlap_frame = synth.make_frame(depth, s.rows, s.cols, np.random.default_rng(6), occluder=False)
    cases = [("truth", T, s.frame), ("overlapping", overlap, overlap_frame)]
    seen = {}
    for tag, want, frame in _residual_case(s, [c[2] for c in cases], [c[1] for c in cases], 2, radius, [c[0] for c in cases]):
        seen[tag] = int((bits(want) != bits(frame)).sum())
    print(radius, seen)
    assert seen["truth"] > 0 and seen["overlapping"] > 0


# ---------------------------------------------------------------- 2. a body's find is the single-object finder's
def _assert_same_find(body, ref, p, fg, rf, what):
    for stage in ("seeds", "coarse", "candidates", "survivors", "result"):
        for got, want in zip(body.stage(stage), ref.stage(stage)):
            np.testing.assert_array_equal(got, want, err_msg=f"{what} {stage}")
    for r in range(p.rounds):
        for got, want in zip(body.stage("children", r), ref.stage("children", r)):
            np.testing.assert_array_equal(got, want, err_msg=f"{what} children {r}")
    if fg:
        assert body.plane() == ref.plane(), what
        assert_same_bits(body.seed_frame(), ref.seed_frame(), what)
    if rf:
        for r in range(p.rounds + 1):
            np.testing.assert_array_equal(body.covariance(r), ref.covariance(r), err_msg=f"{what} covariance {r}")
        for r in range(p.rounds):
            np.testing.assert_array_equal(body.perturbations(r), ref.perturbations(r), err_msg=f"{what} perturbations {r}")


@pytest.mark.parametrize("variant", ["fixed", "foreground", "refinement"])
def test_a_bodys_find_is_the_single_object_finders(gpu_lib, variant):
    s = ss.Scene(("m1", "m2"), 160, 120, 3)
    p = _params(**SMALL, seed=11)
    fg = FG if variant == "foreground" else None
    rf = ObjectFinder.Refinement() if variant == "refinement" else None
    with RbSensor(s.om, s.cam, s.P, max_particles=1) as sensor:
        a = PoseAssessor(sensor)
        with SceneFinder(sensor, s.om, p, foreground=fg, refinement=rf) as fnd:
            res = fnd.find(s.frame)
            order, e = fnd.order()
            assert order == st.order(s.e, 3) and e.tolist() == s.e
            placed, X = [], np.tile(np.array([1.0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 1]), (s.B, 1))
            for b in order:
                planes = device_planes(a, X)
                want = twin_residual(s, planes, placed, s.frame, 2)
                assert_same_bits(fnd.residual(b), want, (variant, b))
                body = fnd.body_finder(b)
                om1 = s.part_model(b)
                with RbSensor(om1, s.cam, s.P, max_particles=1) as one, ObjectFinder(one, om1, p, foreground=fg, refinement=rf) as ref:
                    r1 = ref.find(want)
                    _assert_same_find(body, ref, p, fg, rf, (variant, b))
                    assert len(r1.poses) > 0 and r1.found == bool(res.found[b])
                    assert res.scores[b] == r1.scores[0]
                X[b] = r1.poses[0]                                   # the body's pose as the next residual saw it (before the polish)
                if r1.found:
                    placed.append(b)
            assert len(placed) == 2 and (bits(fnd.residual(order[1]).ravel()) != bits(s.frame)).any()


# ---------------------------------------------------------------- 3. one body
def test_one_body_without_polish_is_rbs_find_run(gpu_lib):
    s = ss.Scene(("m2",), 160, 120, 5)
    p = _params(**SMALL, seed=2)
    with RbSensor(s.om, s.cam, s.P, max_particles=1) as sensor:
        with ObjectFinder(sensor, s.om, p) as one, SceneFinder(sensor, s.om, p, SceneFinder.Parameters(polish_sweeps=0)) as fnd:
            want = one.find(s.frame)
            got = fnd.find(s.frame)
            np.testing.assert_array_equal(got.poses[0], want.poses[0])
            assert got.scores[0] == want.scores[0] and bool(got.found[0]) == want.found
            assert got.joint_score == want.scores[0]                 # the same pose under the same likelihood, scored once
            np.testing.assert_array_equal(got.states[0], want.states[0])
            assert_same_bits(fnd.residual(0), s.frame, "one body")
            ch, cs, best = fnd.polish(0)
            assert ch.shape == (1, 1, 12) and best == 0 and cs[0] == got.joint_score


# ---------------------------------------------------------------- 4. the polish
def _joint_reference(s, frame, poses, occlusion):
    poses = np.asarray(poses).reshape(len(poses), -1)
    n = len(poses)
    m = max(n, 1024)
    padded = np.concatenate([poses, np.repeat(poses[-1:], m - n, 0)])
    with RbSensor(s.om, s.cam, s.P, max_particles=m, occlusion=occlusion) as ref:
        ref.reset()
        ref.set_observation(np.asarray(frame, dtype=np.float32).ravel())
        return ref.loglikes_poses(padded.reshape(m, s.B, 12), np.zeros(m, dtype=np.int32), update=False)[:n]


@pytest.mark.parametrize("occlusion", ["device", "reference"])
def test_polish_rounds_match_the_twin_and_the_sensors_loglikes(gpu_lib, occlusion):
    s = ss.Scene(("m1", "m2"), 160, 120, 3)
    p = _params(**SMALL, seed=11)
    sp = SceneFinder.Parameters(polish_children=32)
    spd = dict(polish_sigma_translation=sp.polish_sigma_translation, polish_sigma_angle=sp.polish_sigma_angle, polish_decay=sp.polish_decay)
    with RbSensor(s.om, s.cam, s.P, max_particles=1, occlusion=occlusion) as sensor, SceneFinder(sensor, s.om, p, sp) as fnd:
        res = fnd.find(s.frame)
        order, _ = fnd.order()
        X = np.stack([fnd.body_finder(b).stage("result")[0][0] for b in range(s.B)])
        prev, rounds = -np.inf, sp.polish_sweeps * len(order)
        all_children = []
        for r in range(rounds):
            ch, cs, best = fnd.polish(r)
            c = order[r % len(order)]
            st_r, sa_r = st.polish_scales(spd, len(order), r)
            np.testing.assert_allclose(ch, st.polish_children(X, c, sp.polish_children, r, p.seed, st_r, sa_r), rtol=0, atol=1e-14)
            np.testing.assert_array_equal(ch[0], X)                  # child 0 is X, bit for bit
            others = [b for b in range(s.B) if b != c]
            np.testing.assert_array_equal(ch[:, others], np.repeat(X[None, others], len(ch), 0))
            assert best == int(tw.best_child(cs[None])[0])
            assert cs[best] >= prev
            prev, X = cs[best], ch[best]
            all_children.append((ch, cs))
        np.testing.assert_array_equal(res.poses, X)
        assert res.joint_score == prev
        ref = _joint_reference(s, s.frame, np.concatenate([c for c, _ in all_children]), occlusion)
        np.testing.assert_array_equal(np.concatenate([c for _, c in all_children]), ref)
        with pytest.raises(RbSensorError):
            fnd.polish(rounds)
        # a body without a pose (no seed on an all-NaN frame): no polish, and the joint score is NaN
        none = fnd.find(np.full(s.rows * s.cols, np.nan, dtype=np.float32))
        assert math.isnan(none.joint_score) and not none.found.any() and np.isnan(none.poses).all() and np.isnan(none.scores).all()
        with pytest.raises(RbSensorError):
            fnd.polish(0)


# ---------------------------------------------------------------- 5. masks and refusals
def test_every_search_mask_and_the_refusals(gpu_lib):
    s = ss.Scene(("m1", "m2", "m3"), 160, 120, 7)
    p = _params(**TINY)
    lib = _capi.load()
    with RbSensor(s.om, s.cam, s.P, max_particles=1) as sensor, SceneFinder(sensor, s.om, p) as fnd:
        results = {}
        for mask in range(1, 8):
            r = fnd.find(s.frame, search=mask, given_poses=s.truth)
            order, e = fnd.order()
            assert order == st.order(s.e, mask) and e.tolist() == s.e, mask
            for b in range(3):
                if mask >> b & 1:
                    assert np.isfinite(r.poses[b]).all() and np.isfinite(r.scores[b])
                else:
                    assert np.array_equal(r.poses[b], s.truth[b]) and math.isnan(r.scores[b]) and r.found[b]
                    with pytest.raises(RbSensorError):
                        fnd.residual(b)
            assert r.searched.tolist() == [bool(mask >> b & 1) for b in range(3)] and math.isfinite(r.joint_score)
            results[mask] = r
        all_again = fnd.find(s.frame)                                 # search=None: every body, no poses given
        np.testing.assert_array_equal(all_again.poses, results[7].poses)
        last = fnd.find(s.frame, search=[0, 2], given_poses=s.truth)
        # refusals: the previous find's state stays, and a good call after a bad one is unaffected
        bad_pose = s.truth.copy()
        bad_pose[1, 4] = np.inf
        for kw, text in ((dict(search=0), "search_mask"), (dict(search=8), "search_mask"), (dict(search=[0, 3]), "search_mask"),
                         (dict(search=[0, 2]), "given_poses is NULL"), (dict(search=[0, 2], given_poses=bad_pose), "not finite")):
            with pytest.raises(RbSensorError) as err:
                fnd.find(s.frame, **kw)
            assert err.value.code == _capi.RBS_ERR_INVALID_ARGUMENT and text in str(err.value), kw
            assert fnd.order()[0] == st.order(s.e, 0b101)
        found, joint = _capi.C.c_uint32(), _capi.C.c_double()
        assert lib.rbs_find_scene_run(fnd._f, None, 7, None, None, None, None, _capi.C.byref(joint)) == _capi.RBS_ERR_INVALID_ARGUMENT
        again = fnd.find(s.frame, search=[0, 2], given_poses=s.truth)
        np.testing.assert_array_equal(again.poses, last.poses)
        np.testing.assert_array_equal(again.scores, last.scores)
        assert again.joint_score == last.joint_score
        with pytest.raises(RbSensorError):
            fnd.set_refinement(ObjectFinder.Refinement(elite=1000))
        with pytest.raises(RbSensorError):
            fnd.set_foreground(ObjectFinder.Foreground(plane_trials=0))
        with pytest.raises(ValueError):
            fnd.body_finder(3)
    with RbSensor(s.om, s.cam, s.P, max_particles=1) as sensor:
        with pytest.raises(RbSensorError) as err:
            SceneFinder(sensor, s.om, p, SceneFinder.Parameters(explain_radius=9))
        assert "explain_radius outside 0..8" in str(err.value)
        with pytest.raises(RbSensorError) as err:                     # the one-object finder keeps its refusal
            ObjectFinder(sensor, s.om, p)
        assert err.value.code == _capi.RBS_ERR_UNSUPPORTED and "one object" in str(err.value)


def test_a_multi_device_handle_is_refused(gpu_lib, monkeypatch):
    monkeypatch.setenv("RBS_GROUP_SINGLE", "1")
    s = ss.Scene(("m1", "m2"), 160, 120, 3)
    with RbSensor(s.om, s.cam, s.P, max_particles=2, device_ids=[0]) as g:
        with pytest.raises(RbSensorError) as e:
            SceneFinder(g, s.om)
        assert e.value.code == _capi.RBS_ERR_UNSUPPORTED and "single-device" in str(e.value)


# ---------------------------------------------------------------- 6. explain-away
def test_two_copies_of_one_mesh_land_on_their_own_blobs(gpu_lib):
    """ss.explain_away_scene(): two copies of m1, 33 cm apart.  The twin run on the CPU (tests/test_scene_find_cpu.py) places
    them 5.0 mm and 1.5 mm from one copy each.  The contrast, also from the twin: with explain_sigmas = 1e-9 nothing is
    explained and both bodies land on the same blob, 5 mm from each other (the second find repeats the first)."""
    s, kw = ss.explain_away_scene()
    p = _params(**kw["find"], seed=kw["seed"])
    with RbSensor(s.om, s.cam, s.P, max_particles=1) as sensor, SceneFinder(sensor, s.om, p, foreground=FG) as fnd:
        r = fnd.find(s.frame)
        d = ss.distances_to_copies(r.poses, s.truth)
        apart = float(np.linalg.norm(r.poses[0, 9:] - r.poses[1, 9:]))
        print("explain-away: distances to the copies (m)", d.tolist(), "apart", apart, "twin", ss.EXPLAIN_AWAY_TWIN_DISTANCES)
        assert r.found.all() and apart > p.nms_translation
        assert sorted(int(np.argmin(row)) for row in d) == [0, 1]
        # within the distance the twin finds for it; 1e-6: the constants above are rounded to that
        for b in range(2):
            assert d[b].min() <= ss.EXPLAIN_AWAY_TWIN_DISTANCES[b] + 1e-6, (b, d[b].min())
    with RbSensor(s.om, s.cam, s.P, max_particles=1) as sensor:
        with SceneFinder(sensor, s.om, p, SceneFinder.Parameters(explain_sigmas=1e-9), foreground=FG) as fnd:
            r0 = fnd.find(s.frame)
            assert float(np.linalg.norm(r0.poses[0, 9:] - r0.poses[1, 9:])) < p.nms_translation
            assert r0.joint_score < r.joint_score


# ---------------------------------------------------------------- 7. non-interference and determinism
def _state(om, poses):
    out = np.zeros((len(poses), 12))
    for b, P in enumerate(poses):
        R = P[:9].reshape(3, 3)
        out[b, 0:3] = P[9:] - R @ om.centers[b]
        out[b, 3:6] = matrix_to_rotvec(R)
    return out.ravel()


def test_a_scene_find_leaves_a_tracker_alone_and_repeats_itself(gpu_lib):
    from dbot_ros_amd.tracker import DeviceParticleTracker, ObjectTransitionBuilder, ParticleTrackerBuilder
    s = ss.Scene(("m1", "m2"), 80, 60, 3)
    rng = np.random.default_rng(4)
    truths = [synth.truth_pose(2, z=0.7, frame=k) for k in range(6)]
    orc = s.oracle()
    frames = [synth.make_frame(orc.render_depth(t), s.rows, s.cols, rng) for t in truths]
    p = _params(**TINY)

    def run(find, look_ahead):
        sensor = RbSensor(s.om, s.cam, RbSensorBuilder.Parameters(sample_count=200), max_particles=200)
        tr = DeviceParticleTracker(ObjectTransitionBuilder(ObjectTransitionBuilder.Parameters(
            0.002, 0.002, 0.002, 0.01, 0.01, 0.01, 0.8, 2)).build(), sensor, s.om, ParticleTrackerBuilder.Parameters(evaluation_count=200),
            device_rng=True, seed=3)
        fnd = SceneFinder(sensor, s.om, p) if find else None
        tr.initialize([_state(s.om, truths[0])])
        ests, finds = [], []
        if look_ahead:
            tr.submit(frames[0])
            for k in range(1, len(frames)):
                tr.submit(frames[k])
                ests.append(tr.result())
                if find:
                    finds.append(fnd.find(frames[k - 1]))
            ests.append(tr.result())
        else:
            for fr in frames:
                ests.append(tr.track(fr))
                if find:
                    given = fnd.find(fr)
                    held = fnd.find()                               # frame=None: the sensor's observation IS this frame
                    np.testing.assert_array_equal(given.poses, held.poses)
                    assert given.joint_score == held.joint_score
                    finds.append(given)
        if fnd is not None:
            fnd.close()
        tr.close()
        sensor.close()
        return np.array(ests), finds

    for la in (False, True):
        base, _ = run(False, la)
        got, finds = run(True, la)
        assert np.array_equal(got, base), la
        again, finds2 = run(True, la)
        for a, b in zip(finds, finds2):                              # two runs: the same bits
            np.testing.assert_array_equal(a.poses, b.poses)
            np.testing.assert_array_equal(a.scores, b.scores)
            assert a.joint_score == b.joint_score


# ---------------------------------------------------------------- 8. hand-off
def test_replay_of_a_two_object_dataset_found_on_frame_0(tmp_path, gpu_lib):
    from dbot_ros_amd import CameraData, ObjectModel, node, objloader
    from dbot_ros_amd import dataset as ds
    from test_node import _write
    paths = _write(tmp_path)
    v, t = synth.mesh_m2()
    objloader.write_obj(tmp_path / "object_models" / "part2.obj", v, t)
    tree = node.load_rosparams(*paths)
    tree["object"]["meshes"] = ["part.obj", "part2.obj"]
    tree["object_finder"] = dict(SMALL, scene=dict(polish_children=16))
    K = synth.camera_matrix(640, 480)
    vs, ts = objloader.SimpleWavefrontObjectModelLoader(
        objloader.ObjectResourceIdentifier(str(tmp_path), "object_models", ["part.obj", "part2.obj"])).load()
    om = ObjectModel(vs, ts, center=True)
    rng = np.random.default_rng(0)
    rec = ds.TrackingDataset(tmp_path / "recording", load=False)
    with RbSensor(om, CameraData(K, 480, 640), RbSensorBuilder.Parameters(sample_count=1), max_particles=1) as full:
        for k in range(1, 5):
            native = synth.make_frame(full.render_depth(synth.truth_pose(2, frame=k)), 480, 640, rng, occluder=False)
            stamp = ds.Stamp.from_sec(1500000000.0 + k / 30.0)
            rec.add_frame(ds.Image(native.reshape(480, 640), stamp, seq=k), ds.CameraInfo(K, 480, 640, stamp, seq=k),
                          ground_truth=_state(om, synth.truth_pose(2, frame=k)))
    rec.store()
    data = ds.TrackingDataset(tmp_path / "recording")
    ests, wall = node.replay_dataset(tree, data, str(tmp_path), None, seed=3)
    assert ests.shape == (4, 24) and np.isfinite(ests).all() and wall > 0
    finder, _, _ = node.build_scene_finder(tree, data.get_camera_matrix(0), str(tmp_path))
    try:
        assert isinstance(finder, SceneFinder) and finder.parts == 2 and finder.scene.polish_children == 16
        assert finder.params.n_rotations == SMALL["n_rotations"]
    finally:
        finder.close()
        finder.sensor.close()


def test_supervisor_refinds_the_one_body_that_jumped(gpu_lib):
    """The loop, not the search: find_bodies answers with the truth for the bodies it is asked for (as the existing supervisor
    test stubs its finder) and with the estimate's poses for the others."""
    from dbot_ros_amd.supervisor import TrackSupervisor
    from dbot_ros_amd.tracker import DeviceParticleTracker, ObjectTransitionBuilder, ParticleTrackerBuilder
    s = ss.Scene(("m1", "m2"), 80, 60, 3)
    rng = np.random.default_rng(6)
    n_frames, jump_at = 14, 4
    truths = []
    for k in range(n_frames):
        t = synth.truth_pose(2, z=0.7, frame=k)
        if k >= jump_at:
            t[1, 9] += 0.10                                           # body 1 jumps 10 cm, away from body 0, between two frames
        truths.append(t)
    orc = s.oracle()
    frames = [synth.make_frame(orc.render_depth(t), s.rows, s.cols, rng, occluder=False) for t in truths]
    states = [_state(s.om, t) for t in truths]
    index = {fr.tobytes(): k for k, fr in enumerate(frames)}
    asked = []

    def find_bodies(frame, lost, estimate):
        k = index[np.asarray(frame).tobytes()]
        asked.append((k, lost.tolist()))
        out = np.asarray(estimate, dtype=np.float64).reshape(2, 12).copy()
        out[lost] = states[k].reshape(2, 12)[lost]
        return out.ravel()

    with RbSensor(s.om, s.cam, RbSensorBuilder.Parameters(sample_count=400), max_particles=400) as sensor:
        tr = DeviceParticleTracker(ObjectTransitionBuilder(ObjectTransitionBuilder.Parameters(
            0.002, 0.002, 0.002, 0.01, 0.01, 0.01, 0.8, 2)).build(), sensor, s.om, ParticleTrackerBuilder.Parameters(evaluation_count=400),
            device_rng=True, seed=3)
        sup = TrackSupervisor(tr, PoseAssessor(sensor), find_bodies=find_bodies, lost_frames=3)
        tr.initialize([states[0]])
        events, errs = [], []
        for k, fr in enumerate(frames):
            est, verdicts, ev = sup.step(fr)
            events.append(ev)
            errs.append([float(np.linalg.norm(est[12 * b:12 * b + 3] - states[k][12 * b:12 * b + 3])) for b in range(2)])
            print(k, ev, verdicts.tolist(), np.round(errs[-1], 4).tolist())
        tr.close()
    assert [e for e in events if e is not None] == ["lost", "reacquired"], events
    assert asked == [(events.index("reacquired"), [False, True])], asked          # body 1 alone was searched, once
    at = events.index("reacquired")
    assert errs[jump_at][1] > 0.08 and max(e[1] for e in errs[at:]) < 0.025 and max(e[0] for e in errs) < 0.025, errs


# ---------------------------------------------------------------- 9. accuracy, recorded
def _iou(a, b):
    a, b = np.isfinite(a), np.isfinite(b)
    return (a & b).sum() / max((a | b).sum(), 1)


# Measured on one MI355X with the settings below, and NOT met: of the ten bodies of the four scenes two
# are found (M1 of m1+m2+m3 seed 1: 0.24 mm, IoU 0.995; M2 of seed 2: 0.23 mm, IoU 0.992); the other eight lie 0.18-0.49 m
# from their truth at IoU 0-0.36 -- m1+m2 seed 1: 429 / 196 mm, seed 2: 486 / 179 mm; m1+m2+m3 seed 1: M2 237 mm, M3 337 mm,
# seed 2: M1 482 mm, M3 341 mm -- while every joint score is ABOVE the truth's (41 424 against 9 792, 43 621 against 6 427,
# 67 090 against 30 520, 66 530 against 26 554): the poses found lie in the flat surfaces of the scene (synth.make_frame's
# occluding slab spans a quarter of the whole group of bodies here, and the wall), which the likelihood prices above a
# half-hidden body.  The bar stays as stated; this test records it.
@pytest.mark.xfail(reason="accuracy bar not met on the multi-object scenes (measured values above)", strict=True)
@pytest.mark.parametrize("names, seed", [(("m1", "m2"), 1), (("m1", "m2"), 2), (("m1", "m2", "m3"), 1), (("m1", "m2", "m3"), 2)])
def test_accuracy_on_synthetic_scenes(gpu_lib, names, seed):
    """The settings for which all six single-object scenes meet the bar: the foreground on, seed_stride 4, the adaptive
    refinement from sigma (25 degrees, 1.5 cm), 16 rounds.  The bar is tests/test_gpu_finder.py's, per body, and the joint
    score within 2 % of the truth's."""
    s = ss.Scene(names, 640, 480, 100 + seed)
    p = _params(seed_stride=4, sigma_angle=math.radians(25.0), sigma_translation=0.015, rounds=16)
    with RbSensor(s.om, s.cam, s.P, max_particles=1) as sensor:
        with SceneFinder(sensor, s.om, p, foreground=ObjectFinder.Foreground(), refinement=ObjectFinder.Refinement()) as fnd:
            r = fnd.find(s.frame)
            ms = fnd.stage_ms()
        a = PoseAssessor(sensor)
        got_planes = device_planes(a, np.where(np.isfinite(r.poses), r.poses, s.truth)).reshape(s.B, -1)
        true_planes = device_planes(a, s.truth).reshape(s.B, -1)
    s_truth = _joint_reference(s, s.frame, s.truth[None], None)[0]
    dts = [float(np.linalg.norm(r.poses[b, 9:] - s.truth[b, 9:])) for b in range(s.B)]
    ious = [float(_iou(got_planes[b], true_planes[b])) for b in range(s.B)]
    print(f"{'+'.join(names)} seed {seed}: |dt| mm {[round(1e3 * d, 2) for d in dts]}, IoU {[round(i, 3) for i in ious]}, "
          f"joint {r.joint_score:.1f} vs truth {s_truth:.1f}, found {r.found.tolist()}, per body ms {[round(m, 2) for m in ms[0]]}, "
          f"render {ms[1]:.3f} residual {ms[2]:.3f} polish {ms[3]:.2f} whole {ms[4]:.2f} ms")
    assert r.found.all()
    assert all(d < 0.01 for d in dts) and all(i >= 0.85 for i in ious), (dts, ious)
    assert r.joint_score >= s_truth - 0.02 * abs(s_truth), (r.joint_score, s_truth)
