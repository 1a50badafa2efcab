"""The pose refiner on the device (rbs_refine_*, dbot_ros_amd/refine.py; the rule: include/rbsensor_mi355x.h, DESIGN.md
Appendix Q) against the numpy twin (tests/refine_twin.py) over the oracle's per-body renders.

Per iteration, from the device's own history (the pose that entered it): the count exactly, every one of the 28 sums
within the first-order bar E of the np.longdouble sum, the delta recomputed from the device's sums bit for bit, the next
translation bit for bit and the next rotation within R_ULPS units in the last place of 1.  Then the four statuses, the
border and occlusion cases, the end-to-end error against the twin's chain, determinism, isolation and the callers."""
import numpy as np
import pytest

import assess_scenes as asc
import refine_twin as rt
from dbot_ros_amd import CameraData, ObjectModel, RbSensor, RbSensorBuilder, _capi, synth
from dbot_ros_amd.assess import PoseAssessor
from dbot_ros_amd.refine import CONVERGED, DEGENERATE, FROZEN, MAX_ITERATIONS, TOO_FEW_PIXELS, PoseRefiner
from dbot_ros_amd.sensor import RbSensorError

pytestmark = pytest.mark.gpu

# R <- R(omega) R differs from the twin's only through sin and cos: the device's are its math library's (within 4 units in the
# last place by OpenCL's bound for them), the twin's libm's (within 1): the quaternion's w and k differ by at most 5 eps
# relative (eps = 2^-52), a product of two of its entries by 10 eps, an entry of R(omega) -- 2 (xy -+ wz) or 1 - 2 (yy + zz),
# with |xy| + |wz| <= 1 -- by 20 eps plus 3 roundings, and a row of matmul3 against a column of R (length 1, so sum |R_i| <=
# sqrt 3) by 23 sqrt(3) + 3 < 43 eps.
R_ULPS = 43
EPS = 2.0 ** -52
START = ((0.005, -0.005, 0.005), 5.0)      # the issue's first start: (5, -5, 5) mm and 5 degrees about (1, 1, 1)


def cam_of(s):
    K = s.cam.camera_matrix
    return (K[0, 0], K[1, 1], K[0, 2], K[1, 2])


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def rigs():
    """name -> (Scene, sensor): shared, read-only."""
    out = {}
    for name in ("m1_80", "m1m2_161", "m1m2m3_322"):
        meshes, cols, rows = asc.SCENES[name]
        s = asc.Scene(meshes, cols, rows)
        out[name] = (s, RbSensor(s.om, s.cam, s.P, max_particles=1))
    yield out
    for s, sensor in out.values():
        sensor.close()
        s.close()


def hold_call_to_the_twin(s, ref, poses_in, frame, poses_out, rec):
    """Every iteration of the last call of `ref` against the twin; -> the worst |device - exact| / E seen."""
    p = {f: getattr(ref.params, f) for f in rt.DEFAULTS}
    n, B, iters = poses_in.shape[0], s.B, int(ref.params.iters)
    worst = 0.0
    for k in range(n):
        hist = [[ref.history(k, b, it) for b in range(B)] for it in range(iters)]
        assert np.array_equal(bits(np.stack([h.pose for h in hist[0]])), bits(poses_in[k]))
        frozen = [False] * B
        last = [None] * B
        for it in range(iters):
            entered = np.stack([h.pose for h in hist[it]])
            nxt = np.stack([h.pose for h in hist[it + 1]]) if it + 1 < iters else poses_out[k]
            planes = s.planes(entered)
            for b in range(B):
                h = hist[it][b]
                if frozen[b]:
                    assert h.status == FROZEN and h.count == 0 and not h.sums.any() and not h.delta.any(), (k, b, it)
                    assert np.array_equal(bits(nxt[b]), bits(entered[b])), (k, b, it)
                    continue
                _, T, _ = rt.terms(planes, frame, entered[b][9:12], b, cam_of(s), s.ms, s.sf, s.rows, s.cols, **p)
                exact, E, N = rt.exact_sums(T)
                assert h.count == N, (k, b, it, h.count, N)
                err = np.abs(h.sums.astype(rt.LD) - exact)
                assert (err <= E).all(), (k, b, it, [float(v) for v in err / np.maximum(E, rt.LD(1e-300))])
                if N:
                    worst = max(worst, float((err[E > 0] / E[E > 0]).max()))
                status, delta = rt.solve(h.sums, h.count, **p)
                assert h.status == status, (k, b, it, h.status, status)
                assert np.array_equal(bits(h.delta), bits(delta)), (k, b, it, h.delta.tolist(), delta)
                if status in (MAX_ITERATIONS, CONVERGED):
                    want = rt.apply(entered[b], delta)
                    assert np.array_equal(bits(nxt[b][9:12]), bits(want[9:12])), (k, b, it)
                    assert np.abs(nxt[b][:9] - want[:9]).max() <= R_ULPS * EPS, (k, b, it, float(np.abs(nxt[b][:9] - want[:9]).max() / EPS))
                else:
                    assert np.array_equal(bits(nxt[b]), bits(entered[b])), (k, b, it)
                frozen[b] = status in (CONVERGED, DEGENERATE)
                last[b] = (it, status, N, h.sums[27])
        for b in range(B):
            it, status, N, q = last[b]
            assert (rec.status[k, b], rec.iterations[k, b], rec.counts[k, b, 1]) == (status, it + 1, N), (k, b)
            assert rec.counts[k, b, 0] == hist[0][b].count
            assert rec.rms[k, b, 1] == (np.sqrt(q / N) if N else 0.0)
    return worst


@pytest.mark.parametrize("name", ["m1m2_161", "m1m2m3_322"])
def test_every_iteration_equals_the_twin(gpu_lib, rigs, name):
    """Worst |device - exact| / E per scene: DESIGN.md Appendix Q records the printed figures."""
    s, sensor = rigs[name]
    ref = PoseRefiner(sensor)
    poses = np.stack([rt.offset_pose(s.truth, *START), rt.offset_pose(s.truth, (0.01, 0.01, -0.01), 10.0)])
    out, rec = ref.refine(poses, s.frame)
    worst = hold_call_to_the_twin(s, ref, poses, s.frame, out, rec)
    print(name, "worst |device - exact| / E =", worst, "statuses", rec.status.tolist(), "iterations", rec.iterations.tolist(),
          "counts", rec.counts.tolist())
    assert worst <= 1.0
    assert (rec.counts[:, :2, 1] > 16).all()


def test_all_four_statuses_are_reached(gpu_lib, rigs):
    s, sensor = rigs["m1m2m3_322"]
    start = rt.offset_pose(s.truth, *START)[None]
    out, rec = PoseRefiner(sensor).refine(start, s.frame)
    assert rec.status[0].tolist() == [CONVERGED, CONVERGED, TOO_FEW_PIXELS], rec           # the slab covers the third body
    assert rec.iterations[0, 2] == 10 and rec.counts[0, 2].max() < 16 and np.array_equal(bits(out[0, 2]), bits(start[0, 2]))
    assert (rec.iterations[0, :2] < 10).all()
    one = PoseRefiner(sensor, PoseRefiner.Parameters(iters=1))
    out1, rec1 = one.refine(start, s.frame)
    assert rec1.status[0].tolist() == [MAX_ITERATIONS, MAX_ITERATIONS, TOO_FEW_PIXELS] and (rec1.iterations == 1).all()
    assert not np.array_equal(bits(out1[0, 0]), bits(start[0, 0])) and not np.array_equal(bits(out1[0, 1]), bits(start[0, 1]))
    # m1_80: the twin sees 18-24 usable pixels there over its iterations: min_pixels = 64 is out of their reach, 8 within it
    s80, sensor80 = rigs["m1_80"]
    p80 = rt.offset_pose(s80.truth, *START)[None]
    few = PoseRefiner(sensor80, PoseRefiner.Parameters(min_pixels=64, iters=2))
    o80, r80 = few.refine(p80, s80.frame)
    assert r80.status[0, 0] == TOO_FEW_PIXELS and 8 < r80.counts[0, 0, 0] < 64 and np.array_equal(bits(o80), bits(p80))
    hold_call_to_the_twin(s80, few, p80, s80.frame, o80, r80)
    some = PoseRefiner(sensor80, PoseRefiner.Parameters(min_pixels=8, iters=2))
    o80, r80 = some.refine(p80, s80.frame)
    assert r80.status[0, 0] == MAX_ITERATIONS and not np.array_equal(bits(o80), bits(p80))
    hold_call_to_the_twin(s80, some, p80, s80.frame, o80, r80)


def test_a_triangle_facing_the_camera_is_degenerate(gpu_lib):
    """One triangle in a plane of constant depth: every normal is (0, 0, -1) exactly, J = (-q1, q0, 0, 0, 0, -1), so
    H_22 = 0 and the third pivot is 0 exactly (the condition is asserted on the twin first).  damping = 0 and the
    default damping alike: damping x 0 = 0."""
    cols, rows = 80, 60
    v = np.array([[-0.06, -0.05, 0.0], [0.07, -0.04, 0.0], [0.0, 0.06, 0.0]])
    om = ObjectModel([v], [np.array([[0, 1, 2]], dtype=np.int32)], center=True)
    cam = CameraData(synth.camera_matrix(cols, rows), rows, cols)
    P = RbSensorBuilder.Parameters(sample_count=1)
    pose = np.concatenate([np.eye(3).ravel(), [0.0, 0.0, 0.75]])[None, None]
    K = cam.camera_matrix
    with RbSensor(om, cam, P, max_particles=1) as sensor:
        d = sensor.render_depth(pose[0])
        fin = np.isfinite(d)
        assert fin.sum() > 40 and (d[fin] == np.float32(0.75)).all()
        frame = np.where(fin, d + np.float32(0.002), np.float32(1.5)).astype(np.float32)
        _, T, _ = rt.terms(d[None], frame, pose[0, 0, 9:], 0, (K[0, 0], K[1, 1], K[0, 2], K[1, 2]), P.kinect.model_sigma,
                           P.kinect.sigma_factor, rows, cols)
        exact, _, N = rt.exact_sums(T)
        assert N >= 16 and exact[11] == 0 and rt.solve(exact.astype(np.float64), N, damping=0.0)[0] == DEGENERATE   # the twin first
        for damping in (0.0, 1e-3):
            ref = PoseRefiner(sensor, PoseRefiner.Parameters(damping=damping, iters=3))
            out, rec = ref.refine(pose, frame)
            assert rec.status[0, 0] == DEGENERATE and rec.iterations[0, 0] == 1 and rec.counts[0, 0, 0] == N, (damping, rec)
            assert np.array_equal(bits(out), bits(pose))
            h = [ref.history(0, 0, it) for it in range(3)]
            assert h[0].status == DEGENERATE and h[0].sums[11] == 0.0 and not h[0].delta.any()
            assert h[1].status == FROZEN and h[2].status == FROZEN


def test_border_and_occlusion_counts_equal_the_twin(gpu_lib, rigs):
    """Poses at the image border (the skipped border, rectangles cut by the image; both bodies at one place: the owner rule
    with its ties) and a body half behind another (the owner and the neighbour rule), each against a frame that shows the
    pose itself 1 mm further away -- the scene's own frame shows the truth, which the gate rejects there: two iterations
    each, every count exact."""
    s, sensor = rigs["m1m2_161"]
    poses = s.poses()
    ref = PoseRefiner(sensor, PoseRefiner.Parameters(iters=2))
    counts = {}
    for name in ("left border", "right border", "top border", "bottom border", "corner", "half behind", "off screen", "fills the image"):
        planes = s.planes(poses[name])
        d = planes.min(axis=0)
        frame = np.where(np.isfinite(d), d + np.float32(0.001), np.float32(np.nan)).astype(np.float32)
        out, rec = ref.refine(poses[name][None], frame)
        hold_call_to_the_twin(s, ref, poses[name][None], frame, out, rec)
        counts[name] = rec.counts[0, :, 0].tolist()
        alone = [rt.terms(planes[[b]], frame, poses[name][b][9:12], 0, cam_of(s), s.ms, s.sf, s.rows, s.cols)[2]["use"].sum() for b in range(s.B)]
        if name == "off screen":
            assert not rec.counts.any() and (rec.status == TOO_FEW_PIXELS).all()
        elif name == "half behind":
            assert rec.counts[0, 0, 0] == alone[0] and 0 < rec.counts[0, 1, 0] < alone[1], (rec.counts.tolist(), alone)   # body 1 lost pixels to body 0
        else:
            assert rec.counts[0, :, 0].sum() > 0 and (rec.counts[0, :, 0] < alone).any(), (name, rec.counts.tolist(), alone)   # the bodies overlap
    print(counts)
    inner = PoseRefiner(sensor, PoseRefiner.Parameters(iters=1)).refine(s.truth[None], s.frame)[1].counts[0, :, 0]
    assert all(sum(counts[n]) < inner.sum() for n in ("left border", "right border", "top border", "bottom border", "corner"))   # cut by the border


def test_end_to_end_error_is_the_twin_chains(gpu_lib, rigs):
    s, sensor = rigs["m1m2m3_322"]
    start = rt.offset_pose(s.truth, *START)
    out, rec = PoseRefiner(sensor).refine(start[None], s.frame)
    pose, trec, trail = rt.chain(s.planes, s.frame, start, cam_of(s), s.ms, s.sf, s.rows, s.cols)
    for b in range(2):
        assert (rec.status[0, b], rec.iterations[0, b], rec.counts[0, b].tolist()) == \
            (trec[b]["status"], trec[b]["iterations"], [trec[b]["count_first"], trec[b]["count_last"]])
        used = trec[b]["iterations"]
        errs = np.array([rt.pose_errors(trail[i][b], s.truth[b]) for i in range(used - 2, used + 1)])   # its last three evaluated iterations
        margin = np.abs(np.diff(errs, axis=0)).max(axis=0)
        got, want = rt.pose_errors(out[0, b], s.truth[b]), rt.pose_errors(pose[b], s.truth[b])
        print("body", b, "device %.4f mm %.4f deg" % (got[0] * 1e3, got[1]), "twin %.4f mm %.4f deg" % (want[0] * 1e3, want[1]),
              "margin %.4f mm %.4f deg" % (margin[0] * 1e3, margin[1]))
        # measured with the twin: body 0 0.60 mm / 2.02 deg, margin 0.04 mm / 0.10 deg; body 1 0.22 mm / 0.65 deg, margin 0.06 mm / 0.06 deg
        assert got[0] <= want[0] + margin[0] and got[1] <= want[1] + margin[1]
        assert got[0] < 1e-3                                                        # from 8.7 mm to under a millimetre


def test_two_calls_give_the_same_bits_in_any_batch(gpu_lib, rigs):
    s, sensor = rigs["m1m2_161"]
    ref = PoseRefiner(sensor)
    a = rt.offset_pose(s.truth, *START)
    b = rt.offset_pose(s.truth, (0.01, 0.01, -0.01), 10.0)
    alone, rec_alone = ref.refine(a[None], s.frame)                                   # n = 1 first: the buffers grow afterwards
    batch = np.stack([b, a] + [s.poses()["half behind"]] * 30)
    out, rec = ref.refine(batch, s.frame)
    again, rec2 = ref.refine(batch, s.frame)
    assert np.array_equal(bits(out), bits(again)) and np.array_equal(rec.counts, rec2.counts) and np.array_equal(bits(rec.rms), bits(rec2.rms))
    assert np.array_equal(bits(out[1]), bits(alone[0])) and np.array_equal(bits(rec.rms[1]), bits(rec_alone.rms[0]))
    sensor.set_observation(s.frame)
    held, _ = ref.refine(batch)                                                      # frame = NULL: the sensor's observation
    assert np.array_equal(bits(held), bits(out))
    assert np.array_equal(sensor.get_observation(), s.frame, equal_nan=True)
    ms = ref.kernel_ms()
    assert len(ms) == 3 and all(0.0 < m < 1000.0 for m in ms), ms


def test_refusals_on_a_live_handle(gpu_lib, rigs):
    s, sensor = rigs["m1_80"]
    ref = PoseRefiner(sensor, PoseRefiner.Parameters(iters=2))
    with RbSensor(s.om, s.cam, s.P, max_particles=1) as fresh:
        for inspect in (lambda: PoseRefiner(fresh).history(0, 0, 0), PoseRefiner(fresh).kernel_ms):
            with pytest.raises(RbSensorError) as e:                                  # before the first call there is nothing to inspect
                inspect()
            assert e.value.code == _capi.RBS_ERR_INVALID_ARGUMENT
    good, _ = ref.refine(s.truth[None], s.frame)
    with pytest.raises(RbSensorError) as e:
        ref.refine(np.repeat(s.truth[None], 65, axis=0), s.frame)
    assert e.value.code == _capi.RBS_ERR_INVALID_ARGUMENT and "exceeds 64" in str(e.value)
    bad = s.truth[None].copy()
    bad[0, 0, 4] = np.inf
    with pytest.raises(RbSensorError) as e:
        ref.refine(bad, s.frame)
    assert e.value.code == _capi.RBS_ERR_INVALID_ARGUMENT and "not finite" in str(e.value)
    for kw in (dict(gate_sigmas=0.0), dict(huber_sigmas=float("nan")), dict(damping=-1e-3), dict(max_rotation=0.0), dict(max_translation=float("inf")),
               dict(eps_rotation=-1.0), dict(eps_translation=float("nan")), dict(min_pixels=0), dict(iters=0), dict(iters=33)):
        with pytest.raises(RbSensorError) as e:
            PoseRefiner(sensor, PoseRefiner.Parameters(**kw)).refine(s.truth[None], s.frame)
        assert e.value.code == _capi.RBS_ERR_INVALID_ARGUMENT, kw
    for bad_index in ((1, 0, 0), (0, 1, 0), (0, 0, 2), (-1, 0, 0)):
        with pytest.raises(RbSensorError):
            ref.history(*bad_index)
    assert np.array_equal(bits(ref.refine(s.truth[None], s.frame)[0]), bits(good))     # a refused call changes nothing
    out32, r32 = PoseRefiner(sensor, PoseRefiner.Parameters(iters=32)).refine(s.truth[None], s.frame)   # the most iterations
    assert r32.iterations[0, 0] <= 32 and np.isfinite(out32).all()


def test_refining_leaves_the_assessor_and_a_tracker_alone(gpu_lib, rigs):
    from dbot_ros_amd.tracker import DeviceParticleTracker, ObjectTransitionBuilder, ParticleTrackerBuilder
    s, sensor = rigs["m1m2_161"]
    a = PoseAssessor(sensor, PoseAssessor.Parameters(**asc.PARAMS))
    before = a.assess(s.truth[None], s.frame)
    plane, ms = a.plane(0, 1).copy(), a.kernel_ms()
    PoseRefiner(sensor).refine(np.stack([rt.offset_pose(s.truth, *START)] * 3), s.frame)
    assert np.array_equal(a.plane(0, 1).view(np.uint32), plane.view(np.uint32)) and a.kernel_ms() == ms   # the assessor's own last call
    assert np.array_equal(a.assess(s.truth[None], s.frame).counts, before.counts)

    s1 = asc.Scene(("m1",), 80, 60)
    rng = np.random.default_rng(4)
    truths = [synth.truth_pose(1, z=0.7, frame=k) for k in range(6)]
    frames = [synth.make_frame(s1.orc.render_depth(t), s1.rows, s1.cols, rng) for t in truths]

    def run(refine, look_ahead):
        sn = RbSensor(s1.om, s1.cam, RbSensorBuilder.Parameters(sample_count=200), max_particles=200)
        tr = DeviceParticleTracker(ObjectTransitionBuilder(ObjectTransitionBuilder.Parameters(
            0.002, 0.002, 0.002, 0.01, 0.01, 0.01, 0.8)).build(), sn, s1.om, ParticleTrackerBuilder.Parameters(evaluation_count=200),
            device_rng=True, seed=3)
        ref = PoseRefiner(sn, PoseRefiner.Parameters(min_pixels=8))
        tr.initialize([asc.truth_state(s1.om, truths[0][0])])
        ests, refined = [], []
        if refine:
            with pytest.raises(ValueError):
                tr.refine(frames[0], refiner=ref)                       # nothing tracked yet
        if look_ahead:
            tr.submit(frames[0])
            for k in range(1, len(frames)):
                tr.submit(frames[k])
                ests.append(tr.result())
                if refine:
                    with pytest.raises(ValueError):
                        tr.refine(refiner=ref)                          # a frame in flight: whose observation?
                    refined.append(tr.refine(frames[k - 1], refiner=ref)[0])
            ests.append(tr.result())
        else:
            for fr in frames:
                ests.append(tr.track(fr))
                if refine:
                    given, rec = tr.refine(fr, refiner=ref)
                    held, _ = tr.refine(refiner=ref)                    # the sensor's observation IS this frame
                    assert np.array_equal(bits(given), bits(held)) and given.shape == (12,)
                    assert np.array_equal(bits(given[6:]), bits(ests[-1][6:]))      # the velocities are the estimate's
                    refined.append(given)
        tr.close()
        sn.close()
        return np.array(ests), refined

    for la in (False, True):
        base, _ = run(False, la)
        got, refined = run(True, la)
        assert np.array_equal(bits(got), bits(base)), la                # observation, clock, staged poses, planes, windows: untouched
        assert len(refined) >= len(frames) - 1 and all(np.isfinite(r).all() for r in refined)
    s1.close()


def test_the_finder_returns_both_pose_sets(gpu_lib):
    """One scene of tests/test_gpu_find_refinement.py's set (m1 at 320 x 240, its SMALL parameters): with refine unset a find
    is what it was; with it the finder's own poses, states and scores are still those, bit for bit, beside the refined ones."""
    from test_gpu_finder import SMALL, _params, _scene
    from dbot_ros_amd.finder import ObjectFinder
    om, cam, P, sensor, truth, frame = _scene("m1", 320, 240, seed=3)
    p = _params(**SMALL, seed=11)
    with sensor, ObjectFinder(sensor, om, p) as fnd:
        plain = fnd.find(frame)
        assert plain.refined is None and plain.refinement is None and plain.refined_states is None
        ref = PoseRefiner(sensor)
        a = PoseAssessor(sensor)
        r = fnd.find(frame, refine=ref, assess=a)
        assert r.found == plain.found and np.array_equal(bits(r.poses), bits(plain.poses)) and np.array_equal(bits(r.scores), bits(plain.scores))
        assert np.array_equal(bits(r.states), bits(plain.states))
        K = len(r.poses)
        assert K >= 1 and r.refined.shape == (K, 12) and r.refined_states.shape == (K, 12) and r.refinement.status.shape == (K, 1)
        want, _ = ref.refine(plain.poses, frame)
        assert np.array_equal(bits(r.refined), bits(want.reshape(K, 12)))
        assert np.array_equal(r.assessment.counts, a.assess(r.refined, frame).counts)        # the assessor judged the refined poses
        t = np.asarray(truth, dtype=np.float64).reshape(-1, 12)[0]
        e0, e1 = rt.pose_errors(r.poses[0], t), rt.pose_errors(r.refined[0], t)
        print("finder %.3f mm %.3f deg -> refined %.3f mm %.3f deg" % (e0[0] * 1e3, e0[1], e1[0] * 1e3, e1[1]), r.refinement.status[0], r.refinement.counts[0])
        again = fnd.find(frame)
        assert np.array_equal(bits(again.poses), bits(plain.poses)) and again.refined is None


def test_the_scene_finder_refines_the_searched_bodies_only(gpu_lib):
    """Two bodies at 160 x 120 (tests/test_gpu_scene_find.py's scene and TINY parameters), body 0 searched and body 1 given:
    the finder's own result is what it is without `refine`, the given body's pose comes back bit for bit in `refined`, and
    the searched body's refined pose is the refiner's of the pair."""
    import scene_find_scenes as ss
    from test_gpu_finder import TINY, _params
    from dbot_ros_amd.finder import SceneFinder
    s = ss.Scene(("m1", "m2"), 160, 120, 3)
    with RbSensor(s.om, s.cam, s.P, max_particles=1) as sensor:
        ref = PoseRefiner(sensor)
        with SceneFinder(sensor, s.om, _params(**TINY), SceneFinder.Parameters(polish_sweeps=0)) as fnd:
            plain = fnd.find(s.frame, search=[0], given_poses=s.truth)
            assert plain.refined is None and plain.refined_state is None and plain.refinement is None
            r = fnd.find(s.frame, search=[0], given_poses=s.truth, refine=ref, assess=PoseAssessor(sensor))
            assert np.array_equal(bits(r.poses), bits(plain.poses)) and np.array_equal(bits(r.state), bits(plain.state))
            assert np.array_equal(bits(r.poses[1]), bits(s.truth[1]))
            if np.isfinite(r.poses).all():
                want, rec = ref.refine(r.poses[None], s.frame)
                assert r.refined.shape == (2, 12) and r.refined_state.shape == (24,) and r.refinement.status.shape == (1, 2)
                assert np.array_equal(bits(r.refined[0]), bits(want[0, 0])) and np.array_equal(bits(r.refined[1]), bits(s.truth[1]))
                assert np.array_equal(r.assessment.counts, PoseAssessor(sensor).assess(r.refined[None], s.frame).counts)
            else:
                assert r.refined is None


def test_the_supervisor_confirms_the_refined_pose(gpu_lib):
    """test_gpu_assess.py's jumping object, with a finder that answers 4 mm off: the state the assessor confirms and the
    tracker restarts from is the refiner's, nearer the truth than the finder's."""
    from dbot_ros_amd.supervisor import TrackSupervisor
    from dbot_ros_amd.tracker import DeviceParticleTracker, ObjectTransitionBuilder, ParticleTrackerBuilder
    s = asc.Scene(("m1",), 160, 120)
    rng = np.random.default_rng(6)
    n_frames, jump_at = 10, 3
    truths = []
    for k in range(n_frames):
        t = synth.truth_pose(1, z=0.7, frame=k)
        if k >= jump_at:
            t[:, 9] += 0.10
        truths.append(t)
    frames = [synth.make_frame(s.orc.render_depth(t), s.rows, s.cols, rng, occluder=False) for t in truths]
    states = [asc.truth_state(s.om, t[0]) for t in truths]
    index = {fr.tobytes(): k for k, fr in enumerate(frames)}
    off = np.array([0.004, 0.0, 0.0] + [0.0] * 9)

    class Spy(PoseAssessor):
        judged = []

        def assess_state(self, tracker, state, frame=None):
            Spy.judged.append(np.array(state, dtype=np.float64))
            return super().assess_state(tracker, state, frame)

    with RbSensor(s.om, s.cam, RbSensorBuilder.Parameters(sample_count=400), max_particles=400) as sensor:
        tr = DeviceParticleTracker(ObjectTransitionBuilder(ObjectTransitionBuilder.Parameters(
            0.002, 0.002, 0.002, 0.01, 0.01, 0.01, 0.8)).build(), sensor, s.om, ParticleTrackerBuilder.Parameters(evaluation_count=400),
            device_rng=True, seed=3)
        ref = PoseRefiner(sensor)
        sup = TrackSupervisor(tr, Spy(sensor, PoseAssessor.Parameters(**asc.PARAMS)),
                              find=lambda fr: states[index[np.asarray(fr).tobytes()]] + off, lost_frames=3, refine=ref)
        tr.initialize([states[0]])
        events = []
        for k, fr in enumerate(frames):
            est, verdicts, ev = sup.step(fr)
            events.append(ev)
            if ev == "reacquired":
                want, _ = ref.refine_state(tr, states[k] + off, fr)
                assert np.array_equal(bits(est), bits(want)) and np.array_equal(bits(Spy.judged[-1]), bits(want))
                e_found, e_ref = np.linalg.norm(off[:3]), np.linalg.norm(est[:3] - states[k][:3])
                print("re-found %.2f mm off, refined %.2f mm off" % (e_found * 1e3, e_ref * 1e3), sup.last_refinement.status, sup.last_refinement.counts)
                assert e_ref < e_found
        tr.close()
    s.close()
    assert [e for e in events if e is not None] == ["lost", "reacquired"], events


# ---------------------------------------------------------------------------------------------- the replays
# a search small enough for a test; the assessor set so that every pose with a pixel on screen reads SUPPORTED: the replays
# below are about WHICH state is refined, judged and started from, not about how good the find is
REPLAY_FINDER = dict(max_seeds=48, n_rotations=128, n_candidates=256, n_survivors=8, rounds=3, children=16, batch=4096, seed=11,
                     foreground={})
LENIENT = dict(min_support_fraction=0.0, min_visible_fraction=0.0, min_pixels=1)


@pytest.fixture()
def recording(tmp_path):
    """test_node.py's recorded-dataset scenario at 320 x 240 (downsampling_factor 2), six frames: (tree, dataset, mesh path, centre)."""
    from test_node import _write
    from dbot_ros_amd import dataset as ds
    from dbot_ros_amd import node, objloader
    tree = node.load_rosparams(*_write(tmp_path))
    tree["downsampling_factor"] = 2
    tree["object_finder"] = dict(REPLAY_FINDER)
    tree["supervisor"] = {"assess": dict(LENIENT)}
    K = synth.camera_matrix(640, 480)
    vs, ts = objloader.SimpleWavefrontObjectModelLoader(objloader.ObjectResourceIdentifier(str(tmp_path), "object_models", ["part.obj"])).load()
    om = ObjectModel(vs, ts, center=True)
    rng = np.random.default_rng(0)
    rec = ds.TrackingDataset(tmp_path / "recording", load=False)
    with RbSensor(om, CameraData(K, 480, 640), RbSensorBuilder.Parameters(sample_count=1), max_particles=1) as full:
        for k in range(1, 7):
            native = synth.make_frame(full.render_depth(synth.truth_pose(1, frame=k)), 480, 640, rng, occluder=False)
            stamp = ds.Stamp.from_sec(1500000000.0 + k / 30.0)
            rec.add_frame(ds.Image(native.reshape(480, 640), stamp, seq=k), ds.CameraInfo(K, 480, 640, stamp, seq=k))
    rec.store()
    return tree, ds.TrackingDataset(tmp_path / "recording"), str(tmp_path), np.array(om.centers[0])


@pytest.fixture()
def spies(monkeypatch):
    """What the refiner was asked and answered, what the assessor judged, what the tracker was started from."""
    from dbot_ros_amd.tracker import DeviceParticleTracker
    log = dict(refined=[], judged=[], started=[])
    refine, assess, initialize = PoseRefiner.refine, PoseAssessor.assess, DeviceParticleTracker.initialize

    def spy_refine(self, poses, frame=None):
        out, rec = refine(self, poses, frame)
        log["refined"].append((np.array(poses, dtype=np.float64).reshape(-1, 12), out.reshape(-1, 12).copy()))
        return out, rec

    def spy_assess(self, poses, frame=None):
        log["judged"].append(np.array(poses, dtype=np.float64).reshape(-1, 12))
        return assess(self, poses, frame)

    def spy_initialize(self, states):
        log["started"].append(np.array(states[0], dtype=np.float64))
        return initialize(self, states)

    monkeypatch.setattr(PoseRefiner, "refine", spy_refine)
    monkeypatch.setattr(PoseAssessor, "assess", spy_assess)
    monkeypatch.setattr(DeviceParticleTracker, "initialize", spy_initialize)
    return log


def which(state, poses, centre):
    """The index of the pose whose tracker state `state` is, bit for bit (-1: none)."""
    hits = [i for i, q in enumerate(poses) if np.array_equal(bits(state_of(q, centre)), bits(state))]
    return hits[0] if hits else -1


def state_of(pose, centre):
    from dbot_ros_amd.pose import matrix_to_rotvec
    R = pose[:9].reshape(3, 3)
    s = np.zeros(12)
    s[0:3] = pose[9:12] - R @ centre
    s[3:6] = matrix_to_rotvec(R)
    return s


def test_a_supervised_replay_refines_only_when_asked(gpu_lib, recording, spies):
    """refine unset and supervisor/refine: false are one replay, bit for bit, and never build a refiner; refine=True and
    supervisor/refine: true are one replay too: the frame-0 find's poses go through the refiner, the assessor judges the
    refined ones, and the tracker starts from the refined state of the confirmed pose -- the replay is, bit for bit, the
    plain one started from that state."""
    from dbot_ros_amd import node
    tree, data, path, centre = recording
    base = node.replay_dataset_supervised(tree, data, path, seed=3)
    assert not spies["refined"]
    found = spies["judged"][0]                                         # the find's poses as the assessor saw them on frame 0
    i = which(spies["started"][-1], found, centre)                     # the confirmed one (lenient assessor: the first on screen)
    assert i >= 0
    for k in spies:
        spies[k].clear()
    off_tree = dict(tree, supervisor=dict(tree["supervisor"], refine=False))
    off = node.replay_dataset_supervised(off_tree, data, path, seed=3)
    assert not spies["refined"]
    assert np.array_equal(bits(off[0]), bits(base[0])) and np.array_equal(off[1], base[1]) and off[2] == base[2]
    assert base[0].shape == (6, 12) and base[2] == [None] * 6          # nothing re-found: the find paths ran once, on frame 0
    for k in spies:
        spies[k].clear()
    on = node.replay_dataset_supervised(tree, data, path, seed=3, refine=True)
    assert len(spies["refined"]) == 1
    asked, answered = spies["refined"][0]
    assert np.array_equal(bits(asked), bits(found))                    # the finder's own poses, the same find
    assert np.array_equal(bits(spies["judged"][0]), bits(answered)) and not np.array_equal(bits(answered), bits(asked))
    j = which(spies["started"][-1], answered, centre)                  # started from a REFINED pose, the confirmed one
    assert j >= 0
    start = spies["started"][-1].copy()
    print("supervised replay: pose", i, "confirmed plain, pose", j, "refined;", float(np.linalg.norm(answered[j][9:] - asked[j][9:])) * 1e3, "mm moved")
    keyed = node.replay_dataset_supervised(dict(tree, supervisor=dict(tree["supervisor"], refine=True)), data, path, seed=3)
    assert np.array_equal(bits(keyed[0]), bits(on[0])) and keyed[2] == on[2]
    given = node.replay_dataset_supervised(tree, data, path, initial_states=[start], seed=3)
    assert np.array_equal(bits(given[0]), bits(on[0])) and np.array_equal(given[1], on[1]) and given[2] == on[2]
    with pytest.raises(ValueError, match=r"'refine'\]"):                # the unknown-key message names the new key
        node.replay_dataset_supervised(dict(tree, supervisor={"refined": True}), data, path)


def test_a_replay_starts_from_the_refined_find_when_the_tree_says_so(gpu_lib, recording, spies):
    from dbot_ros_amd import node
    tree, data, path, centre = recording
    base, _ = node.replay_dataset(tree, data, path, None, seed=3)
    assert not spies["refined"]
    plain_start = spies["started"][-1].copy()
    for k in spies:
        spies[k].clear()
    on_tree = dict(tree, object_finder=dict(tree["object_finder"], refine=True), pose_refiner={"iters": 6})
    on, _ = node.replay_dataset(on_tree, data, path, None, seed=3)
    assert len(spies["refined"]) == 1
    asked, answered = spies["refined"][0]
    assert np.array_equal(bits(state_of(asked[0], centre)), bits(plain_start))            # the same find ...
    start = spies["started"][-1].copy()
    assert np.array_equal(bits(start), bits(state_of(answered[0], centre)))               # ... started from its refined pose 0
    for k in spies:
        spies[k].clear()
    given, _ = node.replay_dataset(tree, data, path, [start], seed=3)
    assert np.array_equal(bits(given), bits(on)) and on.shape == (6, 12)
    off, _ = node.replay_dataset(dict(tree, object_finder=dict(tree["object_finder"], refine=False)), data, path, None, seed=3)
    assert np.array_equal(bits(off), bits(base)) and not spies["refined"]
