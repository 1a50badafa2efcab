"""The occlusion map ON THE DEVICE (dbot_ros_amd/csrc/rbsensor_occmap.hip): rbs_occlusion_mean on every storage layout
against the twin over the planes rbs_get_occlusion hands out afterwards, the sensor left alone, the refusals; the device
tracker's per-frame map on every route against the twin on get_state(), the unchanged filter, look-ahead, determinism;
rbs_occlusion_bodies against the assessor's planes; an occluder seen end to end; the C++ mirror and the node assembly.

The bar (tests/occmap_twin.py, derived there):  |M_dev(p) - T(p)| <= 1/2 spacing32(T(p)) + (n + 16) 2^-52.

Outside every live window the map is the background value bit for bit.  There every live slot has the same float b at the
pixel, so the device forms fl(sum W_s b) / S in binary64: each product and each addition moves the sum by at most 2^-53
relative (all terms have one sign), and sum W_s and S are two orders of the same n additions of the e_i, so the quotient is
b (1 + d) with |d| <= (2 L + 2 n + 2) 2^-53 for L live slots.  b is a float: its neighbours are at least 2^-24 |b| away, so
the one rounding to float gives b back while |d| < 2^-25 -- for every n below 2^25."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import occlusion_map_worker as wk
import occmap_twin as ot
import scenarios as sc
from dbot_ros_amd import CameraData, ObjectModel, RbSensor, RbSensorBuilder, RbSensorError, _capi, synth
from dbot_ros_amd.assess import PoseAssessor
from dbot_ros_amd.tracker import DeviceParticleTracker, ObjectTransitionBuilder, ParticleTrackerBuilder, occlusion_map_of

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ROWS, COLS, N = wk.ROWS, wk.COLS, 24
NPX = ROWS * COLS
# name -> (RbSensor keywords, the shared trail forced with rbs_shared_trail_rebase, planes planted with rbs_set_occlusion)
CONFIGS = {
    "window": (dict(state_layout="window"), False, False),
    "dense": (dict(state_layout="dense"), False, False),
    "slab": (dict(state_layout="window", slab_px=1024), False, True),
    "reference": (dict(state_layout="window", occlusion="reference"), False, True),
    "reference_slab": (dict(state_layout="window", occlusion="reference", slab_px=1024), False, True),
    "trail": (dict(state_layout="window"), True, False),
    "trail_slab": (dict(state_layout="window", slab_px=1024), True, True),
    "trail_reference": (dict(state_layout="window", occlusion="reference"), True, True),
}
PLANTED = 6          # the last slots take tests/occmap_twin.planted_planes on the configurations that plant
worst = {}


def _scene():
    return sc.make_scene(("m1_l2",), COLS, ROWS, max_particles=N)


def _poses(k, rng):
    """N particles spread over the image (a 6 x 4 grid of offsets, the outer ones at the frame's edge) around frame k's truth."""
    truth = synth.truth_pose(1, frame=k)
    p = synth.particle_poses(truth, N, rng, scale=1.0 + 0.5 * k)
    dx, dy = np.meshgrid(np.linspace(-0.37, 0.37, 6), np.linspace(-0.27, 0.27, 4))
    p[:, 0, 9] += dx.ravel()
    p[:, 0, 10] += dy.ravel()
    return p


def _build(name, calls=3, extra_calls=0, maps_between=None):
    """A handle of configuration `name` after `calls` updating loglikes calls (+ planted planes); then, for the test that the
    map leaves the sensor's future alone, maps_between(handle) and extra_calls more updating calls whose log-likelihoods are
    returned too."""
    kw, trail, plant = CONFIGS[name]
    om, cam, P = _scene()
    rng = np.random.default_rng(3)
    g = RbSensor(om, cam, P, max_particles=N, **kw)
    frng = np.random.default_rng(9)
    lls = []
    for k in range(calls + extra_calls):
        if k == calls:
            if plant:
                bg = np.float32(g.get_background())
                for j, plane in ot.planted_planes(ROWS, COLS, PLANTED, bg, seed=5).items():
                    g.set_occlusion(N - PLANTED + j, plane)
            if maps_between is not None:
                maps_between(g)
        g.set_observation(synth.make_frame(g.render_depth(synth.truth_pose(1, frame=k)), ROWS, COLS, frng, occluder=True))
        parents = np.arange(N)
        if k > 0:
            swap = rng.random(N) < 0.25
            parents = np.sort(np.where(swap, np.clip(parents + rng.integers(-1, 2, N), 0, N - 1), parents))
        if trail and k >= 1:
            # (asked before every updating call: a call that is taken back because a region outgrew its slab -- re-measured
            # against slot 0's plane a far particle's window spans the frame -- has spent its request, and left alone the
            # handle's own policy may leave the trail again)
            g.shared_trail_rebase(0)
        lls.append(g.loglikes_poses(_poses(k, rng), parents.astype(np.int32), update=True))
    if extra_calls == 0 and plant:
        bg = np.float32(g.get_background())
        for j, plane in ot.planted_planes(ROWS, COLS, PLANTED, bg, seed=5).items():
            g.set_occlusion(N - PLANTED + j, plane)
    assert g.shared_trail_state()[0] == trail, name
    return g, lls


# ---------------------------------------------------------------- rbs_occlusion_mean on every layout
@pytest.mark.parametrize("name", list(CONFIGS))
def test_map_holds_the_bar_and_leaves_the_sensor_alone(gpu_lib, name):
    g, _ = _build(name)
    windowed = CONFIGS[name][0]["state_layout"] == "window"
    with g:
        pops = ot.populations(N, seed=11)
        wins = [g.get_window(s) for s in range(N)]
        state = g.shared_trail_state()
        maps = [g.occlusion_mean(idx, lw) for _, _, idx, lw in pops]
        again = [g.occlusion_mean(idx, lw) for _, _, idx, lw in pops[::7]]
        assert g.occlusion_mean_ms() > 0.0                    # the events either side of the launches work
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(maps[::7], again)), "two calls, other bits"
        assert [g.get_window(s) for s in range(N)] == wins and g.shared_trail_state() == state, "the map moved a window"
        if windowed and not CONFIGS[name][1]:          # (the cases the windows are meant to make: they differ, one is at the edge, one is empty)
            areas = [(w[2] - w[0]) * (w[3] - w[1]) for w in wins if w[2] > w[0]]
            assert len(set(wins)) >= 4 and min(areas) < NPX // 4, "the windows do not differ"
            assert any(w[0] == 0 or w[1] == 0 or w[2] == COLS or w[3] == ROWS for w in wins if w[2] > w[0]), "no window at the frame's edge"
            if CONFIGS[name][2]:
                assert wins[N - PLANTED][2] <= wins[N - PLANTED][0], "the all-background plane has a window"
        planes = np.stack([g.get_occlusion(s) for s in range(N)])          # AFTER the maps (on float windowed planes this makes them dense)
        assert (planes >= 0).all() and (planes <= 1).all()
        saw_outside = False
        for (pname, n, idx, lw), m in zip(pops, maps):
            twin = occlusion_map_of(planes, lw, idx)
            ot.check(m, twin, n, note=worst, what=name)
            live = np.unique(idx if lw is None else idx[np.isfinite(lw)])
            assert (m >= planes[live].min(axis=0)).all() and (m <= planes[live].max(axis=0)).all(), pname
            if windowed:
                outside = ~np.any([ot.inside(wins[s], ROWS, COLS) for s in live], axis=0)
                if outside.any():
                    saw_outside = True
                    assert (planes[live][:, outside] == planes[live[0]][outside]).all(), pname        # every live plane is the background there
                    assert np.array_equal(m[outside].view(np.uint32), planes[live[0]][outside].view(np.uint32)), pname
        assert saw_outside or not windowed
    print("worst share of the bar so far:", worst)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_calls_that_follow_give_the_bits_of_a_handle_that_never_asked(gpu_lib, name):
    pops = ot.populations(N, seed=12)[::5]

    def ask(g):
        for _, _, idx, lw in pops:
            g.occlusion_mean(idx, lw)

    a, lla = _build(name, extra_calls=2, maps_between=ask)
    b, llb = _build(name, extra_calls=2)
    with a, b:
        for k, (x, y) in enumerate(zip(lla, llb)):
            assert np.isfinite(x).all() and x.tobytes() == y.tobytes(), (name, k)
        assert [a.get_window(s) for s in range(N)] == [b.get_window(s) for s in range(N)]
        for s in (0, 5, N - 1):
            assert np.array_equal(a.get_occlusion(s).view(np.uint32), b.get_occlusion(s).view(np.uint32)), s


def test_render_depth_observation_and_staged_poses_are_left_alone(gpu_lib):
    g, _ = _build("window")
    with g:
        pose = synth.truth_pose(1, frame=2)
        before = (g.render_depth(pose), g.get_observation(), g.get_poses(N), g.get_background())
        g.occlusion_mean(np.arange(N, dtype=np.int32) % 5, None)
        after = (g.render_depth(pose), g.get_observation(), g.get_poses(N), g.get_background())
        for x, y in zip(before[:3], after[:3]):
            assert np.asarray(x).tobytes() == np.asarray(y).tobytes()
        assert before[3] == after[3]


def test_sensor_level_refusals(gpu_lib):
    om, cam, P = _scene()

    def refused(code, fn):
        with pytest.raises(RbSensorError) as e:
            fn()
        assert e.value.code == code, (e.value.code, str(e.value))

    inv = _capi.RBS_ERR_INVALID_ARGUMENT
    with RbSensor(om, cam, P, max_particles=N) as g:
        refused(inv, g.occlusion_mean_ms)                                                  # no map yet
        refused(inv, lambda: g.occlusion_mean(np.zeros(0, np.int32)))                       # n < 1
        refused(inv, lambda: g.occlusion_mean(np.array([0, N], np.int32)))                  # a slot out of range
        refused(inv, lambda: g.occlusion_mean(np.array([-1], np.int32)))
        refused(inv, lambda: g.occlusion_mean(np.array([0, 1], np.int32), np.array([0.0, np.nan])))
        refused(inv, lambda: g.occlusion_mean(np.array([0, 1], np.int32), np.array([0.0, np.inf])))
        refused(inv, lambda: g.occlusion_mean(np.array([0, 1], np.int32), np.array([-np.inf, -np.inf])))
        m = g.occlusion_mean(np.array([0, 1], np.int32), np.array([-np.inf, 0.0]))           # -inf alone is a member without weight
        assert np.array_equal(m, g.get_occlusion(1))
        pose = synth.truth_pose(1, frame=0)
        flat = np.full(NPX, 0.5, np.float32)
        refused(inv, lambda: g.occlusion_bodies(flat, np.zeros((0, 1, 12))))                # n < 1
        refused(inv, lambda: g.occlusion_bodies(flat, np.repeat(pose[None], 65, axis=0)))    # n x n_objects > 64
        refused(inv, lambda: g.occlusion_bodies(flat, pose[None], threshold=1.5))
        refused(inv, lambda: g.occlusion_bodies(flat, pose[None], threshold=float("nan")))
        for bad in (np.nan, -0.25, 1.5, np.inf):
            spoiled = flat.copy()
            spoiled[NPX // 2] = bad
            refused(inv, lambda: g.occlusion_bodies(spoiled, pose[None]))
        nanpose = pose[None].copy()
        nanpose[0, 0, 3] = np.nan
        refused(inv, lambda: g.occlusion_bodies(flat, nanpose))
    with RbSensor(om, cam, P, max_particles=N, precision="f64", device_ids=[0, 0]) as grp:      # a handle over several shards
        refused(_capi.RBS_ERR_UNSUPPORTED, lambda: grp.occlusion_mean(np.zeros(2, np.int32)))
        refused(_capi.RBS_ERR_UNSUPPORTED, lambda: grp.occlusion_bodies(np.full(NPX, 0.5, np.float32), synth.truth_pose(1)[None]))


# ---------------------------------------------------------------- the tracker itself
_runs = {}


def _run(n, max_kl=2.0, again=0, **kw):
    key = (n, max_kl, again, tuple(sorted(kw.items())))
    if key not in _runs:
        _runs[key] = wk.run(n, max_kl, **kw)
    return _runs[key]


def _same_maps(a, b):
    return a["maps"].tobytes() == b["maps"].tobytes() and a["map_frames"].tobytes() == b["map_frames"].tobytes()


SIZES = pytest.mark.parametrize("n", [300, 600, 8200], ids=["fused_300", "tail_600", "grid_8200"])


@pytest.mark.parametrize("max_kl", [0.0, 1e9], ids=["always_resamples", "never_resamples"])
@SIZES
def test_tracker_map_matches_the_twin_on_get_state(gpu_lib, n, max_kl):
    r = wk.run(n, max_kl, states=True, planes=True)        # (not kept: at 8 200 particles that never resample 8 200 planes a frame)
    for k in range(wk.FRAMES):
        idx, lw = r["indices"][k], r["log_weights"][k]
        by_slot = dict(zip((int(s) for s in r["slots"][k]), r["planes"][k]))
        ot.check(r["maps"][k], occlusion_map_of(by_slot, lw, idx), n, note=worst, what="tracker")
        assert r["map_frames"][k] == k + 1 and r["maps"][k].shape == (ROWS, COLS)
        assert len(by_slot) < n if max_kl == 0.0 else len(by_slot) == n
    assert np.ptp(r["maps"][-1]) > 0.01, "a flat map: nothing was learnt"
    print("worst share of the bar so far:", worst)


@SIZES
def test_filter_is_unchanged_by_the_map(gpu_lib, n):
    """Estimates, particles, weights, slot maps and resamplings with the map on are those of a tracker without it -- also with
    the posterior report beside it, whose own numbers do not move either."""
    on, off = _run(n, states=True), _run(n, occlusion_map=False, states=True)
    both, post = _run(n, posterior=True), _run(n, occlusion_map=False, posterior=True)
    assert "maps" in on and "maps" not in off
    for k in ("estimates", "particles", "log_weights", "indices", "resamplings"):
        assert on[k].tobytes() == off[k].tobytes(), k
    for k in ("estimates", "resamplings"):
        assert both[k].tobytes() == off[k].tobytes() and post[k].tobytes() == off[k].tobytes(), k
    assert both["post_mean"].tobytes() == post["post_mean"].tobytes()
    assert on["resamplings"][-1] >= 1


@SIZES
def test_look_ahead_gives_the_maps_of_frame_by_frame(gpu_lib, n):
    """Two frames in flight: result(k)'s map is frame k's (its number says so) while k + 1 is in flight -- whose sampling
    blocks write the plane buffer beside the one frame k's map reads, and the one after that the very buffer --, bit for bit
    the map of the frame-by-frame run; with the posterior report beside it as well."""
    a, b = _run(n), _run(n, look_ahead=True)
    assert a["estimates"].tobytes() == b["estimates"].tobytes()
    assert b["map_frames"].tolist() == list(range(1, wk.FRAMES + 1))
    assert _same_maps(a, b)
    assert _same_maps(a, _run(n, posterior=True)) and _same_maps(a, _run(n, posterior=True, look_ahead=True))


def test_two_runs_give_the_same_bits(gpu_lib):
    for n in (600, 8200):
        assert _same_maps(_run(n), _run(n, again=1)), n


def test_tracker_refusals(gpu_lib):
    n = 64
    om, cam, P = sc.make_scene(("m1_l2",), COLS, ROWS, max_particles=n)
    tp = ParticleTrackerBuilder.Parameters(evaluation_count=n)
    trans = ObjectTransitionBuilder(ObjectTransitionBuilder.Parameters()).build()
    inv = _capi.RBS_ERR_INVALID_ARGUMENT

    def refused(code, fn):
        with pytest.raises(RbSensorError) as e:
            fn()
        assert e.value.code == code, (e.value.code, str(e.value))

    with RbSensor(om, cam, P, max_particles=n) as s:
        dev = DeviceParticleTracker(trans, s, om, tp, np.random.default_rng(5))
        dev.initialize([wk.initial_state(om)])
        frames = wk.scene_frames(s, 3)
        dev.track(frames[0])
        refused(inv, dev.occlusion_map)                       # the map is off
        refused(inv, dev.occlusion_map_ms)
        dev.set_occlusion_map(True)
        refused(inv, dev.occlusion_map)                       # on, but no frame has been handed out since
        dev.track(frames[1])
        assert dev.occlusion_map().frame == 2
        dev.initialize([wk.initial_state(om)])
        refused(inv, dev.occlusion_map)                       # after initialize, before the next result
        dev.submit(frames[0])
        refused(inv, lambda: dev.set_occlusion_map(False))    # a frame in flight
        refused(inv, dev.occlusion_map)
        dev.result()
        m = dev.occlusion_map()
        assert m.frame == 1 and m.plane.shape == (ROWS, COLS)
        assert dev.occlusion_map_ms() > 0.0                   # the map's kernels' device time, from events
        p, w, i = dev.get_state()
        assert np.array_equal(m.plane.ravel().view(np.uint32), s.occlusion_mean(i, w).view(np.uint32))   # the sensor-level call: the same kernels
        dev.set_occlusion_map(False)
        dev.track(frames[1])
        refused(inv, dev.occlusion_map)                       # off again
        dev.set_occlusion_map(True)
        dev.set_posterior(True)                                # either, both or neither
        dev.track(frames[2])
        assert dev.occlusion_map().frame == 3 and dev.posterior().frame == 3
        import ctypes as C
        frame = C.c_int32()
        assert dev._lib.rbs_tracker_occlusion_map(dev._t, None, None) == 0           # NULL outputs are allowed, one by one
        assert dev._lib.rbs_tracker_occlusion_map(dev._t, C.byref(frame), None) == 0 and frame.value == 3
        occ = dev.occlusion_of_estimate()
        assert len(occ) == 1 and occ[0].rendered > 20 and 0.0 <= occ[0].mean <= 1.0 and 0 <= occ[0].occluded <= occ[0].rendered
        dev.close()
    with RbSensor(om, cam, P, max_particles=n, precision="f64", device_ids=[0, 0]) as grp:      # a tracker over several shards
        dev = DeviceParticleTracker(trans, grp, om, tp, np.random.default_rng(5))
        refused(_capi.RBS_ERR_UNSUPPORTED, lambda: dev.set_occlusion_map(True))
        dev.close()


def test_poisoned_tracker_refuses_the_map_first(gpu_lib):
    """In a process of its own that loads the hooks build, where the injected fault exists (tests/occlusion_map_worker.py).
    The fault poisons handles over several devices only: the sensor-level calls refuse such a handle as UNSUPPORTED before
    they look at the poison, which the same run pins."""
    import filter_probes as fp
    hooks = fp.hooks_path(_capi.LIB_PATH)
    assert os.path.exists(hooks), "build() makes librbsensor_mi355x_hooks.so"
    r = subprocess.run([sys.executable, os.path.join(HERE, "occlusion_map_worker.py"), "poisoned"], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, RBS_LIB_PATH=hooks))
    assert r.returncode == 0 and r.stdout.strip().endswith("POISONED_OK"), (r.returncode, r.stdout[-2000:], r.stderr[-2000:])


def test_host_tracker_asks_the_sensor_with_its_own_population(gpu_lib):
    from dbot_ros_amd.tracker import ParticleTracker
    n = 32
    om, cam, P = sc.make_scene(("m1_l2",), COLS, ROWS, max_particles=n)
    tp = ParticleTrackerBuilder.Parameters(evaluation_count=n)
    trans = ObjectTransitionBuilder(ObjectTransitionBuilder.Parameters()).build()
    with RbSensor(om, cam, P, max_particles=n) as s:
        tr = ParticleTracker(trans, s, om, tp, np.random.default_rng(5))
        tr.initialize([wk.initial_state(om)])
        with pytest.raises(ValueError):
            tr.occlusion_map()
        for f in wk.scene_frames(s, 2):
            tr.track(f)
        m = tr.occlusion_map()
        assert m.frame == 2 and m.plane.shape == (ROWS, COLS)
        planes = {int(q): s.get_occlusion(int(q)) for q in np.unique(tr.indices)}
        ot.check(m.plane, occlusion_map_of(planes, tr.log_weights, tr.indices), n, note=worst, what="host tracker")
        assert tr.occlusion_of_estimate()[0].rendered > 20


# ---------------------------------------------------------------- rbs_occlusion_bodies
def _bodies_case(s, assessor, m, poses, threshold):
    got = s.occlusion_bodies(m, poses, threshold)
    B = s.n_bodies
    assert got.shape == (len(poses), B, 3)
    for k in range(len(poses)):
        planes = np.stack([assessor.plane(k, b) for b in range(B)])         # the assessor's planes of THIS call
        assert np.array_equal(got[k], ot.bodies_of(planes, m, threshold)), (k, got[k], ot.bodies_of(planes, m, threshold))
    return got


@pytest.mark.parametrize("meshes", [("m1_l2",), ("m1_l2", "box12")], ids=["one_body", "two_bodies"])
def test_bodies_against_the_assessors_planes(gpu_lib, meshes):
    B = len(meshes)
    om, cam, P = sc.make_scene(meshes, COLS, ROWS, max_particles=4)
    rng = np.random.default_rng(2)
    with RbSensor(om, cam, P, max_particles=4) as s:
        assessor = PoseAssessor(s)
        truth = synth.truth_pose(B, frame=1)
        poses = np.repeat(truth[None], 4, axis=0)
        poses[1, :, 9] += 0.37                      # the right-hand body partly out of view
        poses[2, :, 10] -= 0.29                     # every body cut by the upper edge
        if B == 2:
            poses[3, 1, 9:12] = poses[3, 0, 9:12] + [0.02, 0.0, 0.01]      # one body in front of the other: owners decide
        m = rng.uniform(0.0, 1.0, NPX).astype(np.float32)
        sensor_before = (s.get_background(), s.get_window(0), s.shared_trail_state())
        got = _bodies_case(s, assessor, m, poses, 0.5)
        assert (s.get_background(), s.get_window(0), s.shared_trail_state()) == sensor_before
        assert (got[0, :, 0] > 20).all() and (got[1, -1, 0] < got[0, -1, 0]) and (got[2, :, 0] < got[0, :, 0]).all()
        assert (got[..., 1] > 0).any() and (got[..., 1] < got[..., 0]).any()
        # what rbs_assess_get_plane hands out afterwards is what an assessment at these poses leaves
        mine = np.stack([assessor.plane(1, b) for b in range(B)])
        assessor.assess(poses, np.full(NPX, 1.5, np.float32))
        assert np.array_equal(mine, np.stack([assessor.plane(1, b) for b in range(B)]))
        # a map AT the threshold is not above it; one ulp more is
        for thr in (0.5, 0.125, 1.0 - 2.0 ** -24):
            at_thr = np.full(NPX, np.float32(thr), np.float32)
            assert float(at_thr[0]) == thr
            r = _bodies_case(s, assessor, at_thr, poses[:1], thr)
            assert (r[0, :, 1] == 0).all() and (r[0, :, 0] > 0).all()
            above = np.nextafter(at_thr, np.float32(2))
            if above[0] <= 1.0:
                r = _bodies_case(s, assessor, above, poses[:1], thr)
                assert (r[0, :, 1] == r[0, :, 0]).all()
        ones = _bodies_case(s, assessor, np.ones(NPX, np.float32), poses[:1], 1.0)
        assert (ones[0, :, 2] == ones[0, :, 0] * (1 << 32)).all() and (ones[0, :, 1] == 0).all()


# ---------------------------------------------------------------- end to end: an occluder is seen
def test_an_occluder_raises_the_covered_bodys_occlusion(gpu_lib):
    """Twenty frames of the M1 scene with synth.make_frame's slab (0.5 m, in front of the right quarter of the object) against
    the same frames without it: the mean of the map over the body at the published estimate must be higher with the slab.
    The direction is asserted, not a magnitude (measured on one MI355X: 0.2691 with the slab, 0.0001 without; DESIGN.md
    Appendix M)."""
    n, frames = 200, 20
    om, cam, P = sc.make_scene(("m1_l2",), COLS, ROWS, max_particles=n)
    tp = ParticleTrackerBuilder.Parameters(evaluation_count=n)
    trans = ObjectTransitionBuilder(ObjectTransitionBuilder.Parameters()).build()
    means = {}
    for occluder in (True, False):
        with RbSensor(om, cam, P, max_particles=n) as s:
            dev = DeviceParticleTracker(trans, s, om, tp, device_rng=True, seed=4, occlusion_map=True)
            dev.initialize([wk.initial_state(om)])
            for f in wk.scene_frames(s, frames, seed=21, occluder=occluder):
                dev.track(f)
            occ = dev.occlusion_of_estimate()[0]
            means[occluder] = occ.mean
            assert occ.rendered > 20
            dev.close()
    print("mean occlusion of the body: with the slab %.4f, without %.4f" % (means[True], means[False]))
    assert means[True] > means[False]


# ---------------------------------------------------------------- the C++ mirror
def test_cpp_mirror_prints_pythons_bits(gpu_lib, tmp_path):
    exe = str(tmp_path / "occlusion_map_check")
    lib = os.path.join(ROOT, "dbot_ros_amd", "lib")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(HERE, "cpp", "occlusion_map_check.cpp"), "-L" + lib, "-lrbsensor_mi355x", "-Wl,-rpath," + lib,
                           "-Wl,-rpath,/opt/rocm/lib"], timeout=300)
    rows, cols, n, count = 60, 80, 300, 4
    verts = [np.array([[0, 0, 0], [0.2, 0, 0], [0, 0.2, 0], [0, 0, 0.2]], dtype=np.float64)]
    tris = [np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], dtype=np.int32)]
    om = ObjectModel(verts, tris, center=True)
    cam = CameraData.from_native([71.2875, 0, 39.5, 0, 71.2875, 29.5, 0, 0, 1], cols, rows, 1)
    P = RbSensorBuilder.Parameters(sample_count=n)
    tp = ParticleTrackerBuilder.Parameters(evaluation_count=n)
    trans = ObjectTransitionBuilder(ObjectTransitionBuilder.Parameters()).build()
    init = np.zeros(12)
    init[2] = 0.7
    got = []
    with RbSensor(om, cam, P, max_particles=n) as s:
        dev = DeviceParticleTracker(trans, s, om, tp, device_rng=True, seed=11, occlusion_map=True)
        frames = []
        for k in range(count):
            Rt = np.r_[np.eye(3).ravel(), om.centers[0] + [0.002 * (k + 1), 0.0, 0.7]]
            d = np.asarray(s.render_depth(Rt[None]), dtype=np.float64).reshape(rows, cols)
            frames.append(np.where(np.isfinite(d), d, 1.5).ravel())
        path = tmp_path / "frames.bin"
        path.write_bytes(struct.pack("<i", count) + b"".join(f.tobytes() for f in frames))
        dev.initialize([init])
        for f in frames:
            dev.track(f)
            got.append(dev.occlusion_map())
        mean = s.occlusion_mean(np.array([0, 1, 2, 2], np.int32))
        dev.close()
    run = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.returncode, run.stdout[-2000:], run.stderr[-2000:])
    lines = run.stdout.strip().split("\n")
    assert len(lines) == 2 * count + 2, run.stdout[-2000:]

    def floats(line):
        return np.array([float.fromhex(v) for v in line.split()]).astype(np.float32)

    for k, m in enumerate(got):
        assert lines[2 * k].split() == ["FRAME", str(k), str(m.frame)] and m.frame == k + 1
        assert np.array_equal(floats(lines[2 * k + 1]).view(np.uint32), m.plane.ravel().view(np.uint32)), k
    assert np.ptp(got[-1].plane) > 0.01
    assert lines[2 * count] == "MEAN" and np.array_equal(floats(lines[2 * count + 1]).view(np.uint32), mean.view(np.uint32))


# ---------------------------------------------------------------- the node assembly
def test_node_replay_hands_out_the_maps(gpu_lib, tmp_path):
    """replay_dataset(occlusion_map=True) additionally returns every frame's map -- behind the posterior reports when both are
    asked for, look-ahead the same bits -- and leaves its return value alone with the flag off; the YAML key
    particle_filter/occlusion_map switches the map on by itself."""
    import test_node as tn
    from dbot_ros_amd import dataset as ds, node, objloader, pose
    tree = node.load_rosparams(*tn._write(tmp_path))
    K = synth.camera_matrix(640, 480)
    vs, ts = objloader.SimpleWavefrontObjectModelLoader(objloader.ObjectResourceIdentifier(str(tmp_path), "object_models", ["part.obj"])).load()
    om = ObjectModel(vs, ts, center=True)

    def truth_state(k):
        Rt = synth.truth_pose(1, frame=k)[0]
        st = np.zeros(12)
        st[3:6] = pose.matrix_to_rotvec(Rt[:9].reshape(3, 3))
        st[0:3] = Rt[9:] - Rt[:9].reshape(3, 3) @ om.centers[0]
        return st

    rng = np.random.default_rng(0)
    rec = ds.TrackingDataset(tmp_path / "recording", load=False)
    with RbSensor(om, CameraData(K, 480, 640), RbSensorBuilder.Parameters(sample_count=1), max_particles=1) as full:
        for k in range(1, 4):
            native = synth.make_frame(full.render_depth(synth.truth_pose(1, frame=k)), 480, 640, rng, occluder=False)
            stamp = ds.Stamp.from_sec(1500000000.0 + k / 30.0)
            rec.add_frame(ds.Image(native.reshape(480, 640), stamp, seq=k), ds.CameraInfo(K, 480, 640, stamp, seq=k), ground_truth=truth_state(k))
    rec.store()
    data = ds.TrackingDataset(tmp_path / "recording")
    off = node.replay_dataset(tree, data, str(tmp_path), [truth_state(0)], seed=3)
    on = node.replay_dataset(tree, data, str(tmp_path), [truth_state(0)], seed=3, occlusion_map=True)
    ahead = node.replay_dataset(tree, data, str(tmp_path), [truth_state(0)], seed=3, occlusion_map=True, look_ahead=True)
    both = node.replay_dataset(tree, data, str(tmp_path), [truth_state(0)], seed=3, posterior=True, occlusion_map=True)
    assert len(off) == 2 and len(on) == 3 and len(ahead) == 3 and len(both) == 4
    assert np.array_equal(off[0], on[0]) and np.array_equal(on[0], ahead[0]) and np.array_equal(on[0], both[0])
    assert [m.frame for m in on[2]] == [1, 2, 3] and [r.frame for r in both[2]] == [1, 2, 3]
    for a, b, c in zip(on[2], ahead[2], both[3]):
        assert a.plane.ndim == 2 and a.plane.tobytes() == b.plane.tobytes() and a.plane.tobytes() == c.plane.tobytes()
    tree["particle_filter"]["occlusion_map"] = True
    keyed = node.replay_dataset(tree, data, str(tmp_path), [truth_state(0)], seed=3)
    assert len(keyed) == 2 and np.array_equal(keyed[0], off[0])                 # the flag off: the return value stays as it is
    tracker, _, _, _ = node.build_particle_tracker(tree, K, str(tmp_path), seed=3)
    try:
        tracker.initialize([truth_state(0)])
        tracker.track(data.frame_vector(0, int(tree["downsampling_factor"])))
        assert tracker.occlusion_map().plane.tobytes() == on[2][0].plane.tobytes()      # ... but the key has switched the map on
    finally:
        tracker.close()
        tracker.sensor.close()
