"""The object map ON THE DEVICE (dbot_ros_amd/csrc/rbsensor_objmap.hip): rbs_object_map against the twin
(dbot_ros_amd.tracker.object_map_of) over the assessor's planes at the same poses -- rbs_assess_get_plane, pinned by
tests/test_gpu_pose_planes.py, not the code under test --, the sensor left alone, the refusals in their order; rbs_object_segment
against segment_of over the device's own float maps, exactly; the device tracker's per-frame map on every route, the
unchanged filter, look-ahead, determinism, rbs_tracker_poses; twenty frames end to end with and without an occluder.

The bars are derived in tests/objmap_twin.py.  Uncovered pixels read 0, +inf, 0 bit for bit, and a body's cover is exactly 0
where none of its planes owns the pixel."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import object_map_worker as wk
import objmap_twin as jt
import scenarios as sc
from dbot_ros_amd import RbSensor, RbSensorError, _capi, synth
from dbot_ros_amd.tracker import DeviceParticleTracker, ObjectTransitionBuilder, ParticleTrackerBuilder, object_map_of, segment_of

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
M = 300                      # poses of a sensor-level case; a population of n members draws on the first n of them
CASES = {"one_body_80x60": (("m1_l2",), 80, 60), "two_bodies_160x120": (("m1_l2", "box12"), 160, 120)}
worst = {}


def _spread_poses(n_bodies, rng):
    """M poses spread to the frame's edge as tests/test_gpu_occlusion_map._poses spreads them (offsets up to +-0.37 m and
    +-0.27 m at 0.7 m); pose 1 fully off screen, pose 5 with its last body behind the camera (that body's rectangle is the
    whole frame and nothing is drawn into it: tests/test_gpu_pose_planes.py), pose 7 with its bodies interpenetrating."""
    p = synth.particle_poses(synth.truth_pose(n_bodies), M, rng, scale=3.0)
    p[:, :, 9] += rng.uniform(-0.37, 0.37, (M, 1))
    p[:, :, 10] += rng.uniform(-0.27, 0.27, (M, 1))
    p[0, :, 9] -= p[0, 0, 9] - 0.37                      # at the right edge
    p[2, :, 10] -= p[2, 0, 10] + 0.27                    # at the top edge
    p[1, :, 9] += 5.0
    p[5, -1, 11] = -1.0
    if n_bodies > 1:
        p[7, 1, 9:12] = p[7, 0, 9:12] + [0.01, 0.0, 0.0]
    return p


_cases = {}


def _case(name):
    """The sensor's scene, the poses and -- computed once, never changed -- the reference planes."""
    if name not in _cases:
        meshes, cols, rows = CASES[name]
        om, cam, P = sc.make_scene(meshes, cols, rows, max_particles=24)
        poses = _spread_poses(len(meshes), np.random.default_rng(21))
        with RbSensor(om, cam, P, max_particles=24) as g:
            planes = wk.reference_planes(g, poses)
        planes.setflags(write=False)
        _cases[name] = (om, cam, P, poses, planes)
    return _cases[name]


def _documented_groups(live, rect, rows, cols, B):
    """G as include/rbsensor_mi355x.h states it."""
    tile_px = 1024 if B <= 4 else 512
    th = tile_px // 32
    tiles = lambda w, h: ((w + 31) // 32) * ((h + th - 1) // th)          # noqa: E731
    one = tiles(cols, rows) * tile_px * (B + 2)
    cap = max(one, min(32 * one, 4 << 20))
    t = tiles(rect[2] - rect[0], rect[3] - rect[1]) if rect[2] > rect[0] and rect[3] > rect[1] else 0
    return max(1, min(32, (live + 7) // 8, cap // (max(t, 1) * tile_px * (B + 2)))), t


# ---------------------------------------------------------------- rbs_object_map
@pytest.mark.parametrize("name", list(CASES))
def test_map_holds_the_bars_and_uncovered_pixels_are_exact(gpu_lib, name):
    om, cam, P, poses, planes = _case(name)
    meshes, cols, rows = CASES[name]
    B = len(meshes)
    rects = np.tile(np.array([0, 0, cols, rows]), (M, B, 1))             # (the reference planes are +inf outside their rectangles)
    assert not np.isfinite(planes[1]).any() and not np.isfinite(planes[5, -1]).any() and np.isfinite(planes[0]).any()
    if B > 1:
        both = np.isfinite(planes[7]).all(axis=0)
        assert both.sum() > 30, "no overlap to own"
    groups = set()
    with RbSensor(om, cam, P, max_particles=24) as g:
        for pname, n, m, idx, lw in jt.populations(lambda n: n, seed=11):
            dev = g.object_map(poses[:m], idx, lw)
            info = g.object_map_info()
            twin = object_map_of(planes[:m], rects[:m], idx, lw)
            jt.check(dev, twin, n, note=worst, what=name)
            live = np.unique(np.arange(n) if idx is None else idx) if lw is None else np.unique((np.arange(n) if idx is None else idx)[np.isfinite(lw)])
            assert info["live"] == live.size, pname
            want, tiles = _documented_groups(info["live"], info["rect"], rows, cols, B)
            assert (info["groups"], info["tiles"]) == (want, tiles), (pname, info)
            groups.add(info["groups"])
            if n == 300 and idx is None:
                assert tiles >= 4 and info["rect"][2] - info["rect"][0] > 32 and info["rect"][3] - info["rect"][1] > info["tile_px"] // 32, info
                again = g.object_map(poses[:m], idx, lw)
                assert all(a.tobytes() == b.tobytes() for a, b in zip(dev, again)), "two calls, other bits"
        assert g.object_map_ms() > 0.0
    assert 1 in groups and max(groups) > 1, groups                        # one part and several parts both ran
    print("worst share of a bar so far:", worst)


def test_sensor_is_left_alone_and_the_calls_that_follow_give_the_bits_of_a_handle_that_never_asked(gpu_lib):
    om, cam, P, poses, _ = _case("one_body_80x60")
    N = 24

    def drive(ask):
        rng, frng = np.random.default_rng(3), np.random.default_rng(9)
        lls, seen = [], None
        with RbSensor(om, cam, P, max_particles=N) as g:
            for k in range(5):
                if k == 3:
                    before = ([g.get_window(s) for s in range(N)], g.shared_trail_state(), g.get_poses(N).tobytes(), g.get_observation().tobytes(),
                              g.render_depth(synth.truth_pose(1, frame=2)).tobytes(), g.get_background())
                    if ask:
                        g.object_map(poses[:65], None, None)
                        g.object_map(poses[:40], np.arange(90, dtype=np.int32) % 40, np.random.default_rng(1).normal(0, 2, 90))
                        g.object_segment()
                    after = ([g.get_window(s) for s in range(N)], g.shared_trail_state(), g.get_poses(N).tobytes(), g.get_observation().tobytes(),
                             g.render_depth(synth.truth_pose(1, frame=2)).tobytes(), g.get_background())
                    assert before == after, "the map moved something of the sensor"
                g.set_observation(synth.make_frame(g.render_depth(synth.truth_pose(1, frame=k)), 60, 80, frng, occluder=True))
                parents = np.sort(rng.integers(0, N, N)).astype(np.int32) if k else np.arange(N, dtype=np.int32)
                lls.append(g.loglikes_poses(synth.particle_poses(synth.truth_pose(1, frame=k), N, rng, scale=2.0), parents, update=True))
            seen = ([g.get_window(s) for s in range(N)], [g.get_occlusion(s).tobytes() for s in (0, 5, N - 1)])
        return lls, seen

    (lla, sa), (llb, sb) = drive(True), drive(False)
    for k, (x, y) in enumerate(zip(lla, llb)):
        assert np.isfinite(x).all() and x.tobytes() == y.tobytes(), k
    assert sa == sb


def test_sensor_level_refusals_in_their_order(gpu_lib):
    om, cam, P, poses, _ = _case("one_body_80x60")
    inv, uns = _capi.RBS_ERR_INVALID_ARGUMENT, _capi.RBS_ERR_UNSUPPORTED

    def refused(code, fn, word=None):
        with pytest.raises(RbSensorError) as e:
            fn()
        assert e.value.code == code and (word is None or word in str(e.value)), (e.value.code, str(e.value))

    two = np.array([0, 1], np.int32)
    nanpose = poses[:2].copy()
    nanpose[1, 0, 3] = np.nan
    with RbSensor(om, cam, P, max_particles=4) as g:
        refused(inv, g.object_map_ms)                                                       # no map yet
        refused(inv, g.object_map_info)
        refused(inv, lambda: g.object_map(np.zeros((0, 1, 12))), "n < 1")
        refused(inv, lambda: g.object_map(poses[:2], np.zeros(0, np.int32)), "n < 1")
        refused(inv, lambda: g.object_map(poses[:2], np.array([0, 2], np.int32)), "pose index")
        refused(inv, lambda: g.object_map(poses[:2], np.array([-1], np.int32)), "pose index")
        refused(inv, lambda: g.object_map(poses[:2], two, np.array([0.0, np.nan])), "log-weight")
        refused(inv, lambda: g.object_map(poses[:2], two, np.array([0.0, np.inf])), "log-weight")
        refused(inv, lambda: g.object_map(poses[:2], two, np.array([-np.inf, -np.inf])), "-inf")
        refused(inv, lambda: g.object_map(nanpose), "not finite")
        # the order: a bad index is named before a bad weight, a bad weight before a bad pose
        refused(inv, lambda: g.object_map(nanpose, np.array([0, 9], np.int32), np.array([0.0, np.nan])), "pose index")
        refused(inv, lambda: g.object_map(nanpose, two, np.array([0.0, np.nan])), "log-weight")
        lib, h = g._lib, g._h
        out = (C.c_float * (80 * 60))()
        assert lib.rbs_object_map(h, None, 1, None, None, 1, out, out, out) == inv            # a null pointer
        # -inf alone is a member without weight; every output may be NULL
        one = g.object_map(poses[:2], two, np.array([-np.inf, 0.0]))
        alone = g.object_map(poses[1:2])
        assert all(a.tobytes() == b.tobytes() for a, b in zip(one, alone))
        p2 = np.ascontiguousarray(poses[:2])
        assert lib.rbs_object_map(h, p2.ctypes.data_as(C.POINTER(C.c_double)), 2, None, None, 2, None, None, None) == 0
        # segmentation: parameters, capacity, then "no observation"
        refused(inv, lambda: g.object_segment(params=dict(min_cover=1.5)))
        refused(inv, lambda: g.object_segment(params=dict(sigmas=0.0)))
        refused(inv, lambda: g.object_segment(params=dict(depth_sigmas=float("nan"))))
        refused(inv, lambda: g.object_segment(capacity=-1))
        refused(inv, lambda: g.object_segment(), "no observation")
        g.set_observation(np.full(80 * 60, 0.7, np.float32))
        g.object_segment()                                                                 # the maps of the last object_map, on the device
        g.object_segment(one)                                                              # host maps replace them ...
        refused(inv, lambda: g.object_segment(), "no rbs_object_map")                      # ... and are not "the last object_map's"
    with RbSensor(om, cam, P, max_particles=4) as g:
        g.set_observation(np.full(80 * 60, 0.7, np.float32))
        refused(inv, lambda: g.object_segment(), "no rbs_object_map")
    with RbSensor(om, cam, P, max_particles=4, precision="f64", device_ids=[0, 0]) as grp:      # several shards: ahead of everything the
        refused(uns, lambda: grp.object_map(poses[:2], np.array([0, 9], np.int32)), "single-device")   # checks on indices, weights and poses
        refused(uns, lambda: grp.object_segment(), "single-device")
    om9, cam9, P9 = sc.make_scene(("box12",) * 9, 80, 60, max_particles=2)
    with RbSensor(om9, cam9, P9, max_particles=2) as g9:
        refused(uns, lambda: g9.object_map(np.tile(synth.truth_pose(9), (1, 1, 1))), "n_objects")
        refused(uns, lambda: g9.object_segment(), "n_objects")


# ---------------------------------------------------------------- rbs_object_segment
def _segment_case(name):
    om, cam, P, _, _ = _case(name)
    meshes, cols, rows = CASES[name]
    B = len(meshes)
    rng = np.random.default_rng(31)
    truth = synth.truth_pose(B, frame=1)
    return om, cam, P, B, rows, cols, truth, synth.particle_poses(truth, 64, rng, scale=1.5), rng.normal(0.0, 1.0, 64)


@pytest.mark.parametrize("name", list(CASES))
def test_segmentation_is_segment_of_over_the_devices_own_maps(gpu_lib, name):
    om, cam, P, B, rows, cols, truth, poses, lw = _segment_case(name)
    K = np.asarray(cam.camera_matrix, dtype=np.float64).reshape(3, 3)
    with RbSensor(om, cam, P, max_particles=4) as g:
        depth_truth = g.render_depth(truth)
        frame = synth.make_frame(depth_truth, rows, cols, np.random.default_rng(7), occluder=True)
        g.set_observation(frame)
        y = g.get_observation()
        maps = g.object_map(poses, None, lw)
        for params in (None, dict(min_cover=0.9, sigmas=1.0, depth_sigmas=1.0), dict(min_cover=0.0, depth_sigmas=0.0)):
            from_device = g.object_segment(None, params) if params is None else None
            labels, counts, pixel, xyz, n_points = g.object_segment(maps, params)
            kw = dict(RbSensor.object_segment_default_params(), **(params or {}))
            want = segment_of(maps[0].reshape(B, rows, cols), maps[1], maps[2], y, K, P.kinect.model_sigma, P.kinect.sigma_factor, **kw)
            assert np.array_equal(labels, want[0]) and np.array_equal(counts, want[1]), params
            assert n_points == want[2].size and np.array_equal(pixel, want[2]), params
            assert xyz.tobytes() == want[3].tobytes(), params                       # bit for bit
            if from_device is not None:                                              # the maps still on the device: the same answer
                assert all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(from_device, (labels, counts, pixel, xyz)))
                maps_again = g.object_map(poses, None, lw)                          # (put them back for the next round's comparison)
                assert all(a.tobytes() == b.tobytes() for a, b in zip(maps, maps_again))
        labels, counts, pixel, xyz, n_points = g.object_segment(maps)
        assert n_points > 20 and counts.sum() == n_points and (counts > 0).all()
        # the occluder slab (0.5 m, in front of the object at 0.7 m) over part of the object: those pixels are not the object
        slab = np.isfinite(depth_truth) & (y < depth_truth - 0.1)
        assert slab.sum() > 5 and (labels[slab] == -1).all()
        # capacity smaller than the count: the full count is reported, nothing is written past capacity, RBS_OK
        cap = 5
        pix = np.full(n_points + 8, -7, np.int32)
        pts = np.full((n_points + 8, 3), -7.0, np.float32)
        npts = C.c_int32()
        fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
        rc = g._lib.rbs_object_segment(g._h, None, maps[0].ctypes.data_as(fp), maps[1].ctypes.data_as(fp), maps[2].ctypes.data_as(fp), None, None,
                                       pix.ctypes.data_as(ip), pts.ctypes.data_as(fp), cap, C.byref(npts))
        assert rc == 0 and npts.value == n_points
        assert np.array_equal(pix[:cap], pixel[:cap]) and pts[:cap].tobytes() == xyz[:cap].tobytes()
        assert (pix[cap:] == -7).all() and (pts[cap:] == -7.0).all()
        g.object_map(poses, None, lw)                       # the maps on the device again; every output NULL but the count
        assert g._lib.rbs_object_segment(g._h, None, None, None, None, None, None, None, None, 0, C.byref(npts)) == 0 and npts.value == n_points


# ---------------------------------------------------------------- the tracker itself
_runs = {}


def _run(n, max_kl=2.0, again=0, **kw):
    key = (n, max_kl, again, tuple(sorted(kw.items())))
    if key not in _runs:
        _runs[key] = wk.run(n, max_kl, **kw)
    return _runs[key]


def _same_maps(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in ("cover", "depth", "var", "map_frames"))


SIZES = pytest.mark.parametrize("n", [300, 600, 8200], ids=["fused_300", "tail_600", "grid_8200"])


@pytest.mark.parametrize("max_kl", [0.0, 1e9], ids=["always_resamples", "never_resamples"])
@SIZES
def test_tracker_poses_and_map_match_the_twin(gpu_lib, n, max_kl):
    r = wk.run(n, max_kl, states=True, planes_of_last=True)           # (not kept: 8 200 planes where nothing resamples)
    for k in range(wk.FRAMES):
        assert np.abs(r["poses"][k] - r["host_poses"][k]).max() <= 1e-12, k        # a wrong gather would be off by a particle's spread
        assert r["map_frames"][k] == k + 1 and r["depth"][k].shape == (wk.ROWS, wk.COLS)
    distinct = r["planes"].shape[0]
    assert distinct < n if max_kl == 0.0 else distinct == n
    rects = np.tile(np.array([0, 0, wk.COLS, wk.ROWS]), (distinct, 1, 1))
    twin = object_map_of(r["planes"], rects, r["plane_members"], r["last_log_weights"])
    jt.check((r["cover"][-1], r["depth"][-1], r["var"][-1]), twin, n, note=worst, what="tracker")
    assert np.isfinite(r["depth"][-1]).sum() > 20 and r["cover"][-1].max() > 0.5
    print("worst share of a bar so far:", worst)


@SIZES
def test_filter_is_unchanged_by_the_map(gpu_lib, n):
    """Estimates, particles, weights, slot maps and resamplings with the map on are those of a tracker without it -- also beside
    the posterior report and the occlusion map, whose own numbers do not move either."""
    on, off = _run(n, states=True), _run(n, object_map=False, states=True)
    assert "cover" in on and "cover" not in off
    for k in ("estimates", "particles", "log_weights", "indices", "resamplings"):
        assert on[k].tobytes() == off[k].tobytes(), k
    both, others = _run(n, posterior=True, occlusion_map=True), _run(n, object_map=False, posterior=True, occlusion_map=True)
    for k in ("estimates", "resamplings", "post_mean", "occ"):
        assert both[k].tobytes() == others[k].tobytes() and (k in ("post_mean", "occ") or both[k].tobytes() == off[k].tobytes()), k
    assert _same_maps(on, both)
    assert on["resamplings"][-1] >= 1


@SIZES
def test_look_ahead_gives_the_maps_of_frame_by_frame(gpu_lib, n):
    """Two frames in flight: result(k)'s map is frame k's while k + 1 is in flight -- whose transition overwrites the poses the
    map was drawn from, behind it in stream order."""
    a, b = _run(n), _run(n, look_ahead=True)
    assert a["estimates"].tobytes() == b["estimates"].tobytes()
    assert b["map_frames"].tolist() == list(range(1, wk.FRAMES + 1))
    assert _same_maps(a, b)
    assert _same_maps(a, _run(n, posterior=True, occlusion_map=True, look_ahead=True))


def test_two_runs_give_the_same_bits(gpu_lib):
    for n in (600, 8200):
        assert _same_maps(_run(n), _run(n, again=1)), n


def test_tracker_refusals(gpu_lib):
    n = 64
    om, cam, P = sc.make_scene(("m1_l2",), wk.COLS, wk.ROWS, max_particles=n)
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
        refused(inv, dev.poses)                               # no frame yet
        frames = wk.scene_frames(s, 3)
        dev.track(frames[0])
        refused(inv, dev.object_map)                          # the map is off
        refused(inv, dev.object_map_ms)
        dev.set_object_map(True)
        refused(inv, dev.object_map)                          # on, but no frame has been handed out since
        dev.track(frames[1])
        assert dev.object_map().frame == 2
        dev.initialize([wk.initial_state(om)])
        refused(inv, dev.object_map)                          # after initialize, before the next result
        dev.submit(frames[0])
        refused(inv, lambda: dev.set_object_map(False))       # a frame in flight
        refused(inv, dev.object_map)
        refused(inv, dev.poses)                               # no snapshot: refused with a frame in flight
        dev.result()
        m = dev.object_map()
        assert m.frame == 1 and m.cover.shape == (1, wk.ROWS, wk.COLS) and m.depth.shape == (wk.ROWS, wk.COLS)
        assert dev.object_map_ms() > 0.0
        p, w, i = dev.get_state()
        again = s.object_map(dev.poses(), None, w)            # the sensor-level call over the same population: the same sums
        ref = wk.reference_planes(s, dev.poses())
        twin = object_map_of(ref, np.tile(np.array([0, 0, wk.COLS, wk.ROWS]), (n, 1, 1)), None, w)
        jt.check(again, twin, n, what="sensor call on the tracker's population")
        jt.check((m.cover, m.depth, m.var), twin, n, what="tracker")
        seg = dev.segment()
        assert seg.labels.shape == (wk.ROWS, wk.COLS) and seg.counts.sum() == seg.pixel.size == (seg.labels >= 0).sum()
        dev.set_object_map(False)
        dev.track(frames[1])
        refused(inv, dev.object_map)                          # off again
        dev.set_object_map(True)
        dev.set_posterior(True)
        dev.set_occlusion_map(True)                           # any of the three, all or none
        dev.track(frames[2])
        assert dev.object_map().frame == 3 and dev.posterior().frame == 3 and dev.occlusion_map().frame == 3
        frame = C.c_int32()
        assert dev._lib.rbs_tracker_object_map(dev._t, None, None, None, None) == 0           # NULL outputs are allowed, one by one
        assert dev._lib.rbs_tracker_object_map(dev._t, C.byref(frame), None, None, None) == 0 and frame.value == 3
        dev.close()
    with RbSensor(om, cam, P, max_particles=n, precision="f64", device_ids=[0, 0]) as grp:      # a tracker over several shards
        dev = DeviceParticleTracker(trans, grp, om, tp, np.random.default_rng(5))
        refused(_capi.RBS_ERR_UNSUPPORTED, lambda: dev.set_object_map(True))
        refused(_capi.RBS_ERR_UNSUPPORTED, dev.poses)
        dev.close()


def test_poisoned_tracker_refuses_the_map_first(gpu_lib):
    """In a process of its own that loads the hooks build, where the injected fault exists (tests/object_map_worker.py)."""
    import filter_probes as fp
    hooks = fp.hooks_path(_capi.LIB_PATH)
    assert os.path.exists(hooks), "build() makes librbsensor_mi355x_hooks.so"
    r = subprocess.run([sys.executable, os.path.join(HERE, "object_map_worker.py"), "poisoned"], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, RBS_LIB_PATH=hooks))
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1] == "POISONED_OK", (r.stdout[-2000:], r.stderr[-2000:])


# ---------------------------------------------------------------- end to end
def _iou(a, b):
    return float((a & b).sum()) / float(max(1, (a | b).sum()))


@pytest.mark.parametrize("occluder", [False, True], ids=["clear", "slab"])
def test_twenty_frames_segment_the_object(gpu_lib, occluder):
    """200 particles, 80 x 60, twenty frames.  The truth pose's silhouette under the last frame: rendered with rbs_render_depth
    and classed with the segmentation's tau (the pixels where the frame agrees with the truth surface).  The expected
    intersection-over-union is the TWIN's: segment_of over object_map_of on the same population; the device's labels may
    differ from those only where a float map sits within its bar of a threshold, so the two values are asked to agree to
    two pixels of the union.  Measured values: DESIGN.md Appendix O."""
    r = wk.run(200, frames=20, occluder=occluder, planes_of_last=True)
    rows, cols = wk.ROWS, wk.COLS
    ms, sf = r["kinect"]
    y = np.asarray(r["frames"][-1], dtype=np.float32).ravel()
    D = np.asarray(r["truth_depth"], dtype=np.float32).ravel().astype(np.float64)
    sig = RbSensor.object_segment_default_params()["sigmas"]
    with np.errstate(invalid="ignore"):
        truth = np.isfinite(D) & np.isfinite(y) & (np.abs(y.astype(np.float64) - D) <= sig * (ms + sf * D * D))
    seg = r["segment"]
    dev = seg.labels.ravel() >= 0
    planes = r["planes"]
    rects = np.tile(np.array([0, 0, cols, rows]), (planes.shape[0], 1, 1))
    tc, td, tv, _, _ = object_map_of(planes, rects, r["plane_members"], r["last_log_weights"])
    want = segment_of(tc.astype(np.float32).reshape(1, rows, cols), td.astype(np.float32), tv.astype(np.float32), y, r["K"], ms, sf,
                      **RbSensor.object_segment_default_params())
    twin = want[0] >= 0
    iou_dev, iou_twin = _iou(dev, truth), _iou(twin, truth)
    print("IoU with the truth silhouette (%s): device %.4f, twin %.4f; labelled %d, truth %d" % ("slab" if occluder else "clear", iou_dev, iou_twin,
                                                                                               int(dev.sum()), int(truth.sum())))
    union = max(1, int((twin | truth).sum()))
    assert truth.sum() > 20 and twin.sum() > 0
    assert abs(iou_dev - iou_twin) <= 2.0 / union, (iou_dev, iou_twin)
    assert int((dev != twin).sum()) <= 2
    if occluder:
        slab = np.isfinite(D) & (y < D - 0.1)
        assert slab.sum() > 3 and not dev[slab].any()


# ---------------------------------------------------------------- the host tracker, the C++ mirror, the node assembly
def test_host_tracker_asks_the_sensor_with_its_own_population(gpu_lib):
    from dbot_ros_amd.tracker import ParticleTracker
    n = 32
    om, cam, P = sc.make_scene(("m1_l2",), wk.COLS, wk.ROWS, max_particles=n)
    tp = ParticleTrackerBuilder.Parameters(evaluation_count=n)
    trans = ObjectTransitionBuilder(ObjectTransitionBuilder.Parameters()).build()
    with RbSensor(om, cam, P, max_particles=n) as s:
        tr = ParticleTracker(trans, s, om, tp, np.random.default_rng(5))
        tr.initialize([wk.initial_state(om)])
        with pytest.raises(ValueError):
            tr.object_map()
        for f in wk.scene_frames(s, 2):
            tr.track(f)
        m = tr.object_map()
        assert m.frame == 2 and m.cover.shape == (1, wk.ROWS, wk.COLS)
        planes = wk.reference_planes(s, tr.poses())
        twin = object_map_of(planes, np.tile(np.array([0, 0, wk.COLS, wk.ROWS]), (n, 1, 1)), None, tr.log_weights)
        jt.check((m.cover, m.depth, m.var), twin, n, note=worst, what="host tracker")
        seg = tr.segment()
        assert seg.counts.sum() == seg.pixel.size > 20


def test_cpp_mirror_prints_pythons_bits(gpu_lib, tmp_path):
    import struct
    from dbot_ros_amd import CameraData, ObjectModel, RbSensorBuilder
    exe = str(tmp_path / "object_map_check")
    lib = os.path.join(ROOT, "dbot_ros_amd", "lib")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(HERE, "cpp", "object_map_check.cpp"), "-L" + lib, "-lrbsensor_mi355x", "-Wl,-rpath," + lib,
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
        dev = DeviceParticleTracker(trans, s, om, tp, device_rng=True, seed=11, object_map=True)
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
            got.append(dev.object_map())
        s.object_map(dev.poses())
        seg = s.object_segment()
        dev.close()
    run = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.returncode, run.stdout[-2000:], run.stderr[-2000:])
    lines = run.stdout.strip().split("\n")
    assert len(lines) == 2 * count + 2, run.stdout[-2000:]
    for k, m in enumerate(got):
        assert lines[2 * k].split() == ["FRAME", str(k), str(m.frame)] and m.frame == k + 1
        vals = np.array([float.fromhex(v) for v in lines[2 * k + 1].split()]).astype(np.float32)
        mine = np.concatenate([m.cover.ravel(), m.depth.ravel(), m.var.ravel()])
        assert np.array_equal(vals.view(np.uint32), mine.view(np.uint32)), k
    assert got[-1].cover.max() > 0.5
    assert lines[2 * count] == "SENSOR same"
    assert lines[2 * count + 1].split() == ["SEGMENT", str(seg[4]), str(int(seg[1][0]))] and seg[4] > 20


def test_node_replay_hands_out_the_maps(gpu_lib, tmp_path):
    """replay_dataset(object_map=True) additionally returns every frame's maps -- last, behind the posterior reports and the
    occlusion maps when those are asked for, look-ahead the same bits -- and leaves its return value alone with the flag off; the
    YAML key particle_filter/object_map switches the map on by itself."""
    import test_node as tn
    from dbot_ros_amd import CameraData, ObjectModel, RbSensorBuilder, dataset as ds, node, objloader, pose
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
    on = node.replay_dataset(tree, data, str(tmp_path), [truth_state(0)], seed=3, object_map=True)
    ahead = node.replay_dataset(tree, data, str(tmp_path), [truth_state(0)], seed=3, object_map=True, look_ahead=True)
    every = node.replay_dataset(tree, data, str(tmp_path), [truth_state(0)], seed=3, posterior=True, occlusion_map=True, object_map=True)
    assert len(off) == 2 and len(on) == 3 and len(ahead) == 3 and len(every) == 5
    assert np.array_equal(off[0], on[0]) and np.array_equal(on[0], ahead[0]) and np.array_equal(on[0], every[0])
    assert [m.frame for m in on[2]] == [1, 2, 3]
    for a, b, c in zip(on[2], ahead[2], every[4]):
        for k in ("cover", "depth", "var"):
            assert getattr(a, k).tobytes() == getattr(b, k).tobytes() and getattr(a, k).tobytes() == getattr(c, k).tobytes()
    assert on[2][-1].cover.max() > 0.5
    tree["particle_filter"]["object_map"] = True
    keyed = node.replay_dataset(tree, data, str(tmp_path), [truth_state(0)], seed=3)
    assert len(keyed) == 2 and np.array_equal(keyed[0], off[0])                 # the flag off: the return value stays as it is
    tracker, _, _, _ = node.build_particle_tracker(tree, K, str(tmp_path), seed=3)
    try:
        tracker.initialize([truth_state(0)])
        tracker.track(data.frame_vector(0, int(tree["downsampling_factor"])))
        assert tracker.object_map().depth.tobytes() == on[2][0].depth.tobytes()      # ... but the key has switched the map on
    finally:
        tracker.close()
        tracker.sensor.close()
