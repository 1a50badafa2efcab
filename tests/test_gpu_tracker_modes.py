"""The posterior modes ON THE DEVICE (dbot_ros_amd/csrc/rbsensor_modes.hip; rbs_pose_modes, rbs_tracker_set_modes /
rbs_tracker_modes): the stateless entry on the planted populations of tests/modes_twin.py at every size where the launch
geometry changes, the tracker itself on every route against the rule applied to get_state(), the unchanged filter,
look-ahead, determinism, pending against immediate re-centring, the posterior report beside it, the refusals, and the C++
mirror.  Bars and margins: tests/modes_twin.py (derived, not tuned); seeds and mode counts must match exactly."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import modes_twin as mt
import scenarios as sc
import tracker_modes_worker as wk
from dbot_ros_amd import CameraData, ObjectModel, RbSensor, RbSensorBuilder, RbSensorError, _capi
from dbot_ros_amd.tracker import DeviceParticleTracker, ModesParams, ObjectTransitionBuilder, ParticleTrackerBuilder, modes_of, modes_params_c

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
# wave, tile and block edges; 1 024 | 1 025 and 4 096 | 4 097: the j-split's part length changes (64 -> 256 -> 1 024 records);
# 4 096 | 4 097 and 8 192 | 8 193: one more chunk of the assignment's means
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1025]
EDGES = [1024, 4095, 4096, 4097, 8191, 8192, 8193]
MAX_N = 8200
worst = {}
_sensors = {}


@pytest.fixture(scope="module")
def sensors(gpu_lib):
    """One small sensor per body count, shared by the stateless tests (the modes do not look at the image)."""
    def get(parts):
        if parts not in _sensors:
            om, cam, P = sc.make_scene(("m1_l2", "box12", "m1_l2")[:parts], 32, 24, max_particles=MAX_N)
            _sensors[parts] = RbSensor(om, cam, P, max_particles=MAX_N)
        return _sensors[parts]
    yield get
    for s in _sensors.values():
        s.close()
    _sensors.clear()


def _patterns(parts):
    return mt.PATTERNS + ((mt.BODIES_123,) if parts == 3 else ())


# ---------------------------------------------------------------- the stateless entry on planted populations
@pytest.mark.parametrize("parts", [1, 2, 3])
@pytest.mark.parametrize("n", SIZES)
def test_pose_modes_on_planted_populations(sensors, n, parts):
    s = sensors(parts)
    for pattern in _patterns(parts):
        x, lw, P, ref = mt.planted(pattern, n, parts)
        got = s.pose_modes(x, lw, P)
        mt.check(got, ref, note=worst)
        assert mt.same_bits(got, s.pose_modes(x, lw, P)), pattern          # two runs, the same bits
        mt.assert_pattern(pattern, n, got)
    print("worst share of the bars so far:", worst)


@pytest.mark.parametrize("n", EDGES)
def test_pose_modes_either_side_of_a_geometry_change(sensors, n):
    """One body, the patterns that load every j-part and every chunk (members of all clusters are spread over the index
    range), and three bodies at the part-length edges."""
    for parts, patterns in ((1, ("many", "beyond_pi")), (3, (mt.BODIES_123,) if n <= 4097 else ())):
        for pattern in patterns:
            x, lw, P, ref = mt.planted(pattern, n, parts)
            got = sensors(parts).pose_modes(x, lw, P)
            mt.check(got, ref, note=worst)
            assert mt.same_bits(got, sensors(parts).pose_modes(x, lw, P))
    print("worst share of the bars so far:", worst)


def test_pose_modes_with_other_parameters(sensors):
    """k_max 1 and 8, a wide and a narrow kernel: the truncation and the masses' sum."""
    x, lw, _, _ = mt.planted("many", 257, 1)
    for P in (ModesParams(k_max=1), ModesParams(k_max=8), ModesParams(h_t=0.05, h_r=1.0, separation=1.0, k_max=3),
              ModesParams(h_t=0.004, h_r=0.05, separation=3.5, k_max=8)):
        ref = mt.reference(x, lw, P)
        assert min(b["margin"] for b in ref["bodies"]) >= mt.MARGIN
        got = sensors(1).pose_modes(x, lw, P)
        mt.check(got, ref, note=worst)
        assert len(got.bodies[0]) <= P.k_max and abs(sum(m.mass for m in got.bodies[0]) - 1.0) <= 8 * 257 * mt.U * P.k_max


def test_pose_modes_weights_below_the_cut_are_no_belief(sensors):
    """A second cluster 640 log units down (e ~ 1e-278) is a mode, to the bars; 690 down (below 2^-960) it is none."""
    for n in (257, 1025):
        x, lw, P, ref = mt.faint(n, -640.0)
        got = sensors(1).pose_modes(x, lw, P)
        mt.check(got, ref, note=worst)
        assert len(got.bodies[0]) >= 2 and 0.0 < got.bodies[0][1].mass < 1e-270
        x, lw, P, ref = mt.faint(n, -690.0)
        got = sensors(1).pose_modes(x, lw, P)
        mt.check(got, ref, note=worst)
        assert not [m for m in got.bodies[0] if x[m.seed, 0, 0] > 5 * P.h_t]


def test_pose_modes_refusals(sensors):
    s = sensors(2)
    x, lw, P, _ = mt.planted("two", 64, 2)

    def refused(code, fn):
        with pytest.raises(RbSensorError) as e:
            fn()
        assert e.value.code == code, (e.value.code, str(e.value))

    for bad in (ModesParams(h_t=0.0), ModesParams(h_t=-1.0), ModesParams(h_t=np.inf), ModesParams(h_r=0.0), ModesParams(h_r=1.0001),
                ModesParams(h_r=np.nan), ModesParams(separation=0.99), ModesParams(k_max=0), ModesParams(k_max=9)):
        refused(_capi.RBS_ERR_INVALID_ARGUMENT, lambda: s.pose_modes(x, lw, bad))
    big = np.zeros((MAX_N + 1, 2, 6))
    refused(_capi.RBS_ERR_INVALID_ARGUMENT, lambda: s.pose_modes(big, np.zeros(MAX_N + 1), P))            # above max_particles
    refused(_capi.RBS_ERR_INVALID_ARGUMENT, lambda: s.pose_modes(x, np.full(64, -np.inf), P))
    refused(_capi.RBS_ERR_INVALID_ARGUMENT, lambda: s.pose_modes(x, np.r_[np.nan, lw[1:]], P))
    refused(_capi.RBS_ERR_INVALID_ARGUMENT, lambda: s.pose_modes(np.where(np.arange(6) == 2, np.inf, x), lw, P))
    import ctypes as C
    rec = (_capi.RbsBodyModes * 2)()
    c = modes_params_c(P)
    dp = C.POINTER(C.c_double)
    xs, lws = np.ascontiguousarray(x), np.ascontiguousarray(lw)
    assert s._lib.rbs_pose_modes(s._h, xs.ctypes.data_as(dp), lws.ctypes.data_as(dp), 0, C.byref(c), rec) == _capi.RBS_ERR_INVALID_ARGUMENT   # n < 1
    assert s._lib.rbs_pose_modes(s._h, None, lws.ctypes.data_as(dp), 64, C.byref(c), rec) == _capi.RBS_ERR_INVALID_ARGUMENT
    assert s._lib.rbs_pose_modes(s._h, xs.ctypes.data_as(dp), lws.ctypes.data_as(dp), 64, None, rec) == _capi.RBS_ERR_INVALID_ARGUMENT
    om, cam, Pm = sc.make_scene(("m1_l2",), 32, 24, max_particles=64)
    with RbSensor(om, cam, Pm, max_particles=64, precision="f64", device_ids=[0, 0]) as grp:                 # a handle over several shards
        x1, lw1, _, _ = mt.planted("two", 64, 1)
        refused(_capi.RBS_ERR_UNSUPPORTED, lambda: grp.pose_modes(x1, lw1, P))
    assert mt.same_bits(s.pose_modes(x, lw, P), s.pose_modes(x, lw, P))                                      # the handle is as good as before


# ---------------------------------------------------------------- the tracker itself
_runs = {}
ROUTES = dict(argnames="n", argvalues=[300, 600, 8200], ids=["fused_300", "tail_600", "grid_8200"])


def _run(n, max_kl=2.0, modes=True, posterior=False, look_ahead=False, again=0, parts=1):
    key = (n, max_kl, modes, posterior, look_ahead, again, parts)
    if key not in _runs:
        _runs[key] = wk.run(n, max_kl, modes, posterior, look_ahead, parts=parts)
    return _runs[key]


def _modes_equal(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in ("n_modes", "table", "mode_frame", "mode_pose"))


@pytest.mark.parametrize("max_kl", [0.0, 1e9], ids=["always_resamples", "never_resamples"])
@pytest.mark.parametrize(**ROUTES)
def test_tracker_modes_match_the_rule_on_get_state(gpu_lib, n, max_kl):
    """Every one of the six frames against the rule by brute force on that frame's get_state(); the numpy twin's seeds beside it
    (at 8 200 particles on the first and last frame: its binary64 pair pass takes three seconds a frame, and what it is compared
    with -- the reference -- is there on every frame)."""
    r = _run(n, max_kl)
    P = ModesParams()
    for k in range(wk.FRAMES):
        x = r["particles"][k].reshape(n, 1, 12)
        got = mt.unpack(r["n_modes"][k], r["table"][k], r["mode_frame"][k])
        assert got.frame == k + 1 and 1 <= len(got.bodies[0]) <= P.k_max
        assert abs(sum(m.mass for m in got.bodies[0]) - 1.0) <= 8 * n * mt.U * P.k_max
        mt.check(got, mt.reference(x, r["log_weights"][k], P), note=worst)
        if n < 8000 or k in (0, wk.FRAMES - 1):
            twin = modes_of(x, r["log_weights"][k], P)
            assert [m.seed for m in twin.bodies[0]] == [m.seed for m in got.bodies[0]]
    print("worst share of the bars so far:", worst)


@pytest.mark.parametrize("max_kl", [0.0, 1e9], ids=["always_resamples", "never_resamples"])
def test_tracker_modes_of_three_bodies_match_the_rule_on_get_state(gpu_lib, max_kl):
    """Three bodies of 600 particles (the tail route: the re-centring is pending, so the pack kernel re-centres every body's
    copy): the particles' stride of 36, the bodies' offset of 12 and the mean rotation of bodies 1 and 2."""
    n, parts = 600, 3
    r = _run(n, max_kl, parts=parts)
    P = ModesParams()
    for k in range(wk.FRAMES):
        x = r["particles"][k].reshape(n, parts, 12)
        got = mt.unpack(r["n_modes"][k], r["table"][k], r["mode_frame"][k])
        assert got.frame == k + 1 and len(got.bodies) == parts
        mt.check(got, mt.reference(x, r["log_weights"][k], P), note=worst)
        twin = modes_of(x, r["log_weights"][k], P)
        assert [[m.seed for m in b] for b in twin.bodies] == [[m.seed for m in b] for b in got.bodies]
    assert np.abs(r["particles"][-1].reshape(n, parts, 12)[:, 1:, 0:6]).max() > 0          # (the other bodies do move)
    print("worst share of the bars so far:", worst)


@pytest.mark.parametrize(**ROUTES)
def test_filter_is_unchanged_by_the_modes(gpu_lib, n):
    on, off = _run(n), _run(n, modes=False)
    assert "table" in on and "table" not in off
    for k in ("estimates", "particles", "log_weights", "indices", "resamplings"):
        assert on[k].tobytes() == off[k].tobytes(), k


@pytest.mark.parametrize(**ROUTES)
def test_look_ahead_gives_the_modes_of_frame_by_frame(gpu_lib, n):
    a, b = _run(n), _run(n, look_ahead=True)
    assert a["estimates"].tobytes() == b["estimates"].tobytes()
    assert [int(v) for v in b["mode_frame"]] == list(range(1, wk.FRAMES + 1))
    assert _modes_equal(a, b)


def test_two_runs_give_the_same_bits(gpu_lib):
    for n in (300, 600, 8200):
        assert _modes_equal(_run(n), _run(n, again=1)), n


@pytest.mark.parametrize(**ROUTES)
def test_modes_and_posterior_leave_each_other_alone(gpu_lib, n):
    both, modes_only, post_only = _run(n, posterior=True), _run(n), _run(n, modes=False, posterior=True)
    assert _modes_equal(both, modes_only)
    for k in ("ess", "mean", "cov", "estimates"):
        assert both[k].tobytes() == post_only[k].tobytes(), k


def test_published_pose_is_the_delta_on_the_frames_state(gpu_lib):
    """Mode.pose: the mode's delta composed with the frame's state and published as the tracker publishes its estimate -- a
    zero delta is the estimate itself, and the heaviest mode of a single tight cloud lies beside it."""
    r = _run(600)
    om, cam, P = sc.make_scene(("m1_l2",), wk.COLS, wk.ROWS, max_particles=8)
    tp = ParticleTrackerBuilder.Parameters(evaluation_count=8)
    trans = ObjectTransitionBuilder(ObjectTransitionBuilder.Parameters()).build()
    from dbot_ros_amd.tracker import Mode, Modes, ParticleTracker
    host = ParticleTracker(trans, None, om, tp)
    for k in range(wk.FRAMES):
        z = r["defaults"][k]
        zero = host._with_poses(Modes(bodies=[[Mode(0, 0.0, 0.0, 0.0, np.zeros(6))]]), z).bodies[0][0].pose
        assert np.abs(zero - host._from_model(z)[0:6]).max() <= 1e-15
        got = mt.unpack(r["n_modes"][k], r["table"][k])
        again = host._with_poses(got, z).bodies[0][0].pose
        assert again.tobytes() == r["mode_pose"][k].tobytes()
        assert np.abs(again[0:3] - zero[0:3]).max() < 0.05


_routes = {}


@pytest.mark.parametrize("n,parts", [(600, 1), (8200, 1), (600, 3)], ids=["tail_600", "grid_8200", "three_bodies_600"])
def test_pending_recentring_gives_the_bits_of_recentring_first(gpu_lib, tmp_path, n, parts):
    """RBS_TRACKER_RECENTRE_NOW=1 (read once per process: a child) re-centres the particles before the report's launches; by
    default the re-centring is pending and the pack kernel re-centres a register copy -- the same function, the same bits."""
    out = str(tmp_path / "run.npz")
    env = {k: v for k, v in os.environ.items() if not k.startswith("RBS_TRACKER_")}
    env["RBS_TRACKER_RECENTRE_NOW"] = "1"
    r = subprocess.run([sys.executable, os.path.join(HERE, "tracker_modes_worker.py"), out, str(n), str(parts)], capture_output=True, text=True,
                       timeout=120, env=env)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    got, ref = dict(np.load(out)), _run(n, parts=parts)
    for k in ("estimates", "particles", "log_weights", "indices"):
        assert ref[k].tobytes() == got[k].tobytes(), k
    assert _modes_equal(ref, got)


def test_tracker_refusals(gpu_lib):
    n = 64
    om, cam, P = sc.make_scene(("m1_l2",), wk.COLS, wk.ROWS, max_particles=n)
    tp = ParticleTrackerBuilder.Parameters(evaluation_count=n)
    trans = ObjectTransitionBuilder(ObjectTransitionBuilder.Parameters()).build()

    def refused(code, fn):
        with pytest.raises(RbSensorError) as e:
            fn()
        assert e.value.code == code, (e.value.code, str(e.value))

    with RbSensor(om, cam, P, max_particles=n) as s:
        dev = DeviceParticleTracker(trans, s, om, tp, np.random.default_rng(5))
        dev.initialize([wk.initial_state(om)])
        frames = wk.scene_frames(s, 3)
        dev.track(frames[0])
        refused(_capi.RBS_ERR_INVALID_ARGUMENT, dev.modes)                    # the report is off
        for bad in (ModesParams(h_t=0.0), ModesParams(h_r=2.0), ModesParams(separation=0.5), ModesParams(k_max=9)):
            refused(_capi.RBS_ERR_INVALID_ARGUMENT, lambda: dev.set_modes(bad))
        refused(_capi.RBS_ERR_INVALID_ARGUMENT, dev.modes)                    # ... and still off
        dev.set_modes(True)
        refused(_capi.RBS_ERR_INVALID_ARGUMENT, dev.modes)                    # on, but no frame has been handed out since
        refused(_capi.RBS_ERR_INVALID_ARGUMENT, dev.modes_ms)
        dev.track(frames[1])
        assert dev.modes().frame == 2
        dev.initialize([wk.initial_state(om)])
        refused(_capi.RBS_ERR_INVALID_ARGUMENT, dev.modes)                    # after initialize, before the next result
        dev.submit(frames[0])
        refused(_capi.RBS_ERR_INVALID_ARGUMENT, lambda: dev.set_modes(None))  # a frame in flight
        refused(_capi.RBS_ERR_INVALID_ARGUMENT, lambda: dev.set_modes(ModesParams(k_max=2)))
        refused(_capi.RBS_ERR_INVALID_ARGUMENT, dev.modes)
        dev.result()
        m = dev.modes()
        assert m.frame == 1 and 1 <= len(m.bodies[0]) <= 4 and m.bodies[0][0].pose.shape == (6,)
        assert 0.0 < dev.modes_ms() < 50.0                                    # the report's kernels' device time, from events
        dev.set_modes(ModesParams(k_max=1))                                   # new parameters, the buffers stay
        dev.track(frames[1])
        assert len(dev.modes().bodies[0]) == 1 and dev.modes().frame == 2
        dev.set_modes(None)
        dev.track(frames[2])
        refused(_capi.RBS_ERR_INVALID_ARGUMENT, dev.modes)                    # off again
        assert dev._lib.rbs_tracker_modes(dev._t, None, None) == _capi.RBS_ERR_INVALID_ARGUMENT
        dev.set_modes(True)
        dev.track(frames[2])
        assert dev._lib.rbs_tracker_modes(dev._t, None, None) == 0            # NULL outputs are allowed
        dev.close()
    with RbSensor(om, cam, P, max_particles=n, precision="f64", device_ids=[0, 0]) as grp:      # a tracker over several shards
        dev = DeviceParticleTracker(trans, grp, om, tp, np.random.default_rng(5))
        refused(_capi.RBS_ERR_UNSUPPORTED, lambda: dev.set_modes(True))
        dev.close()
    # more than 65 536 particles: the stateless entry and the tracker's switch both refuse, before anything is launched
    big = 65537
    om, cam, P = sc.make_scene(("m1_l2",), 32, 24, max_particles=big)
    with RbSensor(om, cam, P, max_particles=big) as s:
        refused(_capi.RBS_ERR_UNSUPPORTED, lambda: s.pose_modes(np.zeros((big, 1, 6)), np.zeros(big), ModesParams()))
        assert len(s.pose_modes(np.zeros((big - 1, 1, 6)), np.zeros(big - 1), ModesParams()).bodies[0]) == 1      # the largest allowed
        dev = DeviceParticleTracker(trans, s, om, ParticleTrackerBuilder.Parameters(evaluation_count=big), np.random.default_rng(5))
        refused(_capi.RBS_ERR_UNSUPPORTED, lambda: dev.set_modes(True))
        refused(_capi.RBS_ERR_INVALID_ARGUMENT, dev.modes)
        dev.close()


# ---------------------------------------------------------------- the C++ mirror
def test_cpp_mirror_prints_pythons_report(gpu_lib, tmp_path):
    exe = str(tmp_path / "modes_check")
    lib = os.path.join(ROOT, "dbot_ros_amd", "lib")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(HERE, "cpp", "modes_check.cpp"), "-L" + lib, "-lrbsensor_mi355x", "-Wl,-rpath," + lib,
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
        dev = DeviceParticleTracker(trans, s, om, tp, device_rng=True, seed=11, modes=True)
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
            got.append(dev.modes())
        dev.close()
    run = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.returncode, run.stdout[-2000:], run.stderr[-2000:])
    lines = run.stdout.strip().split("\n")
    at = 0
    for k, m in enumerate(got):
        head = lines[at].split()
        assert head[0] == "FRAME" and [int(v) for v in head[1:]] == [k, m.frame, len(m.bodies[0])], (head, k)
        for mode in m.bodies[0]:
            row = lines[at + 1].split()
            assert row[0] == "MODE" and int(row[1]) == mode.seed
            vals = np.array([float.fromhex(v) for v in row[2:]])
            assert np.array_equal(vals, np.r_[mode.density, mode.mass, mode.core_mass, mode.delta])
            at += 1
        at += 1
    assert at == len(lines)
