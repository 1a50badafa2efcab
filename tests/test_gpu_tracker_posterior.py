"""The particle tracker's posterior report ON THE DEVICE (dbot_ros_amd/csrc/rbsensor_posterior.hip, rbs_tracker_set_posterior /
rbs_tracker_posterior): the kernels on planted populations through the hooks build's probe, the tracker itself on every
route against the twin applied to get_state(), the unchanged filter, look-ahead, determinism, the refusals, the three route
switches in processes of their own, and the C++ mirror.  Bars: tests/posterior_twin.py (derived, not tuned).

The probe exists in the hooks build only, and two builds of the library do not share a process: outside a process that has
loaded the hooks build, the first probe test re-runs this file's probe tests once in a child with RBS_LIB_PATH set to it, and
every probe test reports its own outcome of that run (as tests/test_gpu_filter_kernels.py does)."""
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

import filter_probes as fp
import posterior_twin as pt
import tracker_posterior_worker as wk
from dbot_ros_amd import CameraData, ObjectModel, RbSensor, RbSensorBuilder, RbSensorError, _capi
from dbot_ros_amd.tracker import BODY, DeviceParticleTracker, ObjectTransitionBuilder, ParticleTrackerBuilder, Posterior, posterior_of

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOOKS = fp.hooks_path(_capi.LIB_PATH)
IN_HOOKS_PROCESS = os.path.abspath(_capi.LIB_PATH) == os.path.abspath(HOOKS)
SIZES = [1, 2, 63, 64, 65, 1023, 1025, 8191, 8192, 8193, 12289]      # wave and block edges, the switch to the grid form, a ragged last chunk
_child = {}
worst = {}


def _delegated(request):
    """True: this process has not loaded the hooks build -- the test's outcome is the one of the child run."""
    if IN_HOOKS_PROCESS:
        return False
    if not _child:
        assert os.path.exists(HOOKS), "build() makes librbsensor_mi355x_hooks.so"
        r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-rA", "-m", "gpu", "-p", "no:cacheprovider", "-k", "probe", __file__],
                           capture_output=True, text=True, timeout=900, env=dict(os.environ, RBS_LIB_PATH=HOOKS))
        _child["outcome"] = dict((m.group(2), m.group(1)) for m in re.finditer(r"^(PASSED|FAILED|ERROR) \S+?::(\S+)", r.stdout, re.M))
        _child["out"] = r.stdout[-8000:] + r.stderr[-2000:]
    assert _child["outcome"].get(request.node.name) == "PASSED", _child["out"]
    return True


@pytest.fixture(scope="module")
def probe(gpu_lib):
    return (pt.PosteriorProbe(HOOKS), fp.FilterProbe(HOOKS)) if IN_HOOKS_PROCESS else None


def _device_recentred(filt, x, mean, parts):
    """x re-centred by recentre_kernel itself -- rbs_tracker_get's route -- through rbs_test_filter."""
    st = fp.make_state(len(x), parts, seed=1)
    st["part_new"], st["mean"] = x, mean
    return filt.run(st, [fp.step(fp.RECENTRE)])["part_new"]


# ---------------------------------------------------------------- the kernels on planted populations
@pytest.mark.parametrize("parts", [1, 2, 3])
@pytest.mark.parametrize("n", SIZES)
def test_probe_planted_populations(request, probe, n, parts):
    """Every weight pattern of the CPU file: against brute force in np.longdouble; pending re-centring bit for bit the result
    on particles recentre_kernel re-centred first; two runs the same bits; the filter's arrays left alone."""
    if _delegated(request):
        return
    post, filt = probe
    mean = pt.planted_mean(parts)
    for kind in pt.KINDS:
        x, lw, idx = pt.population(kind, n, parts)
        xr = _device_recentred(filt, x, mean, parts)
        a, clean_a = post.run(xr, lw, idx, recentred=True, resampled=(n % 2 == 1), frame=n)
        pt.check(a, xr, lw, idx, note=worst)
        assert (a.resampled, a.frame) == (n % 2 == 1, n + 1) and clean_a
        b, clean_b = post.run(x, lw, idx, mean=mean, recentred=False, resampled=(n % 2 == 1), frame=n)
        assert clean_b, "the kernels wrote the filter's arrays"
        assert pt.same_bits(a, b), (kind, float(np.abs(a.cov - b.cov).max()), float(np.abs(a.mean - b.mean).max()))
        a2, _ = post.run(xr, lw, idx, recentred=True, resampled=(n % 2 == 1), frame=n)
        assert pt.same_bits(a, a2), kind
        if kind == "uniform":
            assert a.ess == n
        if parts >= 2 and kind == "uniform" and n >= 1023:        # the planted cross-body correlation, from the cross-body blocks
            c = a.cov[0, BODY] / np.sqrt(a.cov[0, 0] * a.cov[BODY, BODY])
            assert c > 0.5, c
    print("worst share of the bars so far:", worst)


def test_probe_survivors_on_planted_slot_maps(request, probe):
    if _delegated(request):
        return
    post, _ = probe
    for n in (100, 8191, 12289):
        x, lw, _ = pt.population("uniform", n, 1)
        for idx, want in ((np.arange(n), n), (np.zeros(n, int), 1), (np.arange(n) // 7, (n + 6) // 7), (np.r_[np.full(n - 1, n - 1), 0], 2),
                          (np.arange(n)[::-1] % 50, 50)):
            assert post.run(x, lw, idx.astype(np.int32))[0].survivors == want, (n, want)


# ---------------------------------------------------------------- the tracker itself
_runs = {}


def _run(n, max_kl=2.0, posterior=True, look_ahead=False, again=0):
    key = (n, max_kl, posterior, look_ahead, again)
    if key not in _runs:
        _runs[key] = wk.run(n, max_kl, posterior, look_ahead)
    return _runs[key]


def _report(r, k):
    n, surv, res, frame = (int(v) for v in r["ints"][k])
    return Posterior(mean=r["mean"][k], cov=r["cov"][k], ess=float(r["ess"][k]), survivors=surv, resampled=bool(res), n=n, frame=frame)


def _reports_equal(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in ("ess", "mean", "cov", "ints"))


@pytest.mark.parametrize("max_kl", [0.0, 1e9], ids=["always_resamples", "never_resamples"])
@pytest.mark.parametrize("n", [300, 600, 8200], ids=["fused_300", "tail_600", "grid_8200"])
def test_tracker_report_matches_the_twin_on_get_state(gpu_lib, n, max_kl):
    r = _run(n, max_kl)
    for k in range(wk.FRAMES):
        rep = _report(r, k)
        pt.check(rep, r["particles"][k], r["log_weights"][k], r["indices"][k], note=worst)
        twin = posterior_of(r["particles"][k], r["log_weights"][k], r["indices"][k])
        assert rep.survivors == twin.survivors and rep.n == n and rep.frame == k + 1
        if max_kl == 0.0:
            assert rep.resampled and rep.ess == n and rep.survivors < n
        else:
            assert not rep.resampled and rep.survivors == n and rep.ess < n
    print("worst share of the bars so far:", worst)


@pytest.mark.parametrize("n", [300, 600, 8200], ids=["fused_300", "tail_600", "grid_8200"])
def test_filter_is_unchanged_by_the_report(gpu_lib, n):
    on, off = _run(n), _run(n, posterior=False)
    assert "ess" in on and "ess" not in off
    for k in ("estimates", "particles", "log_weights", "indices", "resamplings"):
        assert on[k].tobytes() == off[k].tobytes(), k
    assert on["resamplings"][-1] >= 1


@pytest.mark.parametrize("n", [300, 600, 8200], ids=["fused_300", "tail_600", "grid_8200"])
def test_look_ahead_gives_the_reports_of_frame_by_frame(gpu_lib, n):
    """Two frames in flight: result(k)'s report is frame k's (its number says so) while k + 1 is in flight, bit for bit the
    report of the frame-by-frame run."""
    a, b = _run(n), _run(n, look_ahead=True)
    assert a["estimates"].tobytes() == b["estimates"].tobytes()
    assert [int(v) for v in b["ints"][:, 3]] == list(range(1, wk.FRAMES + 1))
    assert _reports_equal(a, b)


def test_two_runs_give_the_same_bits(gpu_lib):
    for n in (600, 8200):
        assert _reports_equal(_run(n), _run(n, again=1)), n


def test_refusals(gpu_lib):
    n = 64
    om, cam, P = wk.sc.make_scene(("m1_l2",), wk.COLS, wk.ROWS, max_particles=n)
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
        refused(_capi.RBS_ERR_INVALID_ARGUMENT, dev.posterior)               # the report is off
        dev.set_posterior(True)
        refused(_capi.RBS_ERR_INVALID_ARGUMENT, dev.posterior)               # on, but no frame has been handed out since
        dev.track(frames[1])
        assert dev.posterior().frame == 2
        dev.initialize([wk.initial_state(om)])
        refused(_capi.RBS_ERR_INVALID_ARGUMENT, dev.posterior)               # after initialize, before the next result
        dev.submit(frames[0])
        refused(_capi.RBS_ERR_INVALID_ARGUMENT, lambda: dev.set_posterior(False))   # a frame in flight
        refused(_capi.RBS_ERR_INVALID_ARGUMENT, dev.posterior)
        dev.result()
        rep = dev.posterior()
        assert rep.frame == 1 and rep.n == n
        assert 0.0 < dev.posterior_ms() < 50.0                              # the report's kernels' device time, from events
        dev.set_posterior(False)
        dev.track(frames[1])
        refused(_capi.RBS_ERR_INVALID_ARGUMENT, dev.posterior)               # off again
        dev.set_posterior(True)
        dev.track(frames[2])
        assert dev.posterior().frame == 3
        # NULL outputs are allowed, one by one
        info = _capi.RbsTrackerPosteriorInfo()
        import ctypes as C
        assert dev._lib.rbs_tracker_posterior(dev._t, None, None, None) == 0
        assert dev._lib.rbs_tracker_posterior(dev._t, C.byref(info), None, None) == 0 and info.frame == 3 and info.n == n
        dev.close()
    with RbSensor(om, cam, P, max_particles=n, precision="f64", device_ids=[0, 0]) as grp:      # a tracker over several shards
        dev = DeviceParticleTracker(trans, grp, om, tp, np.random.default_rng(5))
        refused(_capi.RBS_ERR_UNSUPPORTED, lambda: dev.set_posterior(True))
        dev.close()


def test_probe_build_poisoned_handle_refuses_the_report(request, gpu_lib, monkeypatch):
    """A tracker whose handle an earlier call left half-way (injected with the test build's RBS_TEST_FAULT, as
    tests/test_gpu_multidevice.py does: an error return, no device fault) answers rbs_tracker_posterior with the poisoned
    error, before anything else is looked at; rbs_tracker_initialize clears it.  (In the hooks process: the hook exists there.)"""
    if _delegated(request):
        return
    n = 30
    om, cam, P = wk.sc.make_scene(("m1_l2",), wk.COLS, wk.ROWS, max_particles=n)
    tp = ParticleTrackerBuilder.Parameters(evaluation_count=n)
    trans = ObjectTransitionBuilder(ObjectTransitionBuilder.Parameters()).build()
    monkeypatch.setenv("RBS_TEST_FAULT", "1:0")        # the group's first rbs_loglikes fails on its second shard
    with RbSensor(om, cam, P, max_particles=n, precision="f64", device_ids=[0, 0]) as grp:
        monkeypatch.delenv("RBS_TEST_FAULT")
        dev = DeviceParticleTracker(trans, grp, om, tp, np.random.default_rng(5))
        dev.initialize([wk.initial_state(om)])
        with RbSensor(om, cam, P, max_particles=1) as one:
            frame = wk.scene_frames(one, 1)[0]
        truth = wk.synth.truth_pose(1, frame=1)
        grp.set_observation(frame)
        with pytest.raises(RbSensorError, match="injected fault"):
            grp.loglikes_poses(wk.synth.particle_poses(truth, n, np.random.default_rng(1)), np.zeros(n, np.int32), update=True)
        with pytest.raises(RbSensorError, match="failed half-way.*injected fault") as e:
            dev.posterior()
        assert e.value.code == _capi.RBS_ERR_HIP
        dev.initialize([wk.initial_state(om)])
        with pytest.raises(RbSensorError) as e:        # a sound tracker again: over several shards the report stays off
            dev.posterior()
        assert e.value.code == _capi.RBS_ERR_INVALID_ARGUMENT
        dev.close()


# ---------------------------------------------------------------- the route switches, each in a process of its own
_routes = {}


def _route(tmp_path_factory, n, switch):
    key = (n, switch)
    if key not in _routes:
        assert not _routes.get("failed"), "an earlier child did not exit 0: " + str(_routes.get("failed"))
        out = str(tmp_path_factory.mktemp("post_route") / "run.npz")
        env = {k: v for k, v in os.environ.items() if not k.startswith("RBS_TRACKER_")}
        if switch:
            env[switch[0]] = switch[1]
        r = subprocess.run([sys.executable, os.path.join(HERE, "tracker_posterior_worker.py"), out, str(n)], capture_output=True, text=True,
                           timeout=120, env=env)
        if r.returncode != 0:
            _routes["failed"] = (key, r.returncode)
        assert r.returncode == 0, (key, r.returncode, r.stdout[-2000:], r.stderr[-2000:])
        _routes[key] = dict(np.load(out))
    return _routes[key]


@pytest.mark.parametrize("n,switch", [(600, ("RBS_TRACKER_TAIL", "0")), (600, ("RBS_TRACKER_RECENTRE_NOW", "1")),
                                      (300, ("RBS_TRACKER_FUSED", "0"))], ids=["tail_off", "recentre_now", "fused_off"])
def test_switched_route_reports_what_the_default_route_reports(gpu_lib, tmp_path_factory, n, switch):
    ref, got = _run(n), _route(tmp_path_factory, n, switch)
    for k in range(wk.FRAMES):
        pt.check(_report(got, k), got["particles"][k], got["log_weights"][k], got["indices"][k])
    for k in ("estimates", "particles", "log_weights", "indices"):
        assert ref[k].tobytes() == got[k].tobytes(), (switch, k)
    assert _reports_equal(ref, got), switch


# ---------------------------------------------------------------- the C++ mirror
def test_cpp_mirror_prints_pythons_report(gpu_lib, tmp_path):
    exe = str(tmp_path / "posterior_check")
    lib = os.path.join(ROOT, "dbot_ros_amd", "lib")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(HERE, "cpp", "posterior_check.cpp"), "-L" + lib, "-lrbsensor_mi355x", "-Wl,-rpath," + lib,
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
        dev = DeviceParticleTracker(trans, s, om, tp, device_rng=True, seed=11, posterior=True)
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
            rep = dev.posterior()
            got.append((rep, dev.pose_covariance(rep)))
        dev.close()
    run = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.returncode, run.stdout[-2000:], run.stderr[-2000:])
    lines = run.stdout.strip().split("\n")
    assert len(lines) == 2 * count, run.stdout[-2000:]
    for k, (rep, pc) in enumerate(got):
        head = lines[2 * k].split()
        assert head[0] == "FRAME" and [int(v) for v in head[1:]] == [k, rep.n, rep.survivors, int(rep.resampled), rep.frame]
        vals = np.array([float.fromhex(v) for v in lines[2 * k + 1].split()])
        assert vals.size == 1 + 12 + 144 + 36
        assert vals[0] == rep.ess and np.array_equal(vals[1:13], rep.mean) and np.array_equal(vals[13:157].reshape(12, 12), rep.cov)
        # J C J^T: two correctly written products of the same numbers in another order of additions
        assert np.abs(vals[157:].reshape(6, 6) - pc[0]).max() <= 64 * pt.U * np.abs(pc[0]).max()
        assert np.abs(pc[0] - rep.cov[:6, :6]).max() > 0          # the centring offset is there


# ---------------------------------------------------------------- the node assembly
def test_node_replay_hands_out_the_reports(gpu_lib, tmp_path):
    """replay_dataset(posterior=True) additionally returns every frame's report -- look-ahead the same bits -- and leaves its
    return value alone with the flag off; the YAML key particle_filter/posterior switches the report on by itself."""
    import test_node as tn
    from dbot_ros_amd import dataset as ds, node, objloader, pose, synth
    tree = node.load_rosparams(*tn._write(tmp_path))
    K = synth.camera_matrix(640, 480)
    vs, ts = objloader.SimpleWavefrontObjectModelLoader(objloader.ObjectResourceIdentifier(str(tmp_path), "object_models", ["part.obj"])).load()
    om = ObjectModel(vs, ts, center=True)

    def truth_state(k):
        Rt = synth.truth_pose(1, frame=k)[0]
        s = np.zeros(12)
        s[3:6] = pose.matrix_to_rotvec(Rt[:9].reshape(3, 3))
        s[0:3] = Rt[9:] - Rt[:9].reshape(3, 3) @ om.centers[0]
        return s

    rng = np.random.default_rng(0)
    rec = ds.TrackingDataset(tmp_path / "recording", load=False)
    with RbSensor(om, CameraData(K, 480, 640), RbSensorBuilder.Parameters(sample_count=1), max_particles=1) as full:
        for k in range(1, 5):
            native = synth.make_frame(full.render_depth(synth.truth_pose(1, frame=k)), 480, 640, rng, occluder=False)
            stamp = ds.Stamp.from_sec(1500000000.0 + k / 30.0)
            rec.add_frame(ds.Image(native.reshape(480, 640), stamp, seq=k), ds.CameraInfo(K, 480, 640, stamp, seq=k), ground_truth=truth_state(k))
    rec.store()
    data = ds.TrackingDataset(tmp_path / "recording")
    off = node.replay_dataset(tree, data, str(tmp_path), [truth_state(0)], seed=3)
    on = node.replay_dataset(tree, data, str(tmp_path), [truth_state(0)], seed=3, posterior=True)
    ahead = node.replay_dataset(tree, data, str(tmp_path), [truth_state(0)], seed=3, posterior=True, look_ahead=True)
    assert len(off) == 2 and len(on) == 3 and len(ahead) == 3
    assert np.array_equal(off[0], on[0]) and np.array_equal(on[0], ahead[0])
    assert [r.frame for r in on[2]] == [1, 2, 3, 4] and all(r.n == 400 and r.cov.shape == (12, 12) and 1.0 <= r.ess <= 400 for r in on[2])
    assert all(pt.same_bits(a, b) for a, b in zip(on[2], ahead[2]))
    tree["particle_filter"]["posterior"] = True
    keyed = node.replay_dataset(tree, data, str(tmp_path), [truth_state(0)], seed=3)
    assert len(keyed) == 2 and np.array_equal(keyed[0], off[0])                 # the flag off: the return value stays as it is
    tracker, _, _, _ = node.build_particle_tracker(tree, K, str(tmp_path), seed=3)
    try:
        tracker.initialize([truth_state(0)])
        tracker.track(data.frame_vector(0, int(tree["downsampling_factor"])))
        assert pt.same_bits(tracker.posterior(), on[2][0])                       # ... but the key has switched the report on
    finally:
        tracker.close()
        tracker.sensor.close()
