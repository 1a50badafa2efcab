"""The Gaussian tracker's reduced moments on the device (rbs_gauss_moments_kernel, rbs_gauss_reduce_kernel) against
the extended-precision reference of tests/gauss_reference.py, entry by entry, inside its derived bar; and the ways a
frame reaches the tracker.  The cases are tests/gauss_cases.py's: one, two and three bodies, 80x60 to 1280x960,
sigma renders straddling every image border, nothing in view, a frame without a reading, every branch of the
per-pixel model, and the handle layouts (windowed, dense, cols % 4 != 0, float32 likelihood)."""
import numpy as np
import pytest

import gauss_cases as gc
import gauss_reference as gr
import gauss_twin as gt
from dbot_ros_amd import RbSensor, RbSensorBuilder
from dbot_ros_amd.gaussian import GaussianTracker, GaussianTrackerBuilder

pytestmark = pytest.mark.gpu

LAYOUTS = {"window": {}, "dense": dict(state_layout="dense"), "f32": dict(precision="f32")}


def _builder_params(p, parts):
    """GaussianTrackerBuilder.Parameters with a twin Params' values."""
    bp = GaussianTrackerBuilder.Parameters()
    bp.ut_alpha = p.ut_alpha
    o = bp.observation
    o.tail_weight, o.bg_depth, o.fg_noise_std, o.bg_noise_std = p.tail_weight, p.bg_depth, p.fg_noise_std, p.bg_noise_std
    o.uniform_tail_min, o.uniform_tail_max = p.uniform_tail_min, p.uniform_tail_max
    bp.object_transition.part_count = parts
    assert gt.Params.from_builder(bp).__dict__.keys() == p.__dict__.keys()
    for k, v in gt.Params.from_builder(bp).__dict__.items():
        assert np.array_equal(v, getattr(p, k)), k
    return bp


def _setup(name, n_frames, seed=0, **sensor_kw):
    om, cam, P, orc, p, frames = gc.scene(name, n_frames, seed)
    B = len(gc.CASES[name]["meshes"])
    sensor = RbSensor(om, cam, RbSensorBuilder.Parameters(sample_count=1), max_particles=1, **sensor_kw)
    tracker = GaussianTracker(sensor, om, _builder_params(p, B))
    tracker.initialize([tracker._from_model(gt.truth_state(frames[0][0]))])
    return cam, orc, p, B, frames, sensor, tracker


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300))


def _check_frame(name, tracker, orc, p, B, y, prev):
    """One tracked frame: render parity of its sigma poses, its moments inside the bar, and the teacher-forced twin.
    y: the frame as staged (float32).  -> (|dev - ref| / bar at worst, the reference, the sigma renders)."""
    poses = tracker.sigma_poses()
    depths = np.stack([orc.render_depth(q) for q in poses])
    for k in range(len(poses)):
        got = tracker.render(k)
        assert np.array_equal(got.view(np.uint32), depths[k].view(np.uint32)), (k, int((got != depths[k]).sum()))
    ref = gr.moments(depths, y, p, B)
    dev = tracker.moments(raw=True)
    ratio = ref.excess(dev)
    assert ratio <= 1.0, (name, ratio, ref.outside(dev), ref.counts)
    lam, eta = tracker.moments()      # (Lambda with the identity, eta): the same entries
    NP = 6 * B
    iu = np.triu_indices(NP)
    upper = np.zeros((NP, NP))
    upper[iu] = dev[:iu[0].size]
    assert np.array_equal(lam, lam.T) and np.array_equal(np.triu(lam, 1), np.triu(upper, 1))
    assert np.array_equal(np.diag(lam), np.diag(upper) + 1.0) and np.array_equal(eta, dev[iu[0].size:])
    # teacher forcing (tests/test_gpu_gaussian.py's bar): the twin's update from the product's prior and sigma poses
    z, mu_m, S_m = tracker.prior()
    if prev is not None:
        mu_prev = prev[0].copy().reshape(-1, 12)
        mu_prev[:, 0:6] = 0.0
        tw0 = gt.GaussTwin(p, B)
        pm, pS = tw0.predict(mu_prev.ravel(), prev[1])
        assert _rel(mu_m, pm) < 1e-12 and _rel(S_m, pS) < 1e-12
    cache = {q.tobytes(): d for q, d in zip(poses, depths)}
    tw = gt.GaussTwin(p, B, lambda q: cache[np.ascontiguousarray(q).tobytes()])
    z2, _, S2, own = tw.step(z, mu_m, S_m, y, poses=poses)
    assert np.abs(own - poses).max() < 1e-12
    assert _rel(tracker.default, z2) < 1e-10 and _rel(tracker.covariance, S2) < 1e-10, \
        (name, _rel(tracker.default, z2), _rel(tracker.covariance, S2))
    if "empty" in gc.CASES[name]["expect"]:
        # nothing to see: Lambda = I and eta = 0 exactly, so the update leaves the predicted mean where it was
        assert not np.any(dev)
        pos = np.arange(tracker.D).reshape(-1, 12)
        assert np.array_equal(tracker.default[pos[:, 0:3]], z[pos[:, 0:3]] + mu_m[pos[:, 0:3]])
        assert np.array_equal(tracker.default[pos[:, 6:12]], mu_m[pos[:, 6:12]])
        assert _rel(tracker.covariance, S_m) < 1e-12
    return ratio, ref, depths


CASE_RUNS = [(n, "window") for n in gc.CASES] + [("slab", "dense"), ("slab", "f32"), ("b2_161x121", "f32")]


@pytest.mark.parametrize("name, layout", CASE_RUNS, ids=[f"{n}-{l}" for n, l in CASE_RUNS])
def test_device_moments_stay_inside_the_bar(gpu_lib, name, layout):
    n_frames = 2 if name == "m4_1280x960" else 3
    cam, orc, p, B, frames, sensor, tracker = _setup(name, n_frames, seed=4, **LAYOUTS[layout])
    worst, prev = 0.0, None
    try:
        for _, y in frames:
            tracker.track(y)
            ratio, ref, depths = _check_frame(name, tracker, orc, p, B, y, prev)
            worst = max(worst, ratio)
            prev = (tracker.default.copy(), tracker.covariance)
        gc.check_reach(name, ref, depths, cam.cols, cam.rows)
        print(f"\nMOMENTS {name}-{layout}: max |dev - ref| / bar = {worst:.3e}; last frame {ref.counts}")
    finally:
        tracker.close()
        sensor.close()


def _run(tracker, frames, feed):
    """Track every frame through feed(tracker, y); -> the bits of every state, covariance and moment vector."""
    tracker.initialize([tracker._from_model(gt.truth_state(frames[0][0]))])
    out = []
    for _, y in frames:
        feed(tracker, y)
        out += [tracker.default.copy(), tracker.covariance, tracker.moments(raw=True)]
    return [a.view(np.uint64).copy() for a in out]


def test_float32_and_float64_frames_give_the_same_bits(gpu_lib):
    _, orc, p, B, frames, sensor, tracker = _setup("slab", 3, seed=6)
    try:
        a = _run(tracker, frames, lambda t, y: t.track(y))
        b = _run(tracker, frames, lambda t, y: t.track(y.astype(np.float64)))
        assert all(np.array_equal(u, v) for u, v in zip(a, b))
    finally:
        tracker.close()
        sensor.close()


def _staged(mode, sensor, keep):
    def feed(tracker, y):
        if mode == "f32":
            sensor.set_observation(y)
        elif mode == "f64":
            sensor.set_observation(y.astype(np.float64))
        elif mode == "borrowed":
            keep.append(y.astype(np.float64))
            sensor.set_observation_borrowed(keep[-1])
        elif mode == "borrowed_f32":
            keep.append(y.copy())
            sensor.set_observation_borrowed(keep[-1])
        elif mode == "native":
            f = 2
            native = np.full((sensor.rows * f, sensor.cols * f), 9.0, dtype=np.float32)   # (never read)
            native[::f, ::f] = y.reshape(sensor.rows, sensor.cols)
            sensor.set_observation_native(native, f)
        else:
            import torch
            d = torch.from_numpy(y).to(torch.device("cuda", 0))
            torch.cuda.synchronize()
            keep.append(d)
            sensor.set_observation_device(d.data_ptr())
        tracker.track(None)
    return feed


@pytest.mark.parametrize("size", ["slab", "b1_80x60"])
@pytest.mark.parametrize("mode", ["f32", "f64", "borrowed", "borrowed_f32", "native", "device"])
def test_a_staged_frame_tracks_as_the_frame_itself(gpu_lib, mode, size):
    """rbs_gauss_track(g, NULL, ...) after each rbs_set_observation* call: the same bits as passing the frame.  (80x60
    frames are read by a kernel straight from the pinned staging buffer; 320x240 ones are copied first.)"""
    _, orc, p, B, frames, sensor, tracker = _setup(size, 3, seed=7)
    keep = []
    try:
        a = _run(tracker, frames, lambda t, y: t.track(y))
        b = _run(tracker, frames, _staged(mode, sensor, keep))
        assert all(np.array_equal(u, v) for u, v in zip(a, b)), mode
    finally:
        tracker.close()
        sensor.close()


def test_moments_are_refused_before_the_first_frame_and_without_pointers(gpu_lib):
    import ctypes as C
    from dbot_ros_amd import _capi
    from dbot_ros_amd.sensor import RbSensorError
    _, orc, p, B, frames, sensor, tracker = _setup("b1_80x60", 1)
    lib = _capi.load()
    try:
        with pytest.raises(RbSensorError, match="no frame tracked yet"):
            tracker.moments()
        tracker.track(frames[0][1])
        out, n = (C.c_double * 27)(), C.c_int32(-1)
        assert lib.rbs_gauss_get_moments(tracker._g, None, C.byref(n)) == _capi.RBS_ERR_INVALID_ARGUMENT and n.value == -1
        assert lib.rbs_gauss_get_moments(tracker._g, out, None) == _capi.RBS_ERR_INVALID_ARGUMENT
        assert lib.rbs_gauss_get_moments(tracker._g, out, C.byref(n)) == _capi.RBS_OK and n.value == 27
        assert np.array_equal(np.frombuffer(out, dtype=np.float64), tracker.moments(raw=True))
        tracker.initialize([tracker._from_model(gt.truth_state(frames[0][0]))])   # a new track: nothing to read yet
        with pytest.raises(RbSensorError, match="no frame tracked yet"):
            tracker.moments()
    finally:
        tracker.close()
        sensor.close()
