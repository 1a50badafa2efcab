"""The Gaussian tracker's filter step on the device (rbs_gauss_submit / rbs_gauss_result, GaussianTracker.submit / result)
against rbs_gauss_track, the in-library reference that runs the same algebra on the host in the same operation order."""
import os
import subprocess

import numpy as np
import pytest

import gauss_reference as gr
import gauss_twin as gt
import oracle_binding as ob
import scenarios as sc
from dbot_ros_amd import RbSensor, RbSensorBuilder, synth
from dbot_ros_amd.gaussian import GaussianTracker, GaussianTrackerBuilder
from dbot_ros_amd.sensor import RbSensorError
from test_gaussian_pipeline_cpu import build_driver, write_driver_input

pytestmark = pytest.mark.gpu

SCENES = {1: (("m1",), 640, 480), 3: (("m1", "m2", "m3"), 640, 480)}
_FRAMES = {}


def _frames(bodies, n):
    """[(truth, float32 frame)] of scenarios.make_frames, cached per scene."""
    if (bodies, n) not in _FRAMES:
        meshes, cols, rows = SCENES[bodies]
        om, cam, P = sc.make_scene(meshes, cols, rows, max_particles=1)
        orc = ob.Oracle(om, cam, P, max_particles=1)
        _FRAMES[(bodies, n)] = sc.make_frames(orc, bodies, n, seed=3)
    return _FRAMES[(bodies, n)]


class _Pair:
    """A tracker on a sensor of its own (a sensor drives one tracker at a time), initialised at the first truth."""

    def __init__(self, bodies, frames, **sensor_kw):
        meshes, cols, rows = SCENES[bodies]
        om, cam, _ = sc.make_scene(meshes, cols, rows, max_particles=1)
        self.sensor = RbSensor(om, cam, RbSensorBuilder.Parameters(sample_count=1), max_particles=1, **sensor_kw)
        params = GaussianTrackerBuilder.Parameters()
        params.object_transition.part_count = bodies
        self.t = GaussianTracker(self.sensor, om, params)
        self.t.initialize([self.t._from_model(gt.truth_state(frames[0][0]))])

    def close(self):
        self.t.close()
        self.sensor.close()


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _one_at_a_time(t, ys):
    out = []
    for y in ys:
        t.submit(y)
        out.append((t.result(), t.covariance))
    return out


def _lookahead(t, ys):
    out = []
    t.submit(ys[0])
    for k in range(len(ys)):
        if k + 1 < len(ys):
            t.submit(ys[k + 1])
        out.append((t.result(), t.covariance))
    return out


@pytest.mark.parametrize("bodies", [1, 3])
def test_first_frame_is_the_host_algebra_bit_for_bit(gpu_lib, bodies):
    frames = _frames(bodies, 30)
    a, b = _Pair(bodies, frames), _Pair(bodies, frames)
    try:
        y = frames[0][1]
        a.t.track(y)
        b.t.submit(y)
        b.t.result()
        for u, v in zip(a.t.prior(), b.t.prior()):
            assert np.array_equal(_bits(u), _bits(v))
        assert np.abs(a.t.sigma_poses() - b.t.sigma_poses()).max() <= 1e-14
        assert np.array_equal(_bits(a.t.moments(raw=True)), _bits(b.t.moments(raw=True)))   # (this scene: no depth flipped)
        assert np.array_equal(_bits(a.t.covariance), _bits(b.t.covariance))
        za, zb = a.t.default.reshape(bodies, 12), b.t.default.reshape(bodies, 12)
        for cols in (slice(0, 3), slice(6, 12)):
            assert np.array_equal(_bits(za[:, cols]), _bits(zb[:, cols]))
        rv = np.abs(za[:, 3:6] - zb[:, 3:6])
        assert (rv <= 8 * np.spacing(np.abs(za[:, 3:6]))).all(), rv
        ms = b.t.kernel_ms()
        assert all(m > 0 for m in ms), ms
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("bodies", [1, 3])
def test_closed_loop_matches_track(gpu_lib, bodies):
    frames = _frames(bodies, 30)
    a, b = _Pair(bodies, frames), _Pair(bodies, frames)
    try:
        ys = [y for _, y in frames]
        ref = [(a.t.track(y), a.t.covariance) for y in ys]
        got = _lookahead(b.t, ys)
        for k, ((sa, ca), (sb, cb)) in enumerate(zip(ref, got)):
            assert _rel(sb, sa) <= 1e-8 and _rel(cb, ca) <= 1e-8, (k, _rel(sb, sa), _rel(cb, ca))
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("layout, dtype", [("window", np.float32), ("window", np.float64), ("dense", np.float32),
                                           ("dense", np.float64)])
def test_lookahead_is_one_frame_at_a_time(gpu_lib, layout, dtype):
    """submit(k + 1) before result(k) reuses the frame slot frame k's kernels read: the estimates must not change a bit."""
    frames = _frames(1, 30)[:8]
    ys = [y.astype(dtype) for _, y in frames]
    a, b = _Pair(1, frames, state_layout=layout), _Pair(1, frames, state_layout=layout)
    try:
        ref = _one_at_a_time(a.t, ys)
        got = _lookahead(b.t, ys)
        for (sa, ca), (sb, cb) in zip(ref, got):
            assert np.array_equal(_bits(sa), _bits(sb)) and np.array_equal(_bits(ca), _bits(cb))
        # determinism: the same pipelined run again
        b.t.initialize([b.t._from_model(gt.truth_state(frames[0][0]))])
        again = _lookahead(b.t, ys)
        for (sa, ca), (sb, cb) in zip(got, again):
            assert np.array_equal(_bits(sa), _bits(sb)) and np.array_equal(_bits(ca), _bits(cb))
    finally:
        a.close()
        b.close()


def test_lookahead_with_frames_staged_on_the_device(gpu_lib):
    import torch
    frames = _frames(1, 30)[:6]
    ys = [y for _, y in frames]
    a, b = _Pair(1, frames), _Pair(1, frames)
    try:
        ref = _one_at_a_time(a.t, ys)
        dev = [torch.from_numpy(np.ascontiguousarray(y, dtype=np.float32)).to("cuda:0") for y in ys]
        stream = torch.cuda.current_stream().cuda_stream
        got = []
        b.sensor.set_observation_device(dev[0].data_ptr(), stream)
        b.t.submit(None)
        for k in range(len(ys)):
            if k + 1 < len(ys):
                b.sensor.set_observation_device(dev[k + 1].data_ptr(), stream)
                b.t.submit(None)
            got.append((b.t.result(), b.t.covariance))
        torch.cuda.synchronize()
        for (sa, ca), (sb, cb) in zip(ref, got):
            assert np.array_equal(_bits(sa), _bits(sb)) and np.array_equal(_bits(ca), _bits(cb))
    finally:
        a.close()
        b.close()


def test_track_and_submit_interleave(gpu_lib):
    frames = _frames(1, 30)[:12]
    ys = [y for _, y in frames]
    a, b = _Pair(1, frames), _Pair(1, frames)
    try:
        ref = [(a.t.track(y), a.t.covariance) for y in ys]
        for k, y in enumerate(ys):
            if k % 2 == 0:
                s = b.t.track(y)
            else:
                b.t.submit(y)
                s = b.t.result()
            assert _rel(s, ref[k][0]) <= 1e-8 and _rel(b.t.covariance, ref[k][1]) <= 1e-8, k
            z, m, c = b.t.prior()   # inspection follows whichever path ran the frame
            assert z.shape == (12,) and c.shape == (12, 12)
    finally:
        a.close()
        b.close()


def test_errors(gpu_lib):
    frames = _frames(1, 30)[:4]
    ys = [y for _, y in frames]
    p = _Pair(1, frames)
    t = p.t
    try:
        with pytest.raises(RbSensorError, match="no frame in flight"):
            t.result()
        t.submit(ys[0])
        with pytest.raises(RbSensorError, match="in flight"):
            t.track(ys[1])
        for inspect in (t.prior, t.sigma_poses, t.kernel_ms, lambda: t.moments(raw=True), lambda: t.render(0)):
            with pytest.raises(RbSensorError, match="in flight"):
                inspect()
        t.submit(ys[1])
        with pytest.raises(RbSensorError, match="two frames are in flight"):
            t.submit(ys[2])
        t.result()
        t.result()
        # a frame whose algebra fails, and the frame in flight behind it
        t.initialize([t._from_model(gt.truth_state(frames[0][0]))], cov0=-np.eye(12))
        t.submit(ys[0])
        t.submit(ys[1])
        for _ in range(2):
            with pytest.raises(RbSensorError, match="predicted covariance is not positive definite"):
                t.result()
        with pytest.raises(RbSensorError, match="rbs_gauss_initialize"):
            t.submit(ys[2])
        with pytest.raises(RbSensorError, match="rbs_gauss_initialize"):
            t.track(ys[2])
        t.initialize([t._from_model(gt.truth_state(frames[0][0]))])
        t.submit(ys[0])
        s = t.result()
        assert np.isfinite(s).all() and np.isfinite(t.track(ys[1])).all()
    finally:
        p.close()


def test_cpp_mirror_submit_result_matches_track(gpu_lib, tmp_path):
    exe = build_driver(tmp_path)
    frames = _frames(1, 30)[:10]
    meshes, cols, rows = SCENES[1]
    p = _Pair(1, frames)
    init = p.t._from_model(gt.truth_state(frames[0][0]))
    p.close()
    inp = str(tmp_path / "in.bin")
    write_driver_input(inp, [sc.MESHES[m]() for m in meshes], synth.camera_matrix(cols, rows), cols, rows, init,
                       [y.astype(np.float64) for _, y in frames])
    outs = {}
    for mode in ("--track", "--submit"):
        o = str(tmp_path / f"out{mode}.bin")
        r = subprocess.run([exe, mode, inp, o], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout.startswith("OK"), (r.stdout, r.stderr)
        outs[mode] = np.fromfile(o, dtype=np.float64)
    n = len(frames) * 12
    a, b = outs["--track"], outs["--submit"]
    assert a.size == b.size == n + 144
    assert _rel(b[:n], a[:n]) <= 1e-8 and _rel(b[n:], a[n:]) <= 1e-8


def test_pipelined_moments_stay_inside_the_extended_precision_bar(gpu_lib):
    from test_gpu_gaussian_moments import _setup
    gr.require_extended()
    name = "b1_80x60"
    _, orc, p, B, frames, sensor, tracker = _setup(name, 2)
    try:
        tracker.submit(frames[0][1])
        tracker.submit(frames[1][1])
        tracker.result()
        tracker.result()
        poses = tracker.sigma_poses()
        depths = np.stack([orc.render_depth(q) for q in poses])
        ref = gr.moments(depths, frames[1][1], p, B)
        dev = tracker.moments(raw=True)
        assert ref.excess(dev) <= 1.0, (ref.outside(dev), ref.counts)
        assert ref.counts["pixels"] > 0
    finally:
        tracker.close()
        sensor.close()
