"""The object finder through its outer layers on the device: the node's auto-detect path (node.replay_dataset with
initial_states=None, on test_node.py's recorded-dataset scenario), the C++ mirror against the Python finder, and the
handles it refuses."""
import os
import subprocess

import numpy as np
import pytest

import scenarios as sc
import test_find_object_cpu as drv
from dbot_ros_amd import RbSensor, _capi, node, objloader, pose, synth
from dbot_ros_amd.finder import ObjectFinder
from dbot_ros_amd.sensor import RbSensorError
from test_node import _write

pytestmark = pytest.mark.gpu


# Measured on one MI355X with the default search, and NOT met: at this scenario's 80x60 (downsampling_factor 8) the
# finder's best pose lies 0.39 m from the truth on frame 0, and the track never recovers (0.33 m on frame 11).  The
# bar stays that of the truth-started run (the coarse candidates miss the object).
@pytest.mark.xfail(reason="the default search does not find the object in this scenario (measured values above)", strict=True)
def test_replay_of_a_recorded_dataset_found_on_frame_0(tmp_path, gpu_lib):
    """test_node.py's recorded-dataset scenario, started by the finder instead of the truth: the same bar."""
    from dbot_ros_amd import CameraData, ObjectModel, RbSensorBuilder
    from dbot_ros_amd import dataset as ds
    paths = _write(tmp_path)
    tree = node.load_rosparams(*paths)
    K = synth.camera_matrix(640, 480)
    vs, ts = objloader.SimpleWavefrontObjectModelLoader(
        objloader.ObjectResourceIdentifier(str(tmp_path), "object_models", ["part.obj"])).load()
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
        for k in range(1, 13):
            native = synth.make_frame(full.render_depth(synth.truth_pose(1, frame=k)), 480, 640, rng, occluder=False)
            stamp = ds.Stamp.from_sec(1500000000.0 + k / 30.0)
            rec.add_frame(ds.Image(native.reshape(480, 640), stamp, seq=k), ds.CameraInfo(K, 480, 640, stamp, seq=k),
                          ground_truth=truth_state(k))
    rec.store()
    data = ds.TrackingDataset(tmp_path / "recording")
    ests, wall = node.replay_dataset(tree, data, str(tmp_path), None, seed=3)
    assert ests.shape == (12, 12) and wall > 0
    err = [np.linalg.norm(ests[i, 0:3] - data.get_ground_truth(i)[0:3]) for i in range(12)]
    print("auto-detect replay: position error per frame (m)", np.round(err, 4))
    assert max(err[-4:]) < 0.025, err


def test_cpp_mirror_is_bit_identical_to_python(tmp_path, gpu_lib):
    om, cam, P = sc.make_scene(("m1",), 320, 240, max_particles=1)
    p = ObjectFinder.Parameters(max_seeds=64, n_rotations=256, n_candidates=256, n_survivors=8, rounds=3, children=32,
                                batch=8192)
    with RbSensor(om, cam, P, max_particles=1) as sensor:
        rng = np.random.default_rng(2)
        d = sensor.render_depth(synth.truth_pose(1, z=0.7)[0])
        frame = synth.make_frame(np.where(np.isfinite(d), d, np.inf), cam.rows, cam.cols, rng)
        with ObjectFinder(sensor, om, p) as fnd:
            want = fnd.find(frame)
    exe = drv.build_driver(tmp_path)
    inp, out = os.path.join(str(tmp_path), "in.bin"), os.path.join(str(tmp_path), "out.bin")
    drv.write_driver_input(inp, om.vertices[0], om.triangles[0], cam.camera_matrix, cam.cols, cam.rows, p, frame)
    r = subprocess.run([exe, inp, out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("OK"), (r.stdout, r.stderr)
    found, poses, scores, states = drv.read_driver_output(out)
    assert found == want.found
    np.testing.assert_array_equal(poses, want.poses)
    np.testing.assert_array_equal(scores, want.scores)
    # (the driver's mesh is already centred: its states are the poses' own)
    for s, q in zip(states, poses):
        np.testing.assert_allclose(s[:3], q[9:], rtol=0, atol=0)
        np.testing.assert_allclose(pose.rotvec_to_matrix(s[3:6]).ravel(), q[:9], rtol=0, atol=1e-12)
        assert not s[6:].any()


def test_a_multi_device_handle_is_refused(gpu_lib, monkeypatch):
    # a handle over a device list is a group (its shards carry the planes) even with one device where
    # RBS_GROUP_SINGLE is set: the finder runs on single-device handles only
    monkeypatch.setenv("RBS_GROUP_SINGLE", "1")
    om, cam, P = sc.make_scene(("m1",), 160, 120, max_particles=2)
    with RbSensor(om, cam, P, max_particles=2, device_ids=[0]) as g:
        with pytest.raises(RbSensorError) as e:
            ObjectFinder(g, om)
        assert e.value.code == _capi.RBS_ERR_UNSUPPORTED
        assert "single-device" in str(e.value)
