"""Runs of the device tracker with the object map for tests/test_gpu_object_map.py: a few frames of the M1 scene at 80 x 60 with
host-supplied randomness, every frame's estimate and maps and -- on request -- get_state() and poses().  As a program (spawned
with RBS_LIB_PATH set to the hooks build, where the injected fault exists) it answers for a poisoned tracker:

    python object_map_worker.py poisoned      prints "POISONED_OK" or the reason it is not"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import scenarios as sc  # noqa: E402
from occlusion_map_worker import COLS, ROWS, initial_state, scene_frames  # noqa: E402
from dbot_ros_amd import RbSensor, RbSensorError, _capi, synth  # noqa: E402
from dbot_ros_amd.assess import PoseAssessor  # noqa: E402
from dbot_ros_amd.tracker import DeviceParticleTracker, ObjectTransitionBuilder, ParticleTrackerBuilder  # noqa: E402

FRAMES = 3


def reference_planes(sensor, poses):
    """[m, B, rows, cols] float32: the assessor's per-body planes at `poses` [m, B, 12] (rbs_assess_get_plane: +inf outside a
    body's rectangle and where it has no surface), 64 planes a call."""
    B = sensor.n_bodies
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, B, 12)
    a = PoseAssessor(sensor)
    blank = np.full(sensor.rows * sensor.cols, np.nan, dtype=np.float32)
    out = np.empty((poses.shape[0], B, sensor.rows, sensor.cols), dtype=np.float32)
    step = 64 // B
    for k0 in range(0, poses.shape[0], step):
        chunk = poses[k0:k0 + step]
        a.assess(chunk, blank)
        for k in range(chunk.shape[0]):
            for b in range(B):
                out[k0 + k, b] = a.plane(k, b).reshape(sensor.rows, sensor.cols)
    return out


def run(n, max_kl=2.0, object_map=True, posterior=False, occlusion_map=False, look_ahead=False, states=False, frames=FRAMES,
        occluder=False, planes_of_last=False):
    """`frames` frames -> dict of arrays: estimates, resamplings; with object_map the maps (cover, depth, var) and their frame
    numbers; with posterior / occlusion_map those products; with states (frame by frame only) every frame's get_state() and
    poses(); with planes_of_last the reference planes of the last frame's distinct poses (planes, plane_members: member i
    points at planes[plane_members[i]]) and the frames themselves."""
    om, cam, P = sc.make_scene(("m1_l2",), COLS, ROWS, max_particles=n)
    tp = ParticleTrackerBuilder.Parameters(evaluation_count=n, max_kl_divergence=max_kl)
    trans = ObjectTransitionBuilder(ObjectTransitionBuilder.Parameters()).build()
    out = dict(estimates=[], cover=[], depth=[], var=[], map_frames=[], post_mean=[], occ=[], particles=[], log_weights=[], indices=[],
               poses=[], resamplings=[])

    def collect(dev):
        if object_map:
            m = dev.object_map()
            out["cover"].append(m.cover), out["depth"].append(m.depth), out["var"].append(m.var), out["map_frames"].append(m.frame)
        if posterior:
            out["post_mean"].append(dev.posterior().mean)
        if occlusion_map:
            out["occ"].append(dev.occlusion_map().plane)
        out["resamplings"].append(dev.n_resamplings)

    with RbSensor(om, cam, P, max_particles=n) as s:
        dev = DeviceParticleTracker(trans, s, om, tp, np.random.default_rng(5), posterior=posterior, occlusion_map=occlusion_map,
                                    object_map=object_map)
        dev.initialize([initial_state(om)])
        imgs = scene_frames(s, frames, occluder=occluder)
        draws = [dev.draw_randomness() for _ in imgs]
        if look_ahead:
            dev.submit(imgs[0], *draws[0])
            for k in range(1, len(imgs) + 1):
                if k < len(imgs):
                    dev.submit(imgs[k], *draws[k])
                out["estimates"].append(dev.result())       # frame k - 1, while frame k is in flight
                collect(dev)
        else:
            for img, (normals, uniforms) in zip(imgs, draws):
                out["estimates"].append(dev.track(img, normals, uniforms))
                collect(dev)
                if states:
                    p, w, i = dev.get_state()
                    out["particles"].append(p), out["log_weights"].append(w), out["indices"].append(i)
                    out["poses"].append(dev.poses())
                    out.setdefault("host_poses", []).append(dev.absolute_poses(p))
        extra = {}
        if planes_of_last:
            poses = dev.poses()
            uniq, inverse = np.unique(poses.reshape(n, -1), axis=0, return_inverse=True)
            extra = dict(planes=reference_planes(s, uniq), plane_members=inverse.ravel(), last_log_weights=dev.get_state()[1],
                         frames=np.array(imgs), K=np.asarray(cam.camera_matrix, dtype=np.float64).reshape(3, 3),
                         truth_depth=s.render_depth(synth.truth_pose(1, frame=frames)),
                         segment=dev.segment(), kinect=(P.kinect.model_sigma, P.kinect.sigma_factor))
        dev.close()
    res = {k: np.array(v) for k, v in out.items() if len(v)}
    res.update(extra)
    return res


def poisoned():
    """A tracker whose handle an earlier call left half-way (the test build's RBS_TEST_FAULT: an error return, no device fault)
    answers rbs_tracker_object_map with the poisoned error before anything else is looked at; the sensor-level calls refuse
    a handle over several devices as UNSUPPORTED before they look at the poison; rbs_tracker_initialize clears it."""
    n = 30
    om, cam, P = sc.make_scene(("m1_l2",), COLS, ROWS, max_particles=n)
    tp = ParticleTrackerBuilder.Parameters(evaluation_count=n)
    trans = ObjectTransitionBuilder(ObjectTransitionBuilder.Parameters()).build()
    os.environ["RBS_TEST_FAULT"] = "1:0"        # the group's first rbs_loglikes fails on its second shard
    with RbSensor(om, cam, P, max_particles=n, precision="f64", device_ids=[0, 0]) as grp:
        del os.environ["RBS_TEST_FAULT"]
        dev = DeviceParticleTracker(trans, grp, om, tp, np.random.default_rng(5))
        dev.initialize([initial_state(om)])
        with RbSensor(om, cam, P, max_particles=1) as one:
            frame = scene_frames(one, 1)[0]
        truth = synth.truth_pose(1, frame=1)
        grp.set_observation(frame)
        try:
            grp.loglikes_poses(synth.particle_poses(truth, n, np.random.default_rng(1)), np.zeros(n, np.int32), update=True)
            return "the injected fault did not fire"
        except RbSensorError as e:
            if "injected fault" not in str(e):
                return "another error: " + str(e)
        for call in (lambda: grp.object_map(truth[None]), lambda: grp.object_segment()):
            try:
                call()
                return "a sensor-level call ran on a handle over several devices"
            except RbSensorError as e:
                if e.code != _capi.RBS_ERR_UNSUPPORTED or "single-device" not in str(e):
                    return "the poisoned group handle: %d %s" % (e.code, e)
        try:
            dev.object_map()
            return "a poisoned tracker handed out a map"
        except RbSensorError as e:
            if e.code != _capi.RBS_ERR_HIP or "failed half-way" not in str(e) or "injected fault" not in str(e):
                return "not the poisoned error: %d %s" % (e.code, e)
        dev.initialize([initial_state(om)])
        try:
            dev.object_map()
            return "a map without a frame"
        except RbSensorError as e:        # a sound tracker again: the map is off
            if e.code != _capi.RBS_ERR_INVALID_ARGUMENT:
                return "after initialize: %d %s" % (e.code, e)
        dev.close()
    return "POISONED_OK"


if __name__ == "__main__":
    if sys.argv[1:] == ["poisoned"]:
        print(poisoned())
