"""Runs of the device tracker with the occlusion map for tests/test_gpu_occlusion_map.py: a few frames of the M1 scene at
80 x 60 with host-supplied randomness, every frame's estimate, map and -- on request -- get_state() and the planes of the
slots the population points at.  As a program (spawned with RBS_LIB_PATH set to the hooks build, where the injected fault
exists) it answers for a poisoned tracker:

    python occlusion_map_worker.py poisoned      prints "POISONED_OK" or the reason it is not"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import scenarios as sc  # noqa: E402
from dbot_ros_amd import RbSensor, RbSensorError, _capi, pose, synth  # noqa: E402
from dbot_ros_amd.tracker import DeviceParticleTracker, ObjectTransitionBuilder, ParticleTrackerBuilder  # noqa: E402

FRAMES, COLS, ROWS = 3, 80, 60


def scene_frames(sensor, frames=FRAMES, seed=77, occluder=False, n_bodies=1):
    rng = np.random.default_rng(seed)
    return [synth.make_frame(sensor.render_depth(synth.truth_pose(n_bodies, frame=k)), ROWS, COLS, rng, occluder=occluder)
            for k in range(1, frames + 1)]


def initial_state(om, n_bodies=1):
    init = np.zeros(12 * n_bodies)
    for b, Rt in enumerate(synth.truth_pose(n_bodies, frame=0)):
        init[12 * b + 3:12 * b + 6] = pose.matrix_to_rotvec(Rt[:9].reshape(3, 3))
        init[12 * b:12 * b + 3] = Rt[9:] - Rt[:9].reshape(3, 3) @ om.centers[b]
    return init


def run(n, max_kl=2.0, occlusion_map=True, posterior=False, look_ahead=False, states=False, planes=False):
    """FRAMES frames -> dict of arrays: estimates, resamplings; with occlusion_map the maps and their frame numbers; with
    posterior the reports' means; with states (frame by frame only) every frame's get_state(); with planes also, per frame,
    the planes of the distinct slots (planes[k][j] belongs to slot slots[k][j]), fetched with get_occlusion AFTER the
    frame's map (which makes those slots dense: runs that are compared bit for bit with others do not ask for them)."""
    om, cam, P = sc.make_scene(("m1_l2",), COLS, ROWS, max_particles=n)
    tp = ParticleTrackerBuilder.Parameters(evaluation_count=n, max_kl_divergence=max_kl)
    trans = ObjectTransitionBuilder(ObjectTransitionBuilder.Parameters()).build()
    out = dict(estimates=[], maps=[], map_frames=[], post_mean=[], particles=[], log_weights=[], indices=[], resamplings=[])
    fetched, slots = [], []

    def collect(dev):
        if occlusion_map:
            m = dev.occlusion_map()
            out["maps"].append(m.plane), out["map_frames"].append(m.frame)
        if posterior:
            out["post_mean"].append(dev.posterior().mean)
        out["resamplings"].append(dev.n_resamplings)

    with RbSensor(om, cam, P, max_particles=n) as s:
        dev = DeviceParticleTracker(trans, s, om, tp, np.random.default_rng(5), posterior=posterior, occlusion_map=occlusion_map)
        dev.initialize([initial_state(om)])
        frames = scene_frames(s)
        draws = [dev.draw_randomness() for _ in frames]
        if look_ahead:
            dev.submit(frames[0], *draws[0])
            for k in range(1, len(frames) + 1):
                if k < len(frames):
                    dev.submit(frames[k], *draws[k])
                out["estimates"].append(dev.result())       # frame k - 1, while frame k is in flight
                collect(dev)
        else:
            for frame, (normals, uniforms) in zip(frames, draws):
                out["estimates"].append(dev.track(frame, normals, uniforms))
                collect(dev)
                if states:
                    p, w, i = dev.get_state()
                    out["particles"].append(p), out["log_weights"].append(w), out["indices"].append(i)
                    if planes:
                        u = np.unique(i)
                        slots.append(u), fetched.append(np.stack([s.get_occlusion(int(q)) for q in u]))
        dev.close()
    res = {k: np.array(v) for k, v in out.items() if len(v)}
    if planes:
        res["planes"], res["slots"] = fetched, slots
    return res


def poisoned():
    """A tracker whose handle an earlier call left half-way (the test build's RBS_TEST_FAULT, as tests/test_gpu_multidevice.py
    injects it: an error return, no device fault) answers rbs_tracker_occlusion_map with the poisoned error before anything
    else is looked at; rbs_tracker_initialize clears it."""
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
        # the sensor-level calls on the poisoned handle over two shards: "several devices" is refused first
        flat = np.full(ROWS * COLS, 0.5, np.float32)
        for call in (lambda: grp.occlusion_mean(np.zeros(2, np.int32)), lambda: grp.occlusion_bodies(flat, truth[None])):
            try:
                call()
                return "a sensor-level call ran on a handle over several devices"
            except RbSensorError as e:
                if e.code != _capi.RBS_ERR_UNSUPPORTED or "single-device" not in str(e):
                    return "the poisoned group handle: %d %s" % (e.code, e)
        try:
            dev.occlusion_map()
            return "a poisoned tracker handed out a map"
        except RbSensorError as e:
            if e.code != _capi.RBS_ERR_HIP or "failed half-way" not in str(e) or "injected fault" not in str(e):
                return "not the poisoned error: %d %s" % (e.code, e)
        dev.initialize([initial_state(om)])
        try:
            dev.occlusion_map()
            return "a map without a frame"
        except RbSensorError as e:        # a sound tracker again: the map is off
            if e.code != _capi.RBS_ERR_INVALID_ARGUMENT:
                return "after initialize: %d %s" % (e.code, e)
        dev.close()
    return "POISONED_OK"


if __name__ == "__main__":
    if sys.argv[1:] == ["poisoned"]:
        print(poisoned())
