"""Spawned by tests/test_gpu_tracker_posterior.py: tests/tracker_route_worker.py's six frames with the posterior report on, in
a process of its own -- RBS_TRACKER_TAIL, RBS_TRACKER_FUSED and RBS_TRACKER_RECENTRE_NOW are read once per process -- writing
every frame's estimate, report and get_state() to the .npz named on the command line.

    python tracker_posterior_worker.py OUT.npz N_PARTICLES"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import scenarios as sc  # noqa: E402
from dbot_ros_amd import RbSensor, pose, synth  # noqa: E402
from dbot_ros_amd.tracker import DeviceParticleTracker, ObjectTransitionBuilder, ParticleTrackerBuilder  # noqa: E402

FRAMES, COLS, ROWS = 6, 160, 120


def scene_frames(sensor, frames=FRAMES, seed=77):
    rng = np.random.default_rng(seed)
    return [synth.make_frame(sensor.render_depth(synth.truth_pose(1, frame=k)), ROWS, COLS, rng, occluder=False) for k in range(1, frames + 1)]


def initial_state(om):
    Rt = synth.truth_pose(1, frame=0)[0]
    init = np.zeros(12)
    init[3:6] = pose.matrix_to_rotvec(Rt[:9].reshape(3, 3))
    init[0:3] = Rt[9:] - Rt[:9].reshape(3, 3) @ om.centers[0]
    return init


def run(n, max_kl=2.0, posterior=True, look_ahead=False, states=True):
    """Six frames, host-supplied randomness -> dict of arrays: estimates; with posterior the reports' ess, mean, cov and
    ints (n, survivors, resampled, frame); with states (frame by frame only) every frame's get_state()."""
    om, cam, P = sc.make_scene(("m1_l2",), COLS, ROWS, max_particles=n)
    tp = ParticleTrackerBuilder.Parameters(evaluation_count=n, max_kl_divergence=max_kl)
    trans = ObjectTransitionBuilder(ObjectTransitionBuilder.Parameters()).build()
    out = dict(estimates=[], ess=[], mean=[], cov=[], ints=[], particles=[], log_weights=[], indices=[], resamplings=[])

    def report(dev):
        if posterior:
            r = dev.posterior()
            out["ess"].append(r.ess), out["mean"].append(r.mean), out["cov"].append(r.cov)
            out["ints"].append([r.n, r.survivors, int(r.resampled), r.frame])

    with RbSensor(om, cam, P, max_particles=n) as s:
        dev = DeviceParticleTracker(trans, s, om, tp, np.random.default_rng(5), posterior=posterior)
        dev.initialize([initial_state(om)])
        frames = scene_frames(s)
        draws = [dev.draw_randomness() for _ in frames]
        if look_ahead:
            dev.submit(frames[0], *draws[0])
            for k in range(1, len(frames) + 1):
                if k < len(frames):
                    dev.submit(frames[k], *draws[k])
                out["estimates"].append(dev.result())       # frame k - 1, while frame k is in flight
                report(dev)
                out["resamplings"].append(dev.n_resamplings)
        else:
            for frame, (normals, uniforms) in zip(frames, draws):
                out["estimates"].append(dev.track(frame, normals, uniforms))
                report(dev)
                out["resamplings"].append(dev.n_resamplings)
                if states:
                    p, w, i = dev.get_state()
                    out["particles"].append(p), out["log_weights"].append(w), out["indices"].append(i)
        dev.close()
    return {k: np.array(v) for k, v in out.items() if len(v)}


if __name__ == "__main__":
    np.savez(sys.argv[1], **run(int(sys.argv[2])))
