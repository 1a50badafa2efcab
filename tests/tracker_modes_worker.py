"""Spawned by tests/test_gpu_tracker_modes.py (and imported by it): tests/tracker_posterior_worker.py's six frames with the
posterior modes on, in a process of its own -- RBS_TRACKER_RECENTRE_NOW is read once per process -- writing every frame's
estimate, modes and get_state() to the .npz named on the command line.

    python tracker_modes_worker.py OUT.npz N_PARTICLES [BODIES]"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import modes_twin as mt  # noqa: E402
import scenarios as sc  # noqa: E402
from tracker_posterior_worker import FRAMES, COLS, ROWS, initial_state, scene_frames  # noqa: E402,F401
from dbot_ros_amd import RbSensor, pose, synth  # noqa: E402
from dbot_ros_amd.tracker import DeviceParticleTracker, ModesParams, ObjectTransitionBuilder, ParticleTrackerBuilder  # noqa: E402


def initial_states(om, parts):
    """The truth of frame 0 for every body, as tracker_posterior_worker.initial_state gives it for one."""
    init = np.zeros(12 * parts)
    for b in range(parts):
        Rt = synth.truth_pose(parts, frame=0)[b]
        init[12 * b + 3:12 * b + 6] = pose.matrix_to_rotvec(Rt[:9].reshape(3, 3))
        init[12 * b:12 * b + 3] = Rt[9:] - Rt[:9].reshape(3, 3) @ om.centers[b]
    return init


def run(n, max_kl=2.0, modes=True, posterior=False, look_ahead=False, states=True, parts=1):
    """Six frames, host-supplied randomness, n particles of `parts` bodies -> dict of arrays: estimates; with modes the reports'
    n_modes [frames, parts], table [frames, parts, 8, 10] (modes_twin.pack), their frame numbers and the published pose of body
    0's first mode; with posterior the reports' ess, mean, cov; with states (frame by frame only) every frame's get_state()."""
    om, cam, P = sc.make_scene(("m1_l2", "box12", "m1_l2")[:parts], COLS, ROWS, max_particles=n)
    tp = ParticleTrackerBuilder.Parameters(evaluation_count=n * parts, max_kl_divergence=max_kl)
    trans = ObjectTransitionBuilder(ObjectTransitionBuilder.Parameters(part_count=parts)).build()
    out = dict(estimates=[], n_modes=[], table=[], mode_frame=[], mode_pose=[], ess=[], mean=[], cov=[], particles=[], log_weights=[], indices=[],
               resamplings=[], defaults=[])

    def report(dev):
        if modes:
            m = dev.modes()
            k, t = mt.pack(m)
            out["n_modes"].append(k), out["table"].append(t), out["mode_frame"].append(m.frame)
            out["mode_pose"].append(m.bodies[0][0].pose)
        if posterior:
            r = dev.posterior()
            out["ess"].append(r.ess), out["mean"].append(r.mean), out["cov"].append(r.cov)
        out["defaults"].append(dev.default.copy())

    with RbSensor(om, cam, P, max_particles=n) as s:
        dev = DeviceParticleTracker(trans, s, om, tp, np.random.default_rng(5), posterior=posterior, modes=ModesParams() if modes else None)
        dev.initialize([initial_states(om, parts)])
        rng = np.random.default_rng(77)
        frames = scene_frames(s) if parts == 1 else [
            synth.make_frame(s.render_depth(synth.truth_pose(parts, frame=k)), ROWS, COLS, rng, occluder=False) for k in range(1, FRAMES + 1)]
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
    np.savez(sys.argv[1], **run(int(sys.argv[2]), parts=int(sys.argv[3]) if len(sys.argv) > 3 else 1))
