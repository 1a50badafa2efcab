"""Spawned by tests/test_gpu_tracker_routes.py: six frames of the device tracker at 160 x 120 with host-supplied
randomness, in a process of its own -- RBS_TRACKER_TAIL, RBS_TRACKER_FUSED and RBS_TRACKER_RECENTRE_NOW are read once per
process -- writing every frame's estimate and get_state() to the .npz named on the command line.

    python tracker_route_worker.py OUT.npz N_PARTICLES"""
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


def main(out, n):
    om, cam, P = sc.make_scene(("m1_l2",), COLS, ROWS, max_particles=n)
    tp = ParticleTrackerBuilder.Parameters(evaluation_count=n, max_kl_divergence=2.0)
    trans = ObjectTransitionBuilder(ObjectTransitionBuilder.Parameters()).build()
    est, parts, logw, idx, nres = [], [], [], [], []
    with RbSensor(om, cam, P, max_particles=n) as s:
        dev = DeviceParticleTracker(trans, s, om, tp, np.random.default_rng(5))
        Rt = synth.truth_pose(1, frame=0)[0]
        init = np.zeros(12)
        init[3:6] = pose.matrix_to_rotvec(Rt[:9].reshape(3, 3))
        init[0:3] = Rt[9:] - Rt[:9].reshape(3, 3) @ om.centers[0]
        dev.initialize([init])
        rng = np.random.default_rng(77)
        for k in range(1, FRAMES + 1):
            frame = synth.make_frame(s.render_depth(synth.truth_pose(1, frame=k)), ROWS, COLS, rng, occluder=False)
            normals, uniforms = dev.draw_randomness()
            est.append(dev.track(frame, normals, uniforms))
            p, w, i = dev.get_state()
            parts.append(p), logw.append(w), idx.append(i), nres.append(dev.n_resamplings)
        dev.close()
    np.savez(out, estimates=np.array(est), particles=np.array(parts), log_weights=np.array(logw), indices=np.array(idx),
             resamplings=np.array(nres))


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]))
