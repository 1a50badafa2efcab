"""RBS_COPY_WALK=1 -- several bodies on windowed planes: the copy kernel walks each particle's whole region and skips the
groups' rectangles -- against the default, the strip list the rectangles kernel cuts the region into: the same updating
sequence in two fresh processes gives the same log-likelihoods, windows and planes, bit for bit."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

N, COLS, ROWS, FRAMES = 64, 160, 120, 10
MESHES = ("m1_l2", "box12", "m1_l2")


def _truth(k):
    """Three bodies side by side that drift apart, together (their rectangles merge) and apart again."""
    from dbot_ros_amd import synth
    t = synth.truth_pose(3, frame=k)
    spread = 1.7 - 1.4 * np.sin(np.pi * k / (FRAMES - 1))
    t[:, 9] = (np.arange(3) - 1.0) * 0.14 * spread + 0.002 * k
    t[:, 10] += (np.arange(3) - 1.0) * 0.03 * (k % 3)
    return t


def _sequence(out):
    """Writes every call's log-likelihoods and poses, and the windows and sampled planes of the last call, to `out`."""
    import scenarios as sc
    from dbot_ros_amd import RbSensor, synth
    om, cam, P = sc.make_scene(MESHES, COLS, ROWS, max_particles=N)
    rng = np.random.default_rng(9)
    lls, all_poses = [], []
    with RbSensor(om, cam, P, max_particles=N) as s:
        truths = [_truth(k) for k in range(FRAMES)]
        frames = [synth.make_frame(s.render_depth(t), ROWS, COLS, rng) for t in truths]
        s.reset()
        idx = np.zeros(N, np.int32)
        for k, (t, frame) in enumerate(zip(truths, frames)):
            s.set_observation(frame)
            poses = synth.particle_poses(t, N, rng, scale=1.0 + 0.5 * (k % 3))
            all_poses.append(poses)
            lls.append(s.loglikes_poses(poses, idx, update=True))
            idx = rng.permutation(N).astype(np.int32) if k % 2 else np.sort(rng.integers(0, N, N)).astype(np.int32)
        wins = np.array([s.get_window(q) for q in range(N)], np.int64)
        planes = np.stack([s.get_occlusion(q) for q in range(0, N, 5)])
    np.savez(out, lls=np.stack(lls), wins=wins, planes=planes, poses=np.stack(all_poses))


def _run(tmp, walk):
    out = os.path.join(tmp, f"walk_{walk}.npz")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, RBS_COPY_WALK=str(walk))
    env["PYTHONPATH"] = os.pathsep.join([root, os.path.join(root, "tests")] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    r = subprocess.run([sys.executable, "-s", os.path.abspath(__file__), out], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return np.load(out)


def _group_counts(poses):
    """From the scene's geometry: a lower bound of the number of groups of every particle of every call -- the partition of the
    bodies' rectangles at their LARGEST (the exact projection grown by twice the stated margin, tests/prep_twin.py): bodies
    that stand apart even so are separate groups on the device."""
    import prep_twin as tw
    import scenarios as sc
    from dbot_ros_amd import synth
    om, cam, _ = sc.make_scene(MESHES, COLS, ROWS, max_particles=N)
    Km = synth.camera_matrix(COLS, ROWS)
    K = (Km[0, 0], Km[1, 1], Km[0, 2], Km[1, 2])
    bodies = [v.astype(np.float32) for v in om.vertices]
    out = np.zeros(poses.shape[:2], dtype=np.int64)
    for k in range(poses.shape[0]):
        for i in range(0, poses.shape[1], 8):
            outer = [tw.rect_bars(tw.extents([bodies[b]], [poses[k, i, b]], K), K, COLS, ROWS, 4)[1] for b in range(3)]
            out[k, i] = len(tw.partition(outer))
    return out


@pytest.mark.gpu
def test_the_walk_gives_the_strip_list_bits(gpu_lib):
    with tempfile.TemporaryDirectory() as tmp:
        a, b = _run(tmp, 0), _run(tmp, 1)
    assert np.isfinite(a["lls"]).all()
    assert np.array_equal(a["poses"], b["poses"])
    assert np.array_equal(a["lls"].view(np.uint64), b["lls"].view(np.uint64))
    assert np.array_equal(a["wins"], b["wins"])
    assert np.array_equal(a["planes"].view(np.uint32), b["planes"].view(np.uint32))
    area = (a["wins"][:, 2] - a["wins"][:, 0]).clip(0) * (a["wins"][:, 3] - a["wins"][:, 1]).clip(0)
    assert (area > 0).all() and (a["planes"] != a["planes"][0, 0]).any()
    groups = _group_counts(a["poses"])
    per_call = groups.max(axis=1)
    print(f"\ngroups per call (lower bound): {per_call.tolist()}, window area: median {np.median(area):.0f} px")
    assert (per_call >= 2).any() and (per_call == 3).any(), per_call        # the strip list had groups to cut around ...
    assert per_call.min() <= 2, per_call                                     # ... and the bodies came together in between


if __name__ == "__main__":
    _sequence(sys.argv[1])
