"""The windowed copy inside the raster kernel (rbs_raster_kernel_wcopy_*) against the side-stream copy kernel
(RBS_FUSED_COPY=0): the same updating sequence in two fresh processes gives the same log-likelihoods, child planes and
windows, bit for bit, in both likelihood precisions."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

N = 512


def _sequence(out, precision):
    """A C1-shaped updating sequence (M1 at 640x480, moving poses, resampled parents): windows grow along the object's
    trail and re-tighten as its values decay.  Writes every call's log-likelihoods, and the planes and windows of the
    last call, to `out`."""
    import scenarios as sc
    from dbot_ros_amd import RbSensor, synth
    om, cam, P = sc.make_scene(("m1",), 640, 480, max_particles=N)
    rng = np.random.default_rng(5)
    lls = []
    with RbSensor(om, cam, P, max_particles=N, precision=precision) as s:
        truths = []
        for k in range(14):
            t = synth.truth_pose(1, frame=k)
            t[:, 9] += -0.08 + 0.012 * k            # across the image: a trail the windows follow
            t[:, 10] += -0.04 + 0.006 * k
            truths.append(t)
        frames = [synth.make_frame(s.render_depth(t), cam.rows, cam.cols, rng) for t in truths]
        s.reset()
        idx = np.zeros(N, np.int32)
        for k, (t, frame) in enumerate(zip(truths, frames)):
            s.set_observation(frame)
            if k % 4 == 3:                        # a read-only call between updating ones
                lls.append(s.loglikes_poses(synth.particle_poses(t, N, rng), idx.copy(), update=False))
            lls.append(s.loglikes_poses(synth.particle_poses(t, N, rng, scale=1.0 + 0.5 * (k % 3)), idx, update=True))
            idx = rng.permutation(N).astype(np.int32) if k % 2 else np.sort(rng.integers(0, N, N)).astype(np.int32)
        wins = np.array([s.get_window(q) for q in range(N)], np.int64)
        planes = np.stack([s.get_occlusion(q) for q in range(0, N, 7)])
    np.savez(out, lls=np.stack(lls), wins=wins, planes=planes)


def _run(tmp, fused, precision):
    out = os.path.join(tmp, f"{precision}_{fused}.npz")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, RBS_FUSED_COPY=str(fused))
    env["PYTHONPATH"] = os.pathsep.join([root, os.path.join(root, "tests")] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    r = subprocess.run([sys.executable, "-s", os.path.abspath(__file__), out, precision], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return np.load(out)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_fused_copy_gives_the_side_stream_bits(gpu_lib, precision):
    with tempfile.TemporaryDirectory() as tmp:
        a, b = _run(tmp, 1, precision), _run(tmp, 0, precision)
    assert np.isfinite(a["lls"]).all()
    assert np.array_equal(a["lls"].view(np.uint64), b["lls"].view(np.uint64))
    assert np.array_equal(a["wins"], b["wins"])
    assert np.array_equal(a["planes"].view(np.uint32), b["planes"].view(np.uint32))
    area = (a["wins"][:, 2] - a["wins"][:, 0]).clip(0) * (a["wins"][:, 3] - a["wins"][:, 1]).clip(0)
    print(f"\nwindow area: median {np.median(area):.0f} px, max {area.max()} px")
    assert (area > 0).any()


if __name__ == "__main__":
    _sequence(sys.argv[1], sys.argv[2])
