"""Scenes for the Gaussian tracker's moments tests (tests/test_gaussian_moments_cpu.py on the twin's sigma poses,
tests/test_gpu_gaussian_moments.py on the device's): bodies, shapes, visibility and the per-pixel model's branches.

Each case names what it must reach; gauss_reference.moments' counts show that it did."""
import numpy as np

import gauss_twin as gt
import oracle_binding as ob
import scenarios as sc
from dbot_ros_amd import synth

EDGE = (0.38, 0.27)   # test_gpu_parity.test_render_edge_poses' straddles_image_edge offset, at z = 0.7

# name: meshes, cols, rows, twin parameters, frame options, and the counts it must reach ("grid": the covered
# bounding box over all sigma renders exceeds one pass of the moments grid, 65 536 pixels)
CASES = {
    "b1_80x60": dict(meshes=("m1",), size=(80, 60), expect=("b_mid",)),
    "b2_161x121": dict(meshes=("m1", "m2"), size=(161, 121), expect=("b_mid",)),
    "b3_640x480": dict(meshes=("m1", "m2", "m3"), size=(640, 480), expect=("b_mid",)),
    "m4_1280x960": dict(meshes=("m4",), size=(1280, 960), expect=("grid", "b_mid")),
    "edge_left_top": dict(meshes=("m1",), size=(320, 240), offset=(-EDGE[0], -EDGE[1]), expect=("left", "top")),
    "edge_right_bottom": dict(meshes=("m1",), size=(320, 240), offset=EDGE, expect=("right", "bottom")),
    "edge_right_top_b2": dict(meshes=("m1", "m2"), size=(320, 240), offset=(EDGE[0], -EDGE[1]), expect=("right", "top")),
    "edge_left_bottom": dict(meshes=("m1",), size=(322, 241), offset=(-EDGE[0], EDGE[1]), expect=("left", "bottom")),
    "off_screen": dict(meshes=("m1",), size=(160, 120), offset=(2.0, 0.0), expect=("empty",)),
    "all_nan": dict(meshes=("m1",), size=(160, 120), frame=dict(nan_frac=1.0), expect=("empty",)),
    # the 1.5 m background lies beyond the tail range: b = 1 by range there
    "tail_range": dict(meshes=("m1",), size=(320, 240), params=dict(uniform_tail_max=1.0), expect=("b_range", "b_mid")),
    # the default slab occluder at 0.5 m: exponents that overflow (b = 0) beside 0 < b < 1
    "slab": dict(meshes=("m1",), size=(320, 240), expect=("b_zero", "b_mid")),
    "tail_weight_0": dict(meshes=("m1",), size=(320, 240), params=dict(tail_weight=0.0), expect=("plain",)),
    # W_m0 != 0 and W_c0 < 0; a background at the object's depth with no spread of its own lets P fall below fg^2
    "alpha_0.5": dict(meshes=("m1",), size=(320, 240), params=dict(ut_alpha=0.5, bg_depth=0.7, bg_noise_std=0.0, fg_noise_std=0.01),
                      expect=("p_clamp",)),
    "alpha_2": dict(meshes=("m1",), size=(320, 240), params=dict(ut_alpha=2.0, bg_depth=0.7, bg_noise_std=0.0, fg_noise_std=0.01),
                    expect=("p_clamp",)),
}


def truth(case, n_bodies, frame):
    t = synth.truth_pose(n_bodies, frame=frame)
    if "offset" in case:
        t[:, 9] += case["offset"][0]
        t[:, 10] += case["offset"][1]
    return t


def scene(name, n_frames, seed=0, max_particles=1):
    """-> (object model, camera, sensor parameters, oracle, twin parameters, [(truth, float32 frame)])."""
    case = CASES[name]
    B = len(case["meshes"])
    om, cam, P = sc.make_scene(case["meshes"], *case["size"], max_particles=max_particles)
    orc = ob.Oracle(om, cam, P, max_particles=max_particles)
    rng = np.random.default_rng(seed)
    frames = []
    for k in range(n_frames):
        t = truth(case, B, k)
        frames.append((t, synth.make_frame(orc.render_depth(t), orc.rows, orc.cols, rng, **case.get("frame", {}))))
    return om, cam, P, orc, gt.Params(**case.get("params", {})), frames


def check_reach(name, ref, depths, cols, rows):
    """Assert that the case reached what it names (ref: gauss_reference.Moments of its frame)."""
    c = ref.counts
    cov = np.isfinite(depths).any(0).reshape(rows, cols)
    for what in CASES[name]["expect"]:
        if what == "empty":
            assert c["pixels"] == 0 and not np.any(ref.value) and not np.any(ref.bar), c
        elif what == "grid":
            rr, cc = np.nonzero(cov)
            bbox = (int(np.ptp(rr)) + 1) * (int(np.ptp(cc)) + 1)
            assert bbox > 256 * 256, bbox          # so the union rectangle is too: some block goes round twice
        elif what == "plain":
            assert c["b_zero"] == c["b_mid"] == c["b_range"] == 0 and c["pixels"] > 0, c
        elif what in ("left", "right", "top", "bottom"):
            line = {"left": cov[:, 0], "right": cov[:, -1], "top": cov[0], "bottom": cov[-1]}[what]
            assert line.any() and not cov.all(), what
        else:
            assert c[what] > 0, (what, c)
