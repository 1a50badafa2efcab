"""Meshes shared by the culling tests on the GPU (tests/test_gpu_parity.py, tests/test_gpu_fullsize.py) and the mesh
preparation's CPU test (tests/test_mesh_prep_cpu.py): closed, inward, holed, mixed, several shells, unwelded."""
import numpy as np

from dbot_ros_amd import synth

VARIANTS = ["closed", "closed_inward", "with_holes", "mixed_winding", "two_shells", "unwelded", "one_shell_inside_out"]


def mesh_variants():
    v, t = synth.mesh_m1(level=2)
    v = np.asarray(v, np.float64)
    t = np.asarray(t, np.int32)
    rng = np.random.default_rng(3)
    flipped = t[:, ::-1].copy()
    holes = np.delete(t, rng.choice(len(t), 40, replace=False), axis=0)
    mixed = t.copy()
    sel = rng.choice(len(t), len(t) // 2, replace=False)
    mixed[sel] = mixed[sel][:, ::-1]
    shells_v = np.concatenate([v, v * 0.5 + np.array([0.0, 0.0, 0.09])])
    shells_t = np.concatenate([t, t + len(v)])
    soup_v = v[t].reshape(-1, 3)                      # every triangle owns its three vertices
    soup_t = np.arange(len(soup_v), dtype=np.int32).reshape(-1, 3)
    inside_out_t = np.concatenate([t, flipped + len(v)])      # second shell wound the other way
    return {"closed": (v, t), "closed_inward": (v, flipped), "with_holes": (v, holes),
            "mixed_winding": (v, mixed), "two_shells": (shells_v, shells_t), "unwelded": (soup_v, soup_t),
            "one_shell_inside_out": (shells_v, inside_out_t)}


def box(x0, x1, y0, y1, z0, z1):
    v = np.array([[x, y, z] for z in (z0, z1) for y in (y0, y1) for x in (x0, x1)], dtype=np.float64)
    quads = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]   # outward
    t = []
    for a, b, c, d in quads:
        t += [(a, b, c), (a, c, d)]
    return v, np.array(t, dtype=np.int32)


def box_variant(variant):
    """A box whose vertices sit at x, y = k/256 on the planes z = 1 and z = 2, in the seven variants."""
    v, t = box(-24 / 256, 40 / 256, -16 / 256, 32 / 256, 1.0, 2.0)
    if variant == "closed_inward":
        t = t[:, ::-1].copy()
    elif variant == "with_holes":
        t = np.delete(t, [4, 5], axis=0)
    elif variant == "mixed_winding":
        t[::2] = t[::2][:, ::-1]
    elif variant == "two_shells":
        v2, t2 = box(56 / 256, 88 / 256, -16 / 256, 32 / 256, 1.0, 2.0)
        v, t = np.concatenate([v, v2]), np.concatenate([t, t2 + len(v)])
    elif variant == "unwelded":
        v, t = v[t].reshape(-1, 3), np.arange(3 * len(t), dtype=np.int32).reshape(-1, 3)
    elif variant == "one_shell_inside_out":
        v2, t2 = box(56 / 256, 88 / 256, -16 / 256, 32 / 256, 1.0, 2.0)
        v, t = np.concatenate([v, v2]), np.concatenate([t, t2[:, ::-1] + len(v)])
    return v, t
