"""The object map without a device: the numpy twins (dbot_ros_amd.tracker.object_map_of, segment_of) on planted planes worked
out by hand and on the oracle's renders, the bars' arithmetic, the C-ABI's entry points and parameter layout, the compiler's
report of the rbs_objmap_* kernels, the Python, node and C++ surface.  Bars: tests/objmap_twin.py."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np

import objmap_twin as jt
import oracle_binding as ob
import scenarios as sc
from dbot_ros_amd import RbSensor, _capi, node, synth
from dbot_ros_amd.tracker import (DeviceParticleTracker, ObjectMap, ParticleTracker, Segmentation, object_map_of, segment_of)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
INC = os.path.join(ROOT, "include")
LIB = os.path.join(ROOT, "dbot_ros_amd", "lib")
LD = np.longdouble


# ---------------------------------------------------------------- the twin on planted planes
def test_twin_on_planted_planes_gives_the_values_worked_out_by_hand():
    """Members 0, 0, 0, 1, 2 with log-weights 0, 0, 0, 0, -inf: W = (3, 1, 0), S = 4 (tests/objmap_twin.planted)."""
    P, R = jt.planted()
    rows, cols = P.shape[2:]
    cover, depth, var, a, S = object_map_of(P, R, [0, 0, 0, 1, 2], [0.0, 0.0, 0.0, 0.0, -np.inf])
    cover, depth, var, a = cover.reshape(2, rows, cols), depth.reshape(rows, cols), var.reshape(rows, cols), a.reshape(rows, cols)
    assert S == 4
    # columns 0, 1 of rows 1..3: body 0 of pose 0 alone
    assert (cover[0, 1:4, 0:2] == 0.75).all() and (cover[1, 1:4, 0:2] == 0).all()
    assert (depth[1:4, 0:2] == 1.0).all() and (var[1:4, 0:2] == 0).all()
    # columns 2, 3 of rows 1 and 3: pose 0's body 1 is nearer
    for r in (1, 3):
        assert (cover[0, r, 2:4] == 0).all() and (cover[1, r, 2:4] == 0.75).all() and (depth[r, 2:4] == 0.5).all() and (var[r, 2:4] == 0).all()
    # columns 2, 3 of row 2: pose 0 -> body 1 at 0.5 (weight 3); pose 1 -> the tie at 2.0 stays with body 0 (weight 1)
    assert (cover[0, 2, 2:4] == 0.25).all() and (cover[1, 2, 2:4] == 0.75).all() and (a[2, 2:4] == 4).all()
    assert (depth[2, 2:4] == 0.875).all() and (var[2, 2:4] == 0.421875).all()
    # column 4: body 1 of pose 0; column 5 holds a value but lies outside the body's rectangle: uncovered
    assert (cover[1, 1:4, 4] == 0.75).all() and (depth[1:4, 4] == 0.5).all()
    none = np.ones((rows, cols), bool)
    none[1:4, 0:5] = False
    assert (a[none] == 0).all() and (cover[:, none] == 0).all() and np.isposinf(depth[none].astype(np.float64)).all() and (var[none] == 0).all()
    assert (cover.sum(axis=0) == a / S).all()                     # cover sums to a / S (exact here: dyadic weights)
    # the member at -inf contributes nothing: without it, the same maps
    again = object_map_of(P[:2], R[:2], [0, 0, 0, 1], None)
    assert all(np.array_equal(x, y) for x, y in zip((cover.reshape(2, -1), depth.ravel(), var.ravel()), again[:3]))


def test_twin_over_the_oracles_renders():
    """Real poses of the two-body scene: the per-body planes are the oracle's renders of each body alone, their minimum is the
    oracle's render of the whole pose, one pose's depth map is that render, and the covers sum to a / S."""
    rows, cols = 60, 80
    names = ("m1_l2", "box12")
    om, cam, P = sc.make_scene(names, cols, rows, max_particles=4)
    whole = ob.Oracle(om, cam, P)
    singles = []
    for b in range(2):
        omb, _, Pb = sc.make_scene(names[b:b + 1], cols, rows, max_particles=4)
        assert np.array_equal(omb.vertices[0], om.vertices[b])      # (the same centring: body b's mesh as the scene has it)
        singles.append(ob.Oracle(omb, cam, Pb))
    rng = np.random.default_rng(2)
    poses = synth.particle_poses(synth.truth_pose(2), 5, rng, scale=4.0)
    poses[3, 1, 9:12] = poses[3, 0, 9:12] + [0.01, 0.0, 0.0]        # the two bodies interpenetrate
    planes = np.stack([[singles[b].render_depth(q[b:b + 1]).astype(np.float32) for b in range(2)] for q in poses]).reshape(5, 2, rows, cols)
    full = np.stack([whole.render_depth(q).astype(np.float32) for q in poses]).reshape(5, rows, cols)
    assert np.array_equal(planes.min(axis=1).view(np.uint32), full.view(np.uint32)), "min over the bodies is not the whole pose"
    assert (np.isfinite(planes[3]).all(axis=0)).sum() > 30, "no overlap to own"
    rects = np.tile(np.array([0, 0, cols, rows]), (5, 2, 1))
    cover, depth, var, a, S = object_map_of(planes, rects, None, rng.normal(0, 2, 5))
    assert np.abs(cover.sum(axis=0) - a / S).max() <= 2.0 ** -60
    assert ((a > 0) == np.isfinite(full).any(axis=0).ravel()).all()
    c1, d1, v1, _, _ = object_map_of(planes[3:4], rects[3:4], None, None)
    assert np.array_equal(d1.astype(np.float32).view(np.uint32), full[3].ravel().view(np.uint32)) and (v1 == 0).all()
    owner0 = planes[3, 0] <= planes[3, 1]
    assert np.array_equal(c1[0] == 1, (owner0 & np.isfinite(planes[3, 0])).ravel())      # a tie stays with body 0


def test_the_bars_are_what_the_derivation_says():
    n = 300
    e = (2 * n + 64) * 2.0 ** -52
    assert float(jt.eps(n)) == e
    assert np.allclose(np.float64(jt.bar_cover(np.array([0.5], dtype=LD), n)[0]), 2.0 ** -25 + e, rtol=1e-12)
    assert np.allclose(np.float64(jt.bar_depth(np.array([0.7], dtype=LD), n)[0]), 2.0 ** -25 + 0.7 * e, rtol=1e-12)
    t, m2 = np.array([1e-6], dtype=LD), np.array([0.49], dtype=LD)
    want = 0.5 * float(np.spacing(np.float32(1e-6))) + 3 * e * 0.49 + 2.0 ** -52 * 1e-6
    assert np.allclose(np.float64(jt.bar_var(t, m2, n)[0]), want, rtol=1e-6)
    assert 3 * e * 0.49 > 100 * 2.0 ** -52 * 1e-6, "the cancellation term is the one that counts"


def test_permuting_the_members_stays_within_the_bars():
    P, R = jt.planted()
    rng = np.random.default_rng(4)
    big = np.tile(P, (4, 1, 1, 1)) * rng.uniform(0.5, 1.5, (12, 1, 1, 1)).astype(np.float32)
    rects = np.tile(R, (4, 1, 1))
    for name, n, m, idx, lw in jt.populations(lambda n: 12, seed=3):
        ref = object_map_of(big, rects, idx, lw)
        perm = rng.permutation(n)
        got = object_map_of(big, rects, idx[perm], None if lw is None else lw[perm])
        jt.check(tuple(x.astype(np.float32) for x in got[:3]), ref, n, what=name)


# ---------------------------------------------------------------- segment_of
def _seg_inputs():
    rows, cols = 4, 6
    K = synth.camera_matrix(cols, rows)
    cover = np.zeros((2, rows, cols), np.float32)
    depth = np.full((rows, cols), 1.0, np.float32)
    var = np.zeros((rows, cols), np.float32)
    y = np.full((rows, cols), 1.0, np.float32)
    return rows, cols, K, cover, depth, var, y


def test_segment_of_thresholds_ties_and_bad_readings():
    rows, cols, K, cover, depth, var, y = _seg_inputs()
    ms, sf, sig = 0.003, 0.0014247, 3.0
    tau = sig * (ms + sf * 1.0)
    cover[0] = 0.5                                            # exactly min_cover: labelled
    cover[0, 0, 1] = np.nextafter(np.float32(0.5), np.float32(0))      # just below: not
    cover[:, 0, 2] = 0.5                                      # a tie between the bodies: the lowest
    cover[1, 0, 3] = 0.75                                     # body 1 wins
    y[1, 0], y[1, 1], y[1, 2] = np.nan, np.inf, -np.inf       # no reading
    # |y - D| exactly tau in binary64 cannot be planted through a float y; the threshold is met from both sides instead
    y[2, 0] = np.float32(1.0 + tau * 0.999)                   # inside tau with zero variance: labelled
    y[2, 1] = np.float32(1.0 + tau * 1.001)                   # outside tau, zero variance: not
    y[2, 2] = y[2, 1]
    ex = max(0.0, abs(float(y[2, 2]) - 1.0) - tau)
    var[2, 2] = np.float32(ex * ex / 9.0)                     # the variance that meets the excess: on the threshold ...
    while not ex * ex <= 9.0 * float(var[2, 2]):
        var[2, 2] = np.nextafter(var[2, 2], np.float32(1))
    y[2, 3], var[2, 3] = y[2, 2], np.nextafter(var[2, 2], np.float32(0))   # ... and one float below it
    labels, counts, pixel, xyz = segment_of(cover, depth, var, y, K, ms, sf, 0.5, sig, 3.0)
    lab = labels.reshape(rows, cols)
    assert lab[0].tolist() == [0, -1, 0, 1, 0, 0]
    assert lab[1].tolist() == [-1, -1, -1, 0, 0, 0]
    assert lab[2].tolist() == [0, -1, 0, -1, 0, 0]
    assert counts.tolist() == [(lab == 0).sum(), 1] and counts.sum() == pixel.size
    assert (np.diff(pixel) > 0).all() and (labels[pixel] >= 0).all()
    assert xyz.dtype == np.float32 and np.array_equal(xyz[:, 2], y.ravel()[pixel])


def test_segment_of_a_pixel_exactly_on_each_threshold():
    """Parameters whose products are exact in binary64: tau = 1 x (0.25 + 0 x D^2) = 0.25, depth_sigmas^2 = 1."""
    rows, cols, K, cover, depth, var, y = _seg_inputs()
    cover[0] = 0.25                                           # = min_cover
    cover[0, 3, 5] = np.nextafter(np.float32(0.25), np.float32(0))
    y[0, 0], y[0, 1] = 1.25, 0.75                             # |y - D| = tau, zero variance: excess 0 <= 0
    y[0, 2] = np.nextafter(np.float32(1.25), np.float32(2))   # one float past tau
    y[1, 0], var[1, 0] = 1.5, 0.0625                          # excess 0.25, squared 0.0625 = 1 x var
    y[1, 1], var[1, 1] = 1.5, np.nextafter(np.float32(0.0625), np.float32(0))
    y[1, 2], var[1, 2] = 0.5, 0.0625                          # the same in front of the surface
    lab = segment_of(cover, depth, var, y, K, 0.25, 0.0, 0.25, 1.0, 1.0)[0].reshape(rows, cols)
    assert lab[0, :3].tolist() == [0, 0, -1] and lab[1, :3].tolist() == [0, -1, 0] and lab[3, 5] == -1 and lab[3, 4] == 0


def test_segment_of_point_coordinates_at_the_four_corners():
    rows, cols, K, cover, depth, var, y = _seg_inputs()
    cover[0] = 1.0
    y[:] = np.float32(1.0) + np.float32(0.001) * np.arange(rows * cols, dtype=np.float32).reshape(rows, cols)
    var[:] = 1.0
    labels, counts, pixel, xyz = segment_of(cover, depth, var, y, K, 0.003, 0.0014247)
    assert counts.tolist() == [rows * cols, 0] and pixel.tolist() == list(range(rows * cols))
    for r, c in ((0, 0), (0, cols - 1), (rows - 1, 0), (rows - 1, cols - 1)):
        z = float(y[r, c])
        want = (np.float32((c - K[0, 2]) / K[0, 0] * z), np.float32((r - K[1, 2]) / K[1, 1] * z), y[r, c])
        assert tuple(xyz[r * cols + c]) == want, (r, c)
    assert xyz[0, 0] < 0 < xyz[cols - 1, 0] and xyz[0, 1] < 0 < xyz[-1, 1]          # integer sample coordinates about (cx, cy)


# ---------------------------------------------------------------- the C-ABI, the kernels' compiler report, the mirrors
NAMES = ("rbs_object_map", "rbs_object_map_ms", "rbs_object_map_info", "rbs_object_segment", "rbs_tracker_set_object_map",
         "rbs_tracker_object_map", "rbs_tracker_object_map_ms", "rbs_tracker_poses")


def test_c_abi_has_the_entry_points_and_the_parameter_layout():
    lib = _capi.load()
    header = open(os.path.join(INC, "rbsensor_mi355x.h")).read()
    for s in NAMES:
        assert hasattr(lib, s) and s in _capi.EXPORTS, s
        assert re.search(r"^int32_t %s\(" % s, header, re.M), s
    assert "rbs_object_segment_default_params" in _capi.EXPORTS and "Object map" in header
    Pm = _capi.RbsObjectSegmentParams
    assert C.sizeof(Pm) == 32 and [f[0] for f in Pm._fields_] == ["min_cover", "sigmas", "depth_sigmas", "reserved"]
    body = re.search(r"typedef struct rbs_object_segment_params \{(.*?)\} rbs_object_segment_params;", header, re.S).group(1)
    assert re.findall(r"double\s+(\w+)", body) == ["min_cover", "sigmas", "depth_sigmas", "reserved"]
    p, a = Pm(), _capi.RbsAssessParams()
    lib.rbs_object_segment_default_params(C.byref(p))
    lib.rbs_assess_default_params(C.byref(a))
    assert (p.min_cover, p.sigmas, p.depth_sigmas, p.reserved) == (0.5, a.sigmas, 3.0, 0.0)
    assert RbSensor.object_segment_default_params() == dict(min_cover=0.5, sigmas=a.sigmas, depth_sigmas=3.0)
    out = (C.c_float * 4)()
    iout = (C.c_int32 * 8)()
    inv = _capi.RBS_ERR_INVALID_ARGUMENT
    assert lib.rbs_object_map(None, None, 1, None, None, 1, out, out, out) == inv
    assert lib.rbs_object_map_ms(None, out) == inv and lib.rbs_object_map_info(None, iout) == inv
    assert lib.rbs_object_segment(None, None, None, None, None, iout, iout, iout, out, 1, iout) == inv
    assert lib.rbs_tracker_set_object_map(None, 1) == inv and lib.rbs_tracker_object_map(None, None, out, out, out) == inv
    assert lib.rbs_tracker_object_map_ms(None, out) == inv and lib.rbs_tracker_poses(None, None) == inv
    assert lib.rbs_abi_version() == _capi.RBS_ABI_VERSION == 2


def test_objmap_kernels_use_no_scratch_and_spill_no_vector_register():
    """Every rbs_objmap_* kernel, and seven of them.  (Scalar registers parked in vector lanes are not memory traffic: the
    plane render kernel the render kernel is built from has some too.)"""
    txt = open(os.path.join(LIB, "resource_usage.txt")).read()
    seen = {}
    for m in re.finditer(r"Function Name: (\S*rbs_objmap_\w*kernel\S*).*?ScratchSize \[bytes/lane\]: (\d+).*?VGPRs Spill: (\d+)", txt, re.S):
        seen[m.group(1)] = (int(m.group(2)), int(m.group(3)))
    names = " ".join(seen)
    for k in ("rbs_objmap_rects_kernel", "rbs_objmap_live_kernel", "rbs_objmap_render_kernel", "rbs_objmap_fold_kernel",
              "rbs_objmap_segment_kernel", "rbs_objmap_scan_kernel", "rbs_objmap_points_kernel"):
        assert k in names, (k, sorted(seen))
    assert len(seen) == 7 and all(v == (0, 0) for v in seen.values()), seen


def test_python_surface():
    assert inspect.signature(DeviceParticleTracker.__init__).parameters["object_map"].default is False
    for cls in (ParticleTracker, DeviceParticleTracker):
        assert callable(cls.object_map) and callable(cls.segment) and callable(cls.poses)
    assert inspect.signature(ParticleTracker.segment).parameters["params"].default is None
    sig = inspect.signature(RbSensor.object_map).parameters
    assert sig["members"].default is None and sig["log_weights"].default is None
    assert list(inspect.signature(RbSensor.object_segment).parameters)[1:] == ["maps", "params", "capacity"]
    m = ObjectMap(cover=np.zeros((1, 2, 2), np.float32), depth=np.zeros((2, 2), np.float32), var=np.zeros((2, 2), np.float32), frame=3)
    assert m.frame == 3 and Segmentation(labels=None, counts=None, pixel=None, xyz=None).xyz is None


def test_cpp_mirror_compiles_and_its_program_runs_or_fails_loudly(tmp_path):
    tu = tmp_path / "only_the_header.cpp"
    tu.write_text("#include <dbot_amd/rb_sensor_builder.hpp>\n"
                  "dbot_amd::ParticleTracker::ObjectMap (dbot_amd::ParticleTracker::*f)() const = &dbot_amd::ParticleTracker::object_map;\n"
                  "void (dbot_amd::ParticleTracker::*g)(bool) = &dbot_amd::ParticleTracker::enable_object_map;\n"
                  "typedef dbot_amd::RbSensor<> S;\n"
                  "S::ObjectMap (S::*h)(const S::RealArray&, const S::IntArray&, const S::RealArray&) = &S::object_map;\n"
                  "S::Segmentation (S::*s)(const S::ObjectMap*, const rbs_object_segment_params*) = &S::object_segment;\n")
    r = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I" + INC, str(tu)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr[-3000:]
    exe = str(tmp_path / "object_map_check")
    r = subprocess.run(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + INC, "-o", exe, os.path.join(HERE, "cpp", "object_map_check.cpp"),
                        "-L" + LIB, "-lrbsensor_mi355x", "-Wl,-rpath," + LIB, "-Wl,-rpath,/opt/rocm/lib"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    if _capi.load().rbs_device_count() <= 0:
        run = subprocess.run([exe, str(tmp_path / "missing.bin")], capture_output=True, text=True, timeout=120)
        assert run.returncode == 0 and run.stdout.startswith("NO_DEVICE") and "no CPU path" in run.stdout, (run.stdout, run.stderr[-2000:])


def test_node_takes_the_flag_and_the_yaml_key_is_optional(tmp_path):
    assert inspect.signature(node.build_particle_tracker).parameters["object_map"].default is False
    assert inspect.signature(node.replay_dataset).parameters["object_map"].default is False
    cfg = os.path.join(HERE, "golden", "reference_config")
    files = [os.path.join(cfg, f) for f in ("particle_tracker.yaml", "camera.yaml", "object.yaml")]
    tree = node.load_rosparams(*files)
    assert "object_map" not in tree["particle_filter"]
    text = open(files[0]).read()
    mine = tmp_path / "particle_tracker.yaml"
    mine.write_text(text.replace("particle_filter:\n", "particle_filter:\n  object_map: true\n"))
    keyed = node.load_rosparams(str(mine), *files[1:])
    assert keyed["particle_filter"].pop("object_map") is True
    assert keyed == tree
