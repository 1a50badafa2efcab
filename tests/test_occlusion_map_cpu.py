"""The occlusion map without a device: the numpy twin's identities (dbot_ros_amd.tracker.occlusion_map_of), the per-body
summary's restatement on planted planes, the C-ABI's entry points and record layout, the YAML key, the compiler's report of
the rbs_occmap_* kernels, and the C++ mirror.  Bars: tests/occmap_twin.py."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import occmap_twin as ot
from dbot_ros_amd import _capi, node
from dbot_ros_amd.tracker import BodyOcclusion, DeviceParticleTracker, OcclusionMap, ParticleTracker, occlusion_map_of

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
INC = os.path.join(ROOT, "include")
LIB = os.path.join(ROOT, "dbot_ros_amd", "lib")
ROWS, COLS, SLOTS = 60, 80, 6


def _planes(seed=0):
    return ot.planted_planes(ROWS, COLS, SLOTS, np.float32(0.1), seed)


# ---------------------------------------------------------------- the twin's identities
def test_identical_planes_give_that_plane_bit_for_bit():
    """sum W_s v / S with every v the same float: W = S up to n roundings of 2^-53, far inside the float's half spacing."""
    p = _planes()[3]
    for name, n, idx, lw in ot.populations(SLOTS, seed=1):
        m = occlusion_map_of({s: p for s in range(SLOTS)}, lw, idx)
        assert np.array_equal(m.astype(np.float32), p), name


def test_one_finite_weight_gives_that_slots_plane():
    planes = _planes()
    for n in ot.SIZES:
        idx = (np.arange(n) % SLOTS).astype(np.int32)
        lw = np.full(n, -np.inf)
        lw[n // 2] = -7.25
        m = occlusion_map_of(planes, lw, idx)
        assert np.array_equal(m.astype(np.float32), planes[int(idx[n // 2])]), n


def test_map_lies_between_the_planes_and_is_the_background_outside_every_window():
    planes = _planes()
    stack = np.stack([planes[s] for s in range(SLOTS)])
    for name, n, idx, lw in ot.populations(SLOTS, seed=2):
        m = occlusion_map_of(planes, lw, idx).astype(np.float32)
        live = np.unique(idx if lw is None else idx[np.isfinite(lw)])
        assert (m >= stack[live].min(axis=0)).all() and (m <= stack[live].max(axis=0)).all(), name
        outside = (stack[live] == np.float32(0.1)).all(axis=0)
        assert outside.any() and (m[outside] == np.float32(0.1)).all(), name


def test_permuting_the_members_stays_within_the_bar():
    planes = _planes()
    rng = np.random.default_rng(4)
    for name, n, idx, lw in ot.populations(SLOTS, seed=3):
        ref = occlusion_map_of(planes, lw, idx)
        perm = rng.permutation(n)
        got = occlusion_map_of(planes, None if lw is None else lw[perm], idx[perm])
        assert (np.abs(got - ref) <= ot.LD(n + 16) * ot.LD(2.0) ** -52).all(), name
        ot.check(got.astype(np.float32), ref, n, what=name)


def test_uniform_weights_are_the_plain_mean_and_arrays_serve_as_planes():
    planes = _planes()
    stack = np.stack([planes[s] for s in range(SLOTS)])
    idx = np.array([1, 1, 2, 5], dtype=np.int32)
    want = (2 * stack[1].astype(np.float64) + stack[2] + stack[5]) / 4
    for lw in (None, np.zeros(4), np.full(4, -3.0)):
        assert np.abs(occlusion_map_of(stack, lw, idx).astype(np.float64) - want).max() <= 2.0 ** -50


def test_the_bar_is_half_a_float_spacing_plus_the_binary64_term():
    t = np.array([0.1, 0.5, 0.75, 1.0], dtype=ot.LD)
    b = ot.bar(t, 300)
    assert np.array_equal(ot.spacing32_below(t).astype(np.float64), [2.0 ** -27, 2.0 ** -24, 2.0 ** -24, 2.0 ** -23])
    assert np.allclose(b.astype(np.float64), 0.5 * np.array([2.0 ** -27, 2.0 ** -24, 2.0 ** -24, 2.0 ** -23]) + 316 * 2.0 ** -52, rtol=1e-12)
    just_below_one = ot.LD(1.0) - ot.LD(2.0) ** -40       # rounds to 1.0f, lies in the binade below
    assert float(ot.spacing32_below(just_below_one)) == 2.0 ** -24


# ---------------------------------------------------------------- the per-body summary restated
def test_bodies_restatement_on_planted_planes():
    npx = 12
    planes = np.full((2, npx), np.inf, dtype=np.float32)
    planes[0, 0:6] = 0.7
    planes[1, 4:10] = [0.6, 0.7, 0.8, 0.8, 0.8, np.inf]      # pixel 4: body 1 nearer; pixel 5: a tie, body 0 keeps it
    m = np.zeros(npx, dtype=np.float32)
    m[0], m[1], m[2] = 0.5, np.nextafter(np.float32(0.5), np.float32(1)), 1.0
    m[4], m[6] = 0.25, 0.75
    got = ot.bodies_of(planes, m, 0.5)
    # body 0 owns 0, 1, 2, 3, 5; body 1 owns 4, 6, 7, 8
    assert got[0].tolist() == [5, 2, (1 << 31) + ((1 << 31) + (1 << 8)) + (1 << 32)]
    assert got[1].tolist() == [4, 1, (1 << 30) + 3 * (1 << 30)]


# ---------------------------------------------------------------- the C-ABI, the kernels' compiler report, the mirrors
def test_c_abi_has_the_entry_points_and_the_record_layout():
    lib = _capi.load()
    names = ("rbs_occlusion_mean", "rbs_occlusion_mean_ms", "rbs_occlusion_bodies", "rbs_tracker_set_occlusion_map",
             "rbs_tracker_occlusion_map", "rbs_tracker_occlusion_map_ms")
    for s in names:
        assert hasattr(lib, s) and s in _capi.EXPORTS, s
    B = _capi.RbsOcclusionBody
    assert C.sizeof(B) == 32 and (B.rendered.offset, B.occluded.offset, B.sum_q32.offset, B.reserved.offset) == (0, 4, 8, 16)
    assert B.sum_q32.size == 8 and B.reserved.size == 16
    header = open(os.path.join(INC, "rbsensor_mi355x.h")).read()
    body = re.search(r"typedef struct rbs_occlusion_body \{(.*?)\} rbs_occlusion_body;", header, re.S).group(1)
    assert re.findall(r"(int32_t|int64_t)\s+(\w+)", body) == [("int32_t", "rendered"), ("int32_t", "occluded"), ("int64_t", "sum_q32"),
                                                              ("int32_t", "reserved")]
    for s in names:
        assert re.search(r"^int32_t %s\(" % s, header, re.M), s
    out = (C.c_float * 4)()
    assert lib.rbs_occlusion_mean(None, None, None, 1, out) == _capi.RBS_ERR_INVALID_ARGUMENT
    assert lib.rbs_occlusion_mean_ms(None, out) == _capi.RBS_ERR_INVALID_ARGUMENT
    assert lib.rbs_occlusion_bodies(None, out, None, 1, 0.5, None) == _capi.RBS_ERR_INVALID_ARGUMENT
    assert lib.rbs_tracker_set_occlusion_map(None, 1) == _capi.RBS_ERR_INVALID_ARGUMENT
    assert lib.rbs_tracker_occlusion_map(None, None, out) == _capi.RBS_ERR_INVALID_ARGUMENT
    assert lib.rbs_tracker_occlusion_map_ms(None, out) == _capi.RBS_ERR_INVALID_ARGUMENT
    assert lib.rbs_abi_version() == _capi.RBS_ABI_VERSION


def test_occmap_kernels_use_no_scratch_and_spill_nothing():
    txt = open(os.path.join(LIB, "resource_usage.txt")).read()
    seen = {}
    for m in re.finditer(r"Function Name: (\S*rbs_occmap_\w*kernel\S*).*?ScratchSize \[bytes/lane\]: (\d+).*?SGPRs Spill: (\d+).*?VGPRs Spill: (\d+)",
                         txt, re.S):
        seen[m.group(1)] = tuple(int(m.group(k)) for k in (2, 3, 4))
    names = " ".join(seen)
    for k in ("rbs_occmap_weights_kernel", "rbs_occmap_slots_kernel", "rbs_occmap_compact_kernel", "rbs_occmap_kernelE", "rbs_occmap_bodies_kernel"):
        assert k in names, (k, sorted(seen))
    assert len(seen) == 5 and all(v == (0, 0, 0) for v in seen.values()), seen


def test_python_surface():
    assert inspect.signature(DeviceParticleTracker.__init__).parameters["occlusion_map"].default is False
    for cls in (ParticleTracker, DeviceParticleTracker):
        assert callable(cls.occlusion_map) and callable(cls.occlusion_of_estimate)
    assert inspect.signature(ParticleTracker.occlusion_of_estimate).parameters["threshold"].default == 0.5
    m = OcclusionMap(plane=np.zeros((2, 2), np.float32), frame=3)
    assert m.frame == 3 and BodyOcclusion(rendered=4, occluded=1, mean=0.25).mean == 0.25


def test_cpp_mirror_compiles_and_its_program_runs_or_fails_loudly(tmp_path):
    tu = tmp_path / "only_the_header.cpp"
    tu.write_text("#include <dbot_amd/rb_sensor_builder.hpp>\n"
                  "dbot_amd::ParticleTracker::OcclusionMap (dbot_amd::ParticleTracker::*f)() const = &dbot_amd::ParticleTracker::occlusion_map;\n"
                  "void (dbot_amd::ParticleTracker::*g)(bool) = &dbot_amd::ParticleTracker::enable_occlusion_map;\n"
                  "typedef dbot_amd::RbSensor<> S;\n"
                  "std::vector<float> (S::*h)(const S::IntArray&, const S::RealArray&) = &S::occlusion_mean;\n")
    r = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I" + INC, str(tu)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr[-3000:]
    exe = str(tmp_path / "occlusion_map_check")
    r = subprocess.run(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + INC, "-o", exe, os.path.join(HERE, "cpp", "occlusion_map_check.cpp"),
                        "-L" + LIB, "-lrbsensor_mi355x", "-Wl,-rpath," + LIB, "-Wl,-rpath,/opt/rocm/lib"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    if _capi.load().rbs_device_count() <= 0:
        run = subprocess.run([exe, str(tmp_path / "missing.bin")], capture_output=True, text=True, timeout=120)
        assert run.returncode == 0 and run.stdout.startswith("NO_DEVICE") and "no CPU path" in run.stdout, (run.stdout, run.stderr[-2000:])


def test_node_takes_the_flag_and_the_yaml_key_is_optional(tmp_path):
    assert inspect.signature(node.build_particle_tracker).parameters["occlusion_map"].default is False
    assert inspect.signature(node.replay_dataset).parameters["occlusion_map"].default is False
    cfg = os.path.join(HERE, "golden", "reference_config")
    files = [os.path.join(cfg, f) for f in ("particle_tracker.yaml", "camera.yaml", "object.yaml")]
    tree = node.load_rosparams(*files)
    assert "occlusion_map" not in tree["particle_filter"]     # the reference's own file: the key is absent, the map off
    text = open(files[0]).read()
    assert text.count("particle_filter:\n") == 1
    mine = tmp_path / "particle_tracker.yaml"
    mine.write_text(text.replace("particle_filter:\n", "particle_filter:\n  occlusion_map: true\n"))
    keyed = node.load_rosparams(str(mine), *files[1:])
    assert keyed["particle_filter"].pop("occlusion_map") is True      # the key parses as a boolean beside the reference's own keys
    assert keyed == tree
