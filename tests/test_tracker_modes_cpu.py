"""The posterior modes without a device: the numpy twin (dbot_ros_amd.tracker.modes_of) against brute force in np.longdouble on
the planted populations, what each pattern is there to show, the yaml mapping, the C-ABI's entry points and struct layouts, the
refusals that need no device, the compiler's report of the rbs_modes_* kernels, and the C++ mirror.  Bars and margins:
tests/modes_twin.py."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import modes_twin as mt
import oracle_binding as ob
import scenarios as sc
from dbot_ros_amd import _capi, node, pose, synth
from dbot_ros_amd.tracker import (BODY, Mode, Modes, ModesParams, ObjectTransitionBuilder, ParticleTracker, ParticleTrackerBuilder, modes_of,
                                  modes_from_c, modes_params_c)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
INC = os.path.join(ROOT, "include")
LIB = os.path.join(ROOT, "dbot_ros_amd", "lib")
worst = {}


# ---------------------------------------------------------------- the twin against brute force
@pytest.mark.parametrize("parts", [1, 2, 3])
@pytest.mark.parametrize("n", [1, 2, 3, 63, 65, 257, 1025])
def test_twin_matches_brute_force(n, parts):
    for pattern in mt.PATTERNS + ((mt.BODIES_123,) if parts == 3 else ()):
        x, lw, P, ref = mt.planted(pattern, n, parts)
        assert min(b["margin"] for b in ref["bodies"]) >= mt.MARGIN
        got = modes_of(x, lw, P, frame=7)
        assert got.frame == 7 and len(got.bodies) == parts
        mt.check(got, ref, note=worst)
        mt.assert_pattern(pattern, n, got)
        assert mt.same_bits(got, modes_of(np.concatenate([x, np.ones((n, parts, 6))], axis=2).reshape(n, parts * BODY), lw, P, frame=7))
    print("worst share of the bars so far:", worst)


def test_the_coarse_stage_of_the_reference_changes_nothing(monkeypatch):
    """Above COARSE_FROM particles reference() takes the pair pass in binary64 first and np.longdouble only near a round's
    maximum: on a population small enough for both, the same seeds, values and no smaller a margin than it reports."""
    x, lw, P, full = mt.planted("many", 1025, 1)
    monkeypatch.setattr(mt, "COARSE_FROM", 256)
    coarse = mt.reference(x, lw, P)
    a, b = full["bodies"][0], coarse["bodies"][0]
    assert a["seeds"] == b["seeds"] and all(u == v for u, v in zip(a["rho_seed"], b["rho_seed"]))
    assert all(np.array_equal(u, v) for key in ("pos", "rot") for u, v in zip(a[key], b[key]))
    assert 0 < b["margin"] <= a["margin"]


def test_the_mean_of_a_split_cloud_lies_in_neither_hump():
    """Two clusters of mass 0.7 / 0.3, ten bandwidths apart: the weighted mean -- what the tracker publishes -- is further than
    one bandwidth from both modes, and mode 0 is the heavy one."""
    x, lw, P, _ = mt.planted("two", 1025, 1)
    m = modes_of(x, lw, P).bodies[0]
    e = np.exp(lw - lw.max())
    mean = (e[:, None] * x[:, 0, 0:3]).sum(0) / e.sum()
    assert m[0].mass > 0.6 > 0.4 > m[1].mass and abs(m[0].mass + m[1].mass - 1.0) < 0.05
    for mode in m[:2]:
        assert np.sum((mean - mode.delta[0:3]) ** 2) / P.h_t ** 2 > 1.0          # outside the core's translation radius already
    assert np.linalg.norm(m[0].delta[0:3] - m[1].delta[0:3]) > 9 * P.h_t


def test_quaternion_sign_and_the_branch_beyond_pi_do_not_matter():
    """The same population with every other rotation vector replaced by its equivalent beyond pi: the same seeds and masses,
    the same mean rotation (to the rot bar's order)."""
    x, lw, P, ref = mt.planted("tight", 257, 1)
    y = np.array(x)
    ang = np.linalg.norm(y[::2, 0, 3:6], axis=1)
    y[::2, 0, 3:6] *= (1.0 - 2.0 * np.pi / ang)[:, None]
    a, b = modes_of(x, lw, P).bodies[0], modes_of(y, lw, P).bodies[0]
    assert [m.seed for m in a] == [m.seed for m in b]
    assert np.abs(a[0].delta - b[0].delta).max() < 1e-12 and abs(a[0].mass - b[0].mass) < 1e-12


def test_weights_below_the_cut_are_no_belief():
    """A second cluster 640 log units down (e ~ 1e-278) is a mode, to the bars; 690 down (below 2^-960) it is none, and no member."""
    x, lw, P, ref = mt.faint(257, -640.0)
    got = modes_of(x, lw, P)
    mt.check(got, ref)
    assert len(got.bodies[0]) >= 2 and 0.0 < got.bodies[0][1].mass < 1e-270
    x, lw, P, ref = mt.faint(257, -690.0)
    got = modes_of(x, lw, P)
    mt.check(got, ref)
    seeds_far = [m for m in got.bodies[0] if x[m.seed, 0, 0] > 5 * P.h_t]
    assert not seeds_far and sum(m.mass for m in got.bodies[0]) == pytest.approx(1.0, abs=1e-12)


def test_params_are_checked_and_the_defaults_are_the_headers():
    for bad in (dict(h_t=0.0), dict(h_t=-1.0), dict(h_r=0.0), dict(h_r=1.5), dict(separation=0.5), dict(k_max=0), dict(k_max=9), dict(k_max=2.5)):
        with pytest.raises(ValueError):
            ModesParams(**bad).check()
    assert ModesParams(h_r=1.0, separation=1.0, k_max=8).check().k_max == 8
    c = _capi.RbsModesParams()
    _capi.load().rbs_modes_default_params(C.byref(c))
    d = ModesParams()
    assert (c.h_t, c.h_r, c.separation, c.k_max, c.reserved) == (d.h_t, d.h_r, d.separation, d.k_max, 0) == (0.02, 0.2, 2.0, 4, 0)
    back = modes_params_c(ModesParams(0.01, 0.5, 3.0, 7))
    assert (back.h_t, back.h_r, back.separation, back.k_max) == (0.01, 0.5, 3.0, 7)


# ---------------------------------------------------------------- the yaml mapping and the node
def test_yaml_key_is_optional_and_maps_the_four_parameters():
    cfg = os.path.join(HERE, "golden", "reference_config")
    tree = node.load_rosparams(*(os.path.join(cfg, f) for f in ("particle_tracker.yaml", "camera.yaml", "object.yaml")))
    assert "modes" not in tree["particle_filter"] and ModesParams.from_rosparam(tree) is None      # the reference's own file: off
    tree["particle_filter"]["modes"] = False
    assert ModesParams.from_rosparam(tree) is None
    tree["particle_filter"]["modes"] = True
    assert ModesParams.from_rosparam(tree) == ModesParams()
    tree["particle_filter"]["modes"] = {"h_t": 0.01, "k_max": 2}
    assert ModesParams.from_rosparam(tree) == ModesParams(h_t=0.01, k_max=2)
    tree["particle_filter"]["modes"] = {"h_t": 0.03, "h_r": 0.4, "separation": 2.5, "k_max": 6}
    assert ModesParams.from_rosparam(tree) == ModesParams(0.03, 0.4, 2.5, 6)
    for bad in ({"h_r": 3.0}, {"bandwidth": 1.0}, {"k_max": 0}):
        tree["particle_filter"]["modes"] = bad
        with pytest.raises(ValueError):
            ModesParams.from_rosparam(tree)
    import yaml
    assert ModesParams.from_rosparam(yaml.safe_load("particle_filter:\n  modes:\n    h_t: 0.015\n    separation: 3\n")) == ModesParams(h_t=0.015, separation=3.0)
    assert inspect.signature(node.build_particle_tracker).parameters["modes"].default is None
    assert inspect.signature(node.replay_dataset).parameters["modes"].default is False


def test_host_tracker_reports_its_own_population_with_published_poses():
    n = 24
    om, cam, P = sc.make_scene(("m1_l2",), 80, 60, max_particles=n)
    o = ob.Oracle(om, cam, P, max_particles=n, mode=ob.EAGER)
    tp = ParticleTrackerBuilder.Parameters(evaluation_count=n, max_kl_divergence=0.0)
    trans = ObjectTransitionBuilder(ObjectTransitionBuilder.Parameters()).build()
    tr = ParticleTracker(trans, o, om, tp, np.random.default_rng(3))
    Rt = synth.truth_pose(1, frame=0)[0]
    init = np.zeros(12)
    init[3:6] = pose.matrix_to_rotvec(Rt[:9].reshape(3, 3))
    init[0:3] = Rt[9:] - Rt[:9].reshape(3, 3) @ om.centers[0]
    tr.initialize([init])
    with pytest.raises(ValueError):
        tr.modes()
    tr.track(synth.make_frame(o.render_depth(synth.truth_pose(1, frame=1)), 60, 80, np.random.default_rng(8), occluder=False))
    m = tr.modes()
    assert isinstance(m, Modes) and m.frame == 1 and isinstance(m.bodies[0][0], Mode)
    mt.check(m, mt.reference(tr.particles.reshape(n, 1, BODY), tr.log_weights, ModesParams()))
    # the published pose: a zero delta is the estimate itself; a mode's is its delta on the frame's state
    est = tr._from_model(tr.default)[0:6]
    zero = tr._with_poses(Modes(bodies=[[Mode(0, 0.0, 0.0, 0.0, np.zeros(6))]]), tr.default).bodies[0][0].pose
    assert np.abs(zero - est).max() <= 1e-15
    assert m.bodies[0][0].pose.shape == (6,) and np.abs(m.bodies[0][0].pose[0:3] - est[0:3]).max() < 0.05
    moved = tr._with_poses(Modes(bodies=[[Mode(0, 0.0, 0.0, 0.0, np.r_[0.01, 0.0, 0.0, 0.0, 0.0, 0.0])]]), tr.default).bodies[0][0].pose
    assert np.allclose(moved - est, [0.01, 0, 0, 0, 0, 0], atol=1e-15)


# ---------------------------------------------------------------- the C-ABI, the kernels' compiler report, the mirrors
NEW = ("rbs_modes_default_params", "rbs_pose_modes", "rbs_tracker_set_modes", "rbs_tracker_modes", "rbs_tracker_modes_ms")


def test_c_abi_declares_and_exports_the_entry_points_and_stays_at_version_2():
    lib = _capi.load()
    header = open(os.path.join(INC, "rbsensor_mi355x.h")).read()
    for s in NEW:
        assert hasattr(lib, s) and s in _capi.EXPORTS and re.search(r"\b%s\(" % s, header), s
    assert "Posterior modes" in header and "#define RBS_MODES_MAX 8" in header and _capi.RBS_MODES_MAX == 8
    assert lib.rbs_abi_version() == _capi.RBS_ABI_VERSION == 2 and re.search(r"#define RBS_ABI_VERSION\s+2\b", header)


def test_struct_layouts():
    assert C.sizeof(_capi.RbsModesParams) == 32 and _capi.RbsModesParams.k_max.offset == 24
    assert C.sizeof(_capi.RbsMode) == 80 and _capi.RbsMode.density.offset == 8 and _capi.RbsMode.delta.offset == 32
    assert C.sizeof(_capi.RbsBodyModes) == 8 + 8 * 80 and _capi.RbsBodyModes.mode.offset == 8
    rec = (_capi.RbsBodyModes * 2)()
    rec[1].n_modes = 2
    rec[1].mode[1].seed, rec[1].mode[1].mass = 5, 0.25
    rec[1].mode[1].delta[5] = -1.5
    m = modes_from_c(rec, frame=3)
    assert m.frame == 3 and [len(b) for b in m.bodies] == [0, 2] and m.bodies[1][1].seed == 5 and m.bodies[1][1].mass == 0.25
    assert m.bodies[1][1].delta[5] == -1.5 and m.bodies[1][1].pose is None


def test_refusals_that_need_no_device():
    lib = _capi.load()
    c = modes_params_c(ModesParams())
    rec = (_capi.RbsBodyModes * 1)()
    x, lw = np.zeros(6), np.zeros(1)
    dp = C.POINTER(C.c_double)
    assert lib.rbs_pose_modes(None, x.ctypes.data_as(dp), lw.ctypes.data_as(dp), 1, C.byref(c), rec) == _capi.RBS_ERR_INVALID_ARGUMENT
    assert lib.rbs_tracker_set_modes(None, C.byref(c)) == _capi.RBS_ERR_INVALID_ARGUMENT
    assert lib.rbs_tracker_set_modes(None, None) == _capi.RBS_ERR_INVALID_ARGUMENT
    frame = C.c_int32()
    assert lib.rbs_tracker_modes(None, C.byref(frame), rec) == _capi.RBS_ERR_INVALID_ARGUMENT
    ms = C.c_float()
    assert lib.rbs_tracker_modes_ms(None, C.byref(ms)) == _capi.RBS_ERR_INVALID_ARGUMENT
    lib.rbs_modes_default_params(None)                                       # a null pointer is ignored


def test_modes_kernels_use_no_scratch_and_spill_nothing():
    txt = open(os.path.join(LIB, "resource_usage.txt")).read()
    seen = {}
    for m in re.finditer(r"Function Name: (\S*rbs_modes_\w*kernel\S*).*?ScratchSize \[bytes/lane\]: (\d+).*?SGPRs Spill: (\d+).*?VGPRs Spill: (\d+)",
                         txt, re.S):
        seen[m.group(1)] = tuple(int(m.group(k)) for k in (2, 3, 4))
    names = " ".join(seen)
    for k in ("rbs_modes_max_kernel", "rbs_modes_pack_kernel", "rbs_modes_density_kernel", "rbs_modes_select_kernel", "rbs_modes_assign_kernel",
              "rbs_modes_finish_kernel"):
        assert k in names, (k, sorted(seen))
    assert len(seen) == 6 and all(v == (0, 0, 0) for v in seen.values()), seen


def test_cpp_mirror_compiles_and_its_program_runs_or_fails_loudly(tmp_path):
    tu = tmp_path / "only_the_header.cpp"
    tu.write_text("#include <dbot_amd/rb_sensor_builder.hpp>\n"
                  "dbot_amd::ParticleTracker::Modes (dbot_amd::ParticleTracker::*f)() const = &dbot_amd::ParticleTracker::modes;\n"
                  "void (dbot_amd::ParticleTracker::*g)(bool) = &dbot_amd::ParticleTracker::enable_modes;\n"
                  "void (dbot_amd::ParticleTracker::*h)(const rbs_modes_params&) = &dbot_amd::ParticleTracker::enable_modes;\n")
    r = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I" + INC, str(tu)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr[-3000:]
    exe = str(tmp_path / "modes_check")
    r = subprocess.run(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + INC, "-o", exe, os.path.join(HERE, "cpp", "modes_check.cpp"),
                        "-L" + LIB, "-lrbsensor_mi355x", "-Wl,-rpath," + LIB, "-Wl,-rpath,/opt/rocm/lib"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    if _capi.load().rbs_device_count() <= 0:
        run = subprocess.run([exe, str(tmp_path / "missing.bin")], capture_output=True, text=True, timeout=120)
        assert run.returncode == 0 and run.stdout.startswith("NO_DEVICE") and "no CPU path" in run.stdout, (run.stdout, run.stderr[-2000:])
