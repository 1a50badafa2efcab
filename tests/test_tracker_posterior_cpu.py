"""The particle tracker's posterior report without a device: the numpy twin (dbot_ros_amd.tracker.posterior_of) against brute
force in np.longdouble on planted populations, survivors on planted slot maps, the object-frame Jacobian against central
finite differences of _from_model, the C-ABI's two entry points, the compiler's report of the rbs_post_* kernels, and the C++
mirror.  Bars: tests/posterior_twin.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import oracle_binding as ob
import posterior_twin as pt
import scenarios as sc
from dbot_ros_amd import _capi, node, pose, synth
from dbot_ros_amd.tracker import (BODY, ObjectTransitionBuilder, ParticleTracker, ParticleTrackerBuilder, Posterior,
                                  object_frame_jacobian, posterior_of)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
INC = os.path.join(ROOT, "include")
LIB = os.path.join(ROOT, "dbot_ros_amd", "lib")


# ---------------------------------------------------------------- the twin against brute force
@pytest.mark.parametrize("parts", [1, 3])
@pytest.mark.parametrize("n", [1, 2, 65, 1000])
@pytest.mark.parametrize("kind", pt.KINDS)
def test_twin_matches_brute_force(kind, n, parts):
    x, lw, idx = pt.population(kind, n, parts)
    rep = posterior_of(x, lw, idx, resampled=True, frame=3)
    ref = pt.check(rep, x, lw, idx)
    assert rep.resampled is True and rep.frame == 3 and rep.mean.shape == (parts * BODY,) and rep.cov.shape == (parts * BODY,) * 2
    if kind == "uniform":
        assert rep.ess == n
    if kind == "dominant" and n > 1:
        assert 1.0 <= rep.ess < 1.0 + 1e-15 * n + 1e-9
    if kind == "identical":
        assert np.abs(rep.cov).max() <= pt.bars(ref, x)[0].max()     # zero up to the floor the mean's rounding leaves
    if n == 1:
        assert rep.ess == 1.0 and not rep.cov.any() and np.array_equal(rep.mean, x[0])
    if parts == 3 and kind == "uniform" and n == 1000:     # the planted cross-body correlation is there to be seen
        c01 = rep.cov[0, BODY] / np.sqrt(rep.cov[0, 0] * rep.cov[BODY, BODY])
        assert c01 > 0.5


def test_the_eigenvalue_instrument_decides_without_an_allowance():
    """smallest_eigenvalue_at_least on matrices whose smallest eigenvalue is known: a rank-one matrix (D - 1 eigenvalues
    exactly 0 up to its entries' rounding) moved by +-t I, two ulps either side of the threshold."""
    rng = np.random.default_rng(2)
    Q, _ = np.linalg.qr(rng.standard_normal((36, 36)))
    for lam in (1e-4, 3e-9):
        A = (Q * np.r_[lam, 1.0, np.linspace(2, 3, 34)]) @ Q.T          # eigenvalues lam, 1, 2 .. 3
        A = np.triu(A) + np.triu(A, 1).T
        true = float(np.linalg.eigvalsh(A).min())
        assert abs(true - lam) <= 1e-14
        assert pt.smallest_eigenvalue_at_least(A, lam - 1e-13) and not pt.smallest_eigenvalue_at_least(A, lam + 1e-13)
        assert pt.smallest_eigenvalue_at_least(-A, -3.0 - 1e-13) and not pt.smallest_eigenvalue_at_least(-A, -3.0 + 1e-13)
    Z = np.zeros((12, 12))
    assert pt.smallest_eigenvalue_at_least(Z, 0.0) and pt.smallest_eigenvalue_at_least(Z, -1e-300) and not pt.smallest_eigenvalue_at_least(Z, 1e-300)
    v = rng.standard_normal(24)
    R1 = np.outer(v, v)                                                  # rank one: smallest eigenvalue 0 up to 24 u |v|^2
    assert pt.smallest_eigenvalue_at_least(R1, -1e-13 * (v @ v)) and not pt.smallest_eigenvalue_at_least(R1, 1e-13 * (v @ v))


def test_one_pass_restatement_fails_where_the_two_pass_rule_holds():
    """Velocities with a mean 1 000 times their spread: raw moments minus mean mean^T cancel six digits and miss the bar."""
    x, lw, idx = pt.population("velocity", 1000, 1)
    ref = pt.reference(x, lw, idx)
    cov_bar = pt.bars(ref, x)[0]
    e = np.exp(lw - lw.max())
    mean = (e[:, None] * x).sum(0) / e.sum()
    one_pass = (e[:, None] * x).T @ x / e.sum() - np.outer(mean, mean)
    err = np.abs(one_pass - ref["cov"].astype(np.float64))
    assert (err[6:, 6:] > cov_bar[6:, 6:]).any(), "the case does not tell the rules apart"
    two_pass = posterior_of(x, lw, idx).cov
    assert (np.abs(two_pass - ref["cov"].astype(np.float64)) <= cov_bar).all()


def test_survivors_on_planted_slot_maps():
    x, lw, _ = pt.population("uniform", 100, 1)
    for idx, want in ((np.arange(100), 100), (np.zeros(100, int), 1), (np.arange(100) // 7, 15), (np.r_[np.full(99, 42), 99], 2),
                      (np.arange(100)[::-1] % 50, 50)):
        assert posterior_of(x, lw, idx.astype(np.int32)).survivors == want


# ---------------------------------------------------------------- the object-frame conversion
def _tracker(center, parts=1):
    names = ("m1_l2", "box12", "m1_l2")[:parts]
    om, cam, P = sc.make_scene(names, 80, 60, max_particles=8)
    o = ob.Oracle(om, cam, P, max_particles=8, mode=ob.EAGER)
    tp = ParticleTrackerBuilder.Parameters(evaluation_count=8 * parts, center_object_frame=center)
    trans = ObjectTransitionBuilder(ObjectTransitionBuilder.Parameters(part_count=parts)).build()
    tr = ParticleTracker(trans, o, om, tp, np.random.default_rng(0))
    tr.centers = np.array([[0.03, -0.02, 0.05], [-0.04, 0.01, 0.02], [0.0, 0.06, -0.01]])[:parts]   # (the synthetic meshes are centred already)
    return tr, om


def test_object_frame_jacobian_against_central_differences():
    tr, om = _tracker(True, parts=2)
    rng = np.random.default_rng(5)
    z = np.zeros((2, BODY))
    z[:, 0:3] = rng.normal([0, 0, 0.8], 0.1, (2, 3))
    z[:, 3:6] = rng.normal(0, 0.9, (2, 3))

    def published(b, delta):          # the published pose of body b after a model perturbation (dt, dtheta from the left)
        s = z.copy()
        s[b, 0:3] += delta[0:3]
        s[b, 3:6] = pose.matrix_to_rotvec(pose.rotvec_to_matrix(delta[3:6]) @ pose.rotvec_to_matrix(z[b, 3:6]))
        out = tr._from_model(s.ravel()).reshape(2, BODY)[b]
        base = tr._from_model(z.ravel()).reshape(2, BODY)[b]
        dR = pose.rotvec_to_matrix(out[3:6]) @ pose.rotvec_to_matrix(base[3:6]).T
        return np.concatenate([out[0:3] - base[0:3], pose.matrix_to_rotvec(dR)])

    h = 1e-6
    for b in range(2):
        J = object_frame_jacobian(pose.rotvec_to_matrix(z[b, 3:6]), tr.centers[b])
        fd = np.stack([(published(b, h * np.eye(6)[k]) - published(b, -h * np.eye(6)[k])) / (2 * h) for k in range(6)], axis=1)
        assert np.abs(J - fd).max() <= 1e-9, np.abs(J - fd).max()     # central differences: h^2 = 1e-12 truncation, 1e-10 rounding
        assert np.abs(J[0:3, 3:6]).max() > 1e-2                        # (a centring offset that matters)


def test_pose_covariance_is_J_C_Jt_and_the_model_block_without_centring():
    x, lw, idx = pt.population("spread", 200, 2)
    rep = posterior_of(x, lw, idx)
    for center in (True, False):
        tr, om = _tracker(center, parts=2)
        tr.default = np.random.default_rng(1).normal(0, 0.5, 2 * BODY)
        pc = tr.pose_covariance(rep)
        assert pc.shape == (2, 6, 6)
        for b in range(2):
            C6 = rep.cov[BODY * b:BODY * b + 6, BODY * b:BODY * b + 6]
            if center:
                J = object_frame_jacobian(pose.rotvec_to_matrix(tr.default[BODY * b + 3:BODY * b + 6]), tr.centers[b])
                assert np.allclose(pc[b], J @ C6 @ J.T, rtol=1e-14, atol=0) and not np.allclose(pc[b], C6)
                assert np.array_equal(pc[b][3:, 3:], C6[3:, 3:])       # the rotation block is the model's
            else:
                assert np.array_equal(pc[b], C6)


def test_host_tracker_reports_its_own_population():
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
        tr.posterior()
    rng = np.random.default_rng(8)
    for k in (1, 2):
        tr.track(synth.make_frame(o.render_depth(synth.truth_pose(1, frame=k)), 60, 80, rng, occluder=False))
        rep = tr.posterior()
        assert isinstance(rep, Posterior) and rep.n == n and rep.frame == k and rep.resampled and rep.ess == n
        assert 1 <= rep.survivors <= n
        pt.check(rep, tr.particles, tr.log_weights, tr.indices)


# ---------------------------------------------------------------- the C-ABI, the kernels' compiler report, the mirrors
def test_c_abi_has_the_two_entry_points_and_refuses_a_null_tracker():
    lib = _capi.load()
    for s in ("rbs_tracker_set_posterior", "rbs_tracker_posterior"):
        assert hasattr(lib, s) and s in _capi.EXPORTS
    assert lib.rbs_tracker_set_posterior(None, 1) == _capi.RBS_ERR_INVALID_ARGUMENT
    info = _capi.RbsTrackerPosteriorInfo()
    assert lib.rbs_tracker_posterior(None, C.byref(info), None, None) == _capi.RBS_ERR_INVALID_ARGUMENT
    assert C.sizeof(_capi.RbsTrackerPosteriorInfo) == 24 and _capi.RbsTrackerPosteriorInfo.ess.offset == 16
    assert lib.rbs_abi_version() == _capi.RBS_ABI_VERSION


def test_posterior_kernels_use_no_scratch_and_spill_nothing():
    txt = open(os.path.join(LIB, "resource_usage.txt")).read()
    seen = {}
    for m in re.finditer(r"Function Name: (\S*rbs_post_\w*kernel\S*).*?ScratchSize \[bytes/lane\]: (\d+).*?SGPRs Spill: (\d+).*?VGPRs Spill: (\d+)",
                         txt, re.S):
        seen[m.group(1)] = tuple(int(m.group(k)) for k in (2, 3, 4))
    names = " ".join(seen)
    for k in ("rbs_post_kernel", "rbs_post_recentre_kernel", "rbs_post_max_kernel", "rbs_post_sums_kernel", "rbs_post_mean_kernel",
              "rbs_post_cov_kernel", "rbs_post_cov_fold_kernel"):
        assert k in names, (k, sorted(seen))
    assert len(seen) == 7 and all(v == (0, 0, 0) for v in seen.values()), seen


def test_release_library_has_no_posterior_probe_and_the_hooks_build_has():
    assert b"rbs_test_posterior" not in open(os.path.join(LIB, "librbsensor_mi355x.so"), "rb").read()
    assert b"rbs_test_posterior\0" in open(os.path.join(LIB, "librbsensor_mi355x_hooks.so"), "rb").read()


def test_cpp_mirror_compiles_and_its_program_runs_or_fails_loudly(tmp_path):
    tu = tmp_path / "only_the_header.cpp"
    tu.write_text("#include <dbot_amd/rb_sensor_builder.hpp>\n"
                  "dbot_amd::ParticleTracker::Posterior (dbot_amd::ParticleTracker::*f)() const = &dbot_amd::ParticleTracker::posterior;\n"
                  "void (dbot_amd::ParticleTracker::*g)(bool) = &dbot_amd::ParticleTracker::enable_posterior;\n")
    r = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I" + INC, str(tu)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr[-3000:]
    exe = str(tmp_path / "posterior_check")
    r = subprocess.run(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + INC, "-o", exe, os.path.join(HERE, "cpp", "posterior_check.cpp"),
                        "-L" + LIB, "-lrbsensor_mi355x", "-Wl,-rpath," + LIB, "-Wl,-rpath,/opt/rocm/lib"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    if _capi.load().rbs_device_count() <= 0:
        run = subprocess.run([exe, str(tmp_path / "missing.bin")], capture_output=True, text=True, timeout=120)
        assert run.returncode == 0 and run.stdout.startswith("NO_DEVICE") and "no CPU path" in run.stdout, (run.stdout, run.stderr[-2000:])


def test_node_takes_the_flag_and_the_yaml_key_is_optional():
    import inspect
    assert inspect.signature(node.build_particle_tracker).parameters["posterior"].default is False
    assert inspect.signature(node.replay_dataset).parameters["posterior"].default is False
    cfg = os.path.join(HERE, "golden", "reference_config")
    tree = node.load_rosparams(*(os.path.join(cfg, f) for f in ("particle_tracker.yaml", "camera.yaml", "object.yaml")))
    assert "posterior" not in tree["particle_filter"]     # the reference's own file: the key is absent, the report off
