"""The robust Gaussian tracker on the CPU: the twin's arithmetic (tests/gauss_twin.py, DESIGN.md
Appendix G) against closed forms, its tracking on the synthetic sequence, the parameter surface, and
the library boundary without a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import gauss_twin as gt
import oracle_binding as ob
import scenarios as sc
from dbot_ros_amd import _capi, node
from dbot_ros_amd.gaussian import GaussianTrackerBuilder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE_CONFIG = os.path.join(ROOT, "tests", "golden", "reference_config")
GAUSS_SYMBOLS = ("rbs_gauss_create", "rbs_gauss_destroy", "rbs_gauss_initialize", "rbs_gauss_track", "rbs_gauss_track_f64",
                 "rbs_gauss_get_prior", "rbs_gauss_get_sigma_poses", "rbs_gauss_get_render", "rbs_gauss_get_moments",
                 "rbs_gauss_kernel_ms")


def _random_spd(rng, n, scale):
    A = rng.standard_normal((n, n))
    return scale * (A @ A.T / n + 0.5 * np.eye(n))


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300))


@pytest.mark.parametrize("parts", [1, 2])
def test_whitened_update_is_the_kalman_update_for_a_linear_observation(parts):
    """Depths linear in the pose (every pixel covered) and w = 0: the unscented transform is exact, so
    the whitened update must be the closed-form Kalman update, to 1e-12."""
    rng = np.random.default_rng(parts)
    tw = gt.GaussTwin(gt.Params(tail_weight=0.0, fg_noise_std=0.01), parts)
    D, NP, npx = tw.D, tw.NP, 40
    a = 0.7 + 0.1 * rng.random(npx)
    Cm = 0.5 * rng.standard_normal((npx, NP))
    mu = 1e-3 * rng.standard_normal(D)
    S = _random_spd(rng, D, 1e-4)
    mpf, Spf = tw.to_pf(mu, S)
    L = np.linalg.cholesky(Spf)
    X = tw.sigma_deltas(mpf, L)
    depths = (a[None] + X @ Cm.T).astype(np.float64)   # [nd, npx], no float rounding: the mock is exact
    y = a + Cm @ (mpf[:NP] + 0.01 * rng.standard_normal(NP)) + 0.01 * rng.standard_normal(npx)
    mup, Spp, _, _ = tw.whitened_update(mpf, L, depths, y)
    H = np.zeros((npx, D))
    H[:, :NP] = Cm
    Sy = H @ Spf @ H.T + tw.p.fg_noise_std ** 2 * np.eye(npx)
    K = Spf @ H.T @ np.linalg.inv(Sy)
    m_ref = mpf + K @ (y - a - H @ mpf)
    S_ref = Spf - K @ H @ Spf
    assert _rel(mup, m_ref) < 1e-12 and _rel(Spp, S_ref) < 1e-12, (_rel(mup, m_ref), _rel(Spp, S_ref))


def test_whitened_update_is_the_x_space_information_form():
    """On a rendered scene with the robust weights: the update equals the information form with
    H_i = P_xy,i^T (Sigma-)^-1, P_xy,i = L h_i, for a positive-definite prior."""
    om, cam, P = sc.make_scene(("m1",), 160, 120, max_particles=2)
    orc = ob.Oracle(om, cam, P, max_particles=2)
    (truth, y), = sc.make_frames(orc, 1, 1, seed=3)
    tw = gt.GaussTwin(gt.Params(), 1, orc.render_depth)
    rng = np.random.default_rng(0)
    z = gt.truth_state(truth)
    mu = np.concatenate([1e-3 * rng.standard_normal(6), 1e-3 * rng.standard_normal(6)])
    S = _random_spd(rng, 12, 2e-6)
    mpf, Spf = tw.to_pf(mu, S)
    L = np.linalg.cholesky(Spf)
    depths = np.stack([orc.render_depth(q) for q in tw.absolute_poses(z, tw.sigma_deltas(mpf, L))])
    mup, Spp, _, _ = tw.whitened_update(mpf, L, depths, y)
    pi, h, res, _ = tw.pixel_terms(depths, y)
    Pxy = np.zeros((12, h.shape[1]))
    Pxy[:] = L[:, :6] @ h
    Si = np.linalg.inv(Spf)
    H = Pxy.T @ Si                                      # [npx, D]
    info = Si + (H.T * pi) @ H
    S_ref = np.linalg.inv(info)
    m_ref = mpf + S_ref @ ((H.T * pi) @ res)
    assert (pi > 0).sum() > 500
    assert _rel(Spp, S_ref) < 1e-8 and _rel(mup - mpf, m_ref - mpf) < 1e-8, (_rel(Spp, S_ref), _rel(mup - mpf, m_ref - mpf))


def _track(meshes, tail_weight, n_frames=30, size=(160, 120)):
    om, cam, P = sc.make_scene(meshes, size[0], size[1], max_particles=2)
    orc = ob.Oracle(om, cam, P, max_particles=2)
    frames = sc.make_frames(orc, len(meshes), n_frames, seed=0)
    tw = gt.GaussTwin(gt.Params(tail_weight=tail_weight), len(meshes), orc.render_depth)
    tw.initialize(gt.truth_state(frames[0][0]))
    errs = []
    for truth, y in frames:
        z = tw.track(y)
        errs.append(np.linalg.norm((z - gt.truth_state(truth)).reshape(-1, 12)[:, 0:3], axis=1).max())
    return np.array(errs)


def test_twin_tracks_the_occluded_sequence_and_robustness_matters():
    """M1, 30 frames of scenarios.make_frames (occluding slab over a quarter of the object, 5 % NaN) at
    160x120, the reference's gaussian_tracker.yaml values.  Measured here: the robust filter's position
    error stays below 3.7 mm on every frame (1.6 mm at the end); bound 6 mm.  The same run with
    tail_weight = 0 -- every pixel trusted, the slab included -- is dragged off the object (0.93 m at
    the end); bound: beyond 0.1 m."""
    robust = _track(("m1",), 0.1)
    assert robust.max() < 6e-3, robust
    plain = _track(("m1",), 0.0)
    assert plain[-1] > 0.1, plain


def test_from_rosparam_reads_the_references_yaml():
    tree = node.load_rosparams(*(os.path.join(REFERENCE_CONFIG, f) for f in ("gaussian_tracker.yaml", "camera.yaml", "object.yaml")))
    p = GaussianTrackerBuilder.Parameters.from_rosparam(tree, part_count=len(tree["object"]["meshes"]), sensors=80 * 60)
    assert p.ut_alpha == 1.0 and p.moving_average_update_rate == 1.0 and p.center_object_frame is True
    o = p.observation
    assert (o.fg_noise_std, o.tail_weight, o.uniform_tail_min, o.uniform_tail_max, o.bg_depth, o.bg_noise_std, o.sensors) == \
        (0.001, 0.1, -5000.0, 5000.0, -3.0, 100.0, 4800)
    t = p.object_transition
    assert (t.linear_sigma_x, t.linear_sigma_y, t.linear_sigma_z) == (0.002, 0.002, 0.002)
    assert (t.angular_sigma_x, t.angular_sigma_y, t.angular_sigma_z, t.velocity_factor, t.part_count) == (0.01, 0.01, 0.01, 0.8, 1)
    cp = p.c_params()
    assert tuple(cp.linear_sigma) == (0.002,) * 3 and cp.ut_alpha == 1.0 and cp.tail_weight == 0.1
    tw = gt.Params.from_builder(p)
    assert tw.fg_noise_std == 0.001 and tw.bg_depth == -3.0


def test_every_gaussian_symbol_is_declared_and_exported():
    lib = C.CDLL(_capi.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "rbsensor_mi355x.h")).read()
    for s in GAUSS_SYMBOLS:
        assert s in _capi.EXPORTS and hasattr(lib, s) and (s + "(") in header, s


def _params(**kw):
    p = GaussianTrackerBuilder.Parameters().c_params()
    for k, v in kw.items():
        if k in ("linear_sigma", "angular_sigma"):
            setattr(p, k, (C.c_double * 3)(*v))
        else:
            setattr(p, k, v)
    return p


@pytest.mark.parametrize("bad, word", [
    (dict(linear_sigma=(0.002, -1.0, 0.002)), "sigma"), (dict(angular_sigma=(0.01, 0.01, -0.01)), "sigma"),
    (dict(ut_alpha=0.0), "alpha"), (dict(ut_alpha=-1.0), "alpha"), (dict(fg_noise_std=0.0), "fg_noise_std"),
    (dict(uniform_tail_min=1.0, uniform_tail_max=1.0), "uniform_tail"), (dict(tail_weight=1.0), "tail_weight"),
    (dict(tail_weight=-0.1), "tail_weight")])
def test_bad_parameters_are_rejected(bad, word):
    lib = _capi.load()
    out = C.c_void_p()
    assert lib.rbs_gauss_create(None, C.byref(_params(**bad)), C.byref(out)) == _capi.RBS_ERR_INVALID_ARGUMENT
    assert word.encode() in lib.rbs_last_error(None) and not out.value


def test_calls_fail_loudly_without_a_tracker_or_device():
    lib = _capi.load()
    out = C.c_void_p()
    assert lib.rbs_gauss_create(None, C.byref(_params()), C.byref(out)) == _capi.RBS_ERR_INVALID_ARGUMENT
    assert b"sensor is NULL" in lib.rbs_last_error(None)
    assert lib.rbs_gauss_create(None, None, C.byref(out)) == _capi.RBS_ERR_INVALID_ARGUMENT
    assert lib.rbs_gauss_initialize(None, None, None) == _capi.RBS_ERR_INVALID_ARGUMENT
    assert lib.rbs_gauss_track(None, None, None, None) == _capi.RBS_ERR_INVALID_ARGUMENT
    assert lib.rbs_gauss_track_f64(None, None, None, None) == _capi.RBS_ERR_INVALID_ARGUMENT
    assert lib.rbs_gauss_get_prior(None, None, None, None) == _capi.RBS_ERR_INVALID_ARGUMENT
    assert lib.rbs_gauss_get_sigma_poses(None, None, None) == _capi.RBS_ERR_INVALID_ARGUMENT
    assert lib.rbs_gauss_get_render(None, 0, None) == _capi.RBS_ERR_INVALID_ARGUMENT
    assert lib.rbs_gauss_kernel_ms(None, None) == _capi.RBS_ERR_INVALID_ARGUMENT
    out_e, n = (C.c_double * 27)(), C.c_int32(-1)
    assert lib.rbs_gauss_get_moments(None, out_e, C.byref(n)) == _capi.RBS_ERR_INVALID_ARGUMENT and n.value == -1
    assert lib.rbs_gauss_get_moments(None, None, None) == _capi.RBS_ERR_INVALID_ARGUMENT
    lib.rbs_gauss_destroy(None)   # no-op


DRIVER = r"""
#include <cmath>
#include <cstdio>
#include <dbot_amd/gaussian_tracker_builder.hpp>
int main()
{
    using namespace dbot_amd;
    GaussianTrackerBuilder<>::Parameters p;
    p.ori.meshes = {"tetra.obj"};
    p.object_transition.part_count = p.ori.count_meshes();
    p.observation.sensors = 80 * 60;
    std::vector<std::vector<Real>> v = {{0, 0, 0, 0.05, 0, 0, 0, 0.05, 0, 0, 0, 0.05}};
    std::vector<std::vector<int32_t>> t = {{0, 2, 1, 0, 1, 3, 0, 3, 2, 1, 2, 3}};
    auto om = std::make_shared<ObjectModel>(v, t, true);
    const Real K[9] = {570.3, 0, 319.5, 0, 570.3, 239.5, 0, 0, 1};
    auto cam = std::make_shared<CameraData>(CameraData::from_native(K, 640, 480, 8));
    try {
        auto tracker = GaussianTrackerBuilder<>(om, cam, p).build();
        FreeFloatingRigidBodiesState s0(1);
        s0.position(0)[2] = 0.7;
        tracker->initialize({s0});
        GaussianTracker::Obsrv frame(80 * 60, NAN);
        const auto s = tracker->track(frame);
        std::printf("OK %.6f %zu\n", s.position(0)[2], tracker->covariance().size());
    } catch (const std::exception& e) {
        std::printf("NO_DEVICE %s\n", e.what());
    }
    return 0;
}
"""


def test_cpp_mirror_compiles_and_runs(tmp_path):
    """A small driver against include/dbot_amd/gaussian_tracker_builder.hpp, built with g++ into tmp_path:
    without a device build() throws (no fallback); with one, a frame without readings leaves the pose."""
    src = tmp_path / "gauss_driver.cpp"
    src.write_text(DRIVER)
    exe = tmp_path / "gauss_driver"
    libdir = os.path.dirname(_capi.LIB_PATH)
    r = subprocess.run(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "include"), "-o", str(exe), str(src),
                        "-L" + libdir, "-lrbsensor_mi355x", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, check=True).stdout
    if _capi.load().rbs_device_count() > 0:
        assert out.startswith("OK ") and abs(float(out.split()[1]) - 0.7) < 1e-9 and out.split()[2] == "144", out
    else:
        assert out.startswith("NO_DEVICE") and "no CPU path" in out, out
