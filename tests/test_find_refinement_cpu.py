"""The object finder's step 6b, the adaptive refinement, without a device: the numpy twin's identities (tests/find_refine_twin.py),
its order on ties and NaN, the parameters' round trip through rosparam, what the libraries export, and the six scenes of the
accuracy bar through the whole twin chain (foreground, seeds, hypotheses, selection, suppression, step 6b) scored by the CPU
oracle."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import find_fg_twin as fg
import find_refine_twin as rt
import find_twin as tw
import oracle_binding as ob
import scenarios as sc
from dbot_ros_amd import CameraData, _capi, synth
from dbot_ros_amd.finder import ObjectFinder
from test_find_foreground_cpu import scene_truth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RNG = np.random.default_rng(5)


def _spd(rng, scale=1e-4):
    A = rng.normal(size=(6, 6))
    return scale * (A @ A.T + 6.0 * np.eye(6))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---------------------------------------------------------------- the twin's identities
def test_the_factor_is_the_lower_cholesky_factor_and_reproduces_c():
    for _ in range(8):
        Cm = _spd(RNG)
        L = rt.factor(Cm, 1e-10)
        assert np.array_equal(L, np.tril(L)) and np.all(np.diag(L) > 0)
        np.testing.assert_allclose(L @ L.T, Cm, rtol=1e-13, atol=0)
        np.testing.assert_allclose(L, np.linalg.cholesky(Cm), rtol=1e-12, atol=0)
    C0 = rt.initial_covariance(math.radians(25.0), 0.015)
    sa, st = np.float64(math.radians(25.0)), np.float64(0.015)
    assert np.array_equal(rt.factor(C0, 1e-10), np.diag([np.sqrt(sa * sa)] * 3 + [np.sqrt(st * st)] * 3))


def test_mix_zero_with_shrink_one_keeps_c():
    Cm = _spd(RNG)
    d = RNG.normal(size=(16, 6))
    d[0] = 0.0
    scores = RNG.normal(size=16)
    out = rt.update(Cm, scores, d, elite=8, mix=0.0, shrink=1.0, jitter=0.0)
    assert np.array_equal(_bits(out), _bits(Cm))
    # ... and the jitter goes on the diagonal alone
    out = rt.update(Cm, scores, d, elite=8, mix=0.0, shrink=1.0, jitter=1e-6)
    assert np.array_equal(out - np.diag(np.diag(out)), Cm - np.diag(np.diag(Cm))) and np.array_equal(np.diag(out), np.diag(Cm) + 1e-6)


def test_an_elite_of_child_0_alone_shrinks_c():
    Cm = _spd(RNG)
    d = RNG.normal(size=(16, 6))
    d[0] = 0.0
    scores = np.full(16, -5.0)
    scores[0] = 1.0
    out = rt.update(Cm, scores, d, elite=1, mix=0.5, shrink=1.0, jitter=0.0)
    assert np.array_equal(out, 0.5 * Cm)                                           # M = 0: C <- (1 - mix) C
    out = rt.update(Cm, scores, d, elite=1, mix=0.25, shrink=0.5, jitter=0.0)
    assert np.array_equal(out, 0.5 * (0.75 * Cm))
    # mix 1: C is the elite's second moment about the survivor, whatever C was
    out = rt.update(Cm, np.arange(16.0), d, elite=4, mix=1.0, shrink=1.0, jitter=0.0)
    np.testing.assert_allclose(out, sum(np.outer(d[j], d[j]) for j in (15, 14, 13, 12)) / 4, rtol=1e-14, atol=1e-300)
    assert np.array_equal(out, out.T)


def test_a_zero_covariance_takes_the_fallback_factor():
    z = np.zeros((6, 6))
    assert np.array_equal(rt.factor(z, 1e-10), np.sqrt(1e-10) * np.eye(6))
    assert np.array_equal(rt.factor(z, 0.0), z)
    # the third pivot exactly 0, and a negative one: the diagonal of sqrt(max(C_ii, jitter))
    L = np.tril(RNG.integers(1, 4, size=(6, 6)).astype(np.float64))
    L[2, 2] = 0.0
    flat = L @ L.T                                                                  # small integers: exact
    want = np.diag(np.sqrt(np.maximum(np.diag(flat), 1e-10)))
    assert np.array_equal(rt.factor(flat, 1e-10), want)
    neg = flat.copy()
    neg[2, 2] -= 1.0
    assert np.array_equal(rt.factor(neg, 1e-10), np.diag(np.sqrt(np.maximum(np.diag(neg), 1e-10))))
    bad = np.diag([1.0, -2.0, np.nan, np.inf, 0.0, 4.0])
    assert np.array_equal(np.diag(rt.factor(bad, 0.25)), [1.0, 0.5, 0.5, np.inf, 0.5, 2.0])
    # with a diagonal factor d_a = L_aa n_a exactly
    nz = RNG.normal(size=(5, 6))
    assert np.array_equal(rt.perturb(want, nz), nz * np.diag(want))


def test_ties_nan_and_all_nan_rows():
    nan, inf = np.nan, np.inf
    assert rt.elite_order([1.0, 3.0, 3.0, 2.0, 3.0], 3).tolist() == [1, 2, 4]      # ties: ascending j
    assert rt.elite_order([nan, 1.0, nan, 5.0], 4).tolist() == [3, 1]               # NaN never: m = 2 < elite
    assert rt.elite_order([nan, nan, nan], 2).tolist() == []
    assert rt.elite_order([-inf, inf, 0.0, -0.0, nan], 5).tolist() == [1, 2, 3, 0]   # -0.0 == 0.0: j decides
    Cm = _spd(RNG)
    d = RNG.normal(size=(4, 6))
    assert np.array_equal(_bits(rt.update(Cm, [nan] * 4, d, 2, 0.5, 0.9, 1e-3)), _bits(Cm))     # m = 0: C stays, no jitter either
    # fewer numbers than the elite: the mean is over those m
    got = rt.update(Cm, [nan, 2.0, nan, 1.0], d, 3, 1.0, 1.0, 0.0)
    np.testing.assert_allclose(got, (np.outer(d[1], d[1]) + np.outer(d[3], d[3])) / 2, rtol=1e-14, atol=1e-300)
    # the elite's order is the order of the sum
    a = rt.update(Cm, [3.0, 2.0, 1.0, 0.0], d, 3, 1.0, 1.0, 0.0)
    acc = d[0, 0] * d[0, 1]
    acc = acc + d[1, 0] * d[1, 1]
    acc = acc + d[2, 0] * d[2, 1]
    assert a[0, 1] == (0.0 + acc) / 3.0 == a[1, 0]


def test_refinement_from_rosparam_round_trip():
    R, Pm = ObjectFinder.Refinement, ObjectFinder.Parameters
    assert Pm.from_rosparam({}).refinement is None and Pm().refinement is None
    p = Pm.from_rosparam({"object_finder": {"rounds": 12, "refinement": {}, "foreground": {}}})
    assert p.refinement == R() and p.rounds == 12 and p.foreground == ObjectFinder.Foreground()
    p = Pm.from_rosparam({"object_finder": {"refinement": {"elite": 16, "mix": 1, "shrink": 0.9, "jitter": 0, "enabled": 0}}})
    assert p.refinement == R(enabled=False, elite=16, mix=1.0, shrink=0.9, jitter=0.0)
    assert isinstance(p.refinement.elite, int) and isinstance(p.refinement.mix, float)
    g = p.refinement.c_params()
    assert (g.enabled, g.elite, g.mix, g.shrink, g.jitter) == (0, 16, 1.0, 0.9, 0.0)
    with pytest.raises(ValueError, match="object_finder/refinement/elites"):
        Pm.from_rosparam({"object_finder": {"refinement": {"elites": 5}}})
    with pytest.raises(ValueError):
        Pm.from_rosparam({"object_finder": {"refinements": {}}})
    # the C parameters never carry the Python-side settings: `refinement` is an attribute beside the dataclass's fields
    assert "refinement" not in Pm.__dataclass_fields__ and not hasattr(p.c_params(), "refinement")
    assert [f[0] for f in _capi.RbsFindParams._fields_] == [f for f in Pm.__dataclass_fields__ if f != "foreground"]
    q = Pm.from_rosparam({"object_finder": {"refinement": {"elite": 4}}})
    assert q.refinement == R(elite=4) and Pm().refinement is None              # (set on the instance, not on the class)


def test_exports_defaults_and_checks_without_a_device():
    lib = _capi.load()
    for s in ("rbs_find_default_refinement", "rbs_find_set_refinement", "rbs_find_get_covariance", "rbs_find_get_perturbations"):
        assert s in _capi.EXPORTS and hasattr(lib, s)
    g = _capi.RbsFindRefinement()
    lib.rbs_find_default_refinement(C.byref(g))
    d = ObjectFinder.Refinement()
    assert (g.enabled, g.elite, g.mix, g.shrink, g.jitter) == (1, d.elite, d.mix, d.shrink, d.jitter) == (1, 8, 0.5, 1.0, 1e-10)
    assert (d.elite, d.mix, d.shrink, d.jitter) == tuple(rt.DEFAULTS[k] for k in ("elite", "mix", "shrink", "jitter"))
    assert C.sizeof(_capi.RbsFindRefinement) == 32
    n = C.c_int64()
    bad = _capi.RBS_ERR_INVALID_ARGUMENT
    assert lib.rbs_find_set_refinement(None, C.byref(g)) == bad
    assert lib.rbs_find_get_covariance(None, 0, None, C.byref(n)) == bad and lib.rbs_find_get_perturbations(None, 0, None, C.byref(n)) == bad
    lib.rbs_find_default_refinement(None)                                          # a null pointer is ignored


def test_refinement_kernels_do_not_spill_and_the_probes_stay_in_the_test_build():
    from find_refine_probes import FINDR_SYMBOLS
    txt = open(os.path.join(ROOT, "dbot_ros_amd", "lib", "resource_usage.txt")).read()
    seen = set()
    for b in re.split(r"remark: Function Name: ", txt)[1:]:
        m = re.search(r"rbs_findr_(\w+?)_kernel", b.split()[0])
        if not m:
            continue
        seen.add(m.group(1))
        assert re.search(r"ScratchSize \[bytes/lane\]: 0\b", b) and re.search(r"SGPRs Spill: 0\b", b) and re.search(r"VGPRs Spill: 0\b", b), b
    assert seen == {"init", "children", "update"}, seen
    lib = os.path.join(ROOT, "dbot_ros_amd", "lib")
    release = open(os.path.join(lib, "librbsensor_mi355x.so"), "rb").read()
    test_build = open(os.path.join(lib, "librbsensor_mi355x_hooks.so"), "rb").read()
    assert b"rbs_test_" not in release
    for s in FINDR_SYMBOLS:
        assert s.encode() + b"\0" in test_build, s


# ---------------------------------------------------------------- the six scenes through the twin chain
# The whole find in numpy (tests/find_fg_twin.py, tests/find_twin.py, tests/find_refine_twin.py), every score the EAGER oracle's
# -- the device rule on the CPU -- with the default foreground at seed_stride 4, from sigma (25 degrees, 1.5 cm), 12 rounds of 64
# children, elite 8, mix 0.5, shrink 1.  The pose part of the accuracy bar on every scene: translation < 1 cm, IoU >= 0.85.
class _OracleScorer:
    """Scores of poses on one frame: the EAGER oracle's first frame after a reset, every index 0 (what the finder scores),
    `chunk` poses per call (the oracle keeps two occlusion planes per particle slot)."""
    def __init__(self, om, cam, P, image, chunk):
        self.o = ob.Oracle(om, cam, P, max_particles=chunk, mode=ob.EAGER)
        self.chunk, self.threads = chunk, min(sc.usable_threads(), chunk)
        self.o.reset()
        self.o.set_observation(np.asarray(image, dtype=np.float64))
        self.zero = np.zeros(chunk, dtype=np.int32)

    def __call__(self, poses):
        poses = np.asarray(poses, dtype=np.float64).reshape(-1, 12)
        out = [self.o.loglikes_poses(poses[i: i + self.chunk], self.zero[: len(poses[i: i + self.chunk])], update=False, threads=self.threads)
               for i in range(0, len(poses), self.chunk)]
        return np.concatenate(out)


def _twin_find(mesh, seed, p, g, rf):
    cols, rows = 640, 480
    om, cam, P = sc.make_scene((mesh,), cols, rows, max_particles=1)
    truth, rng = scene_truth(cols, rows, 100 + seed)
    full = _OracleScorer(om, cam, P, np.zeros(rows * cols), 64)
    depth = full.o.render_depth(truth)
    frame = synth.make_frame(np.where(np.isfinite(depth), depth, np.inf), rows, cols, rng)
    full.o.set_observation(np.asarray(frame, dtype=np.float64))
    f = tw.coarse_factor(cols, p.coarse_downsampling)
    coarse, cr, cc = tw.subsample(frame, rows, cols, f)
    rec, sf = fg.foreground(coarse, cr, cc, p.min_depth, p.max_depth, P.kinect.model_sigma, P.kinect.sigma_factor, p.seed, g.plane_trials,
                            g.ransac_sigmas, g.mask_sigmas, g.min_inlier_fraction)
    seeds, _ = tw.seeds(sf, p.seed_stride, p.min_depth, p.max_depth, p.max_seeds)
    Kc = tw.coarse_K(cam.camera_matrix, f)
    hyp = tw.hypotheses(seeds, p.n_rotations, Kc, tw.depth_offset(om.vertices[0]))
    low = _OracleScorer(om, CameraData(Kc, cr, cc), P, coarse, 1024)
    hs = low(hyp)
    low.o.close()
    order = tw.select_order(hs)[: p.n_candidates]
    kept = tw.nms(hyp[order], p.nms_translation, p.nms_angle, p.n_survivors)
    surv = hyp[order][kept]
    cur, best, _ = rt.refine(surv, full, p.rounds, p.children, p.seed, p.sigma_angle, p.sigma_translation, rf.elite, rf.mix, rf.shrink, rf.jitter)
    o = tw.select_order(best)
    pose, score = cur[o[0]], best[o[0]]
    s_truth = full(truth[None])[0]
    a, b = np.isfinite(full.o.render_depth(pose)), np.isfinite(depth)
    full.o.close()
    return float(np.linalg.norm(pose[9:] - truth[9:])), float((a & b).sum() / max((a | b).sum(), 1)), float(score), float(s_truth)


@pytest.mark.parametrize("mesh, seed", fg.SCENES)
def test_the_twin_chain_meets_the_pose_bar_on_the_six_scenes(mesh, seed):
    p = ObjectFinder.Parameters(seed_stride=4, rounds=12, sigma_angle=math.radians(25.0), sigma_translation=0.015)
    dt, iou, score, s_truth = _twin_find(mesh, seed, p, ObjectFinder.Foreground(), ObjectFinder.Refinement())
    print(f"TWIN CHAIN {mesh} seed {seed}: |dt| {dt * 1e3:.2f} mm, IoU {iou:.3f}, score {score:.1f} = {score / s_truth:.3f} x the truth's {s_truth:.1f}")
    assert dt < 0.01 and iou >= 0.85, (dt, iou, score, s_truth)
