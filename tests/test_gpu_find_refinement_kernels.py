"""The kernels of the object finder's step 6b, the adaptive refinement (rbs_findr_*_kernel, dbot_ros_amd/csrc/rbsensor_find.hip)
ON THE DEVICE, one by one, on planted inputs, against the numpy twin tests/find_refine_twin.py.

The test build of the library (librbsensor_mi355x_hooks.so) has rbs_test_findr_children (rbf::launch_refine_init, when no
factors are given, and rbf::launch_refine_children) and rbs_test_findr_update (rbf::launch_refine_update): the helpers
rbs_find_run itself calls; host arrays in and out, every output with a sentinel-filled tail (tests/find_refine_probes.py).

Bars.  The update kernel -- the elite, the covariance and its factor -- is binary64 with + - * / and sqrt only and the library is
built without contraction: EXACT, compared as bits.  The children kernel draws step 6's normals (log, cos, sin): child 0 and
whatever follows from the normals by + and * alone are exact; d and the poses are within 1e-14 absolute of the twin evaluated in
extended precision, the bar of the existing children kernel.

The probes exist in the hooks build only, and two builds of the library do not share a process: outside a process that has
loaded the hooks build, the first test here re-runs this file once in a child with RBS_LIB_PATH set to it, and every test
reports its own outcome of that run."""
import os

import numpy as np
import pytest

import find_refine_probes as fp
import find_refine_twin as rt
import find_twin as tw
from dbot_ros_amd import _capi
from find_refine_probes import TAIL, untouched

pytestmark = pytest.mark.gpu

HOOKS = fp.hooks_path(_capi.LIB_PATH)
IN_HOOKS_PROCESS = os.path.abspath(_capi.LIB_PATH) == os.path.abspath(HOOKS)
_child = {}
BIG_SEED = 0xC0FFEE1234ABCDEF
CHILD_BAR = 1e-14


def _delegated(request):
    """True: this process has not loaded the hooks build -- the test's outcome is the one of the child run."""
    if IN_HOOKS_PROCESS:
        return False
    if not _child:
        assert os.path.exists(HOOKS), "build() makes librbsensor_mi355x_hooks.so"
        _child["outcome"], _child["out"] = fp.child_outcomes(__file__, HOOKS, 900)
    assert _child["outcome"].get(request.node.name) == "PASSED", _child["out"]
    return True


@pytest.fixture(scope="module")
def probe(gpu_lib):
    return fp.RefinementProbe(HOOKS) if IN_HOOKS_PROCESS else None


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b):
    """The same bits; a NaN matches a NaN (its payload is no part of the definition)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))))


def _spd(S, rng, scale=1e-3):
    A = rng.normal(size=(S, 6, 6))
    return scale * (A @ A.transpose(0, 2, 1) + 6.0 * np.eye(6))


def _random_poses(n, rng):
    R = tw.quat_xyzw_to_matrix(tw.sf_quaternions(4096, rng.integers(0, 4096, n)))
    return np.concatenate([R, rng.uniform(-0.5, 0.5, (n, 3)) + [0.0, 0.0, 1.0]], axis=1)


# ---------------------------------------------------------------- the update kernel: exact
PROFILES = ("random", "ties", "nan first", "all nan", "infinities", "few numbers")


def _scores(profile, S, nc, rng):
    s = rng.normal(size=(S, nc))
    if profile == "ties":                           # three values: ties inside a lane's children (j, j + 64, ...) and across lanes
        s = rng.integers(0, 3, size=(S, nc)).astype(np.float64)
        s[:, ::2] *= -0.0 if nc > 2 else 1.0        # (... and -0.0 beside +0.0: equal, j decides)
    elif profile == "nan first":
        s[:, 0] = np.nan
        s[:, rng.integers(0, nc, max(1, nc // 3))] = np.nan
    elif profile == "all nan":
        s[:] = np.nan
        s[S // 2] = rng.normal(size=nc)             # (one survivor keeps its numbers)
    elif profile == "infinities":
        s[:, rng.integers(0, nc, max(1, nc // 4))] = np.inf
        s[:, rng.integers(0, nc, max(1, nc // 4))] = -np.inf
        s[:, rng.integers(0, nc, max(1, nc // 8))] = np.nan
    elif profile == "few numbers":                  # fewer numbers than the elite
        keep = rng.integers(0, nc, 3)
        t = np.full((S, nc), np.nan)
        t[:, keep] = s[:, keep]
        s = t
    return s


def _check_update(probe, s, d, cov, elite, mix, shrink, jitter, tag):
    S = len(s)
    got_c, got_l = probe.update(s, d, cov, elite, mix, shrink, jitter)
    want_c, want_l = rt.update_all(cov, s, d, elite, mix, shrink, jitter)
    assert untouched(got_c[S:]) and untouched(got_l[S:]), tag
    assert _same(got_c[:S], want_c.reshape(S, 36)), tag
    assert _same(got_l[:S], want_l.reshape(S, 36)), tag
    return want_c, want_l


@pytest.mark.parametrize("S", [1, 7, 64])
def test_update_is_the_twin_bit_for_bit(request, probe, S):
    if _delegated(request):
        return
    rng = np.random.default_rng([S, 6])
    for nc in (1, 2, 63, 64, 65, 4096):
        d = rng.normal(size=(S, nc, 6)) * [0.3, 0.3, 0.3, 0.01, 0.01, 0.01]
        d[:, 0] = 0.0
        cov = _spd(S, rng)
        for elite in sorted({min(e, nc, 64) for e in (1, 8, 64, nc)}):
            for profile in PROFILES if nc <= 65 or S == 7 else ("random", "ties"):
                s = _scores(profile, S, nc, rng)
                _check_update(probe, s, d, cov, elite, 0.5, 1.0, 1e-10, (S, nc, elite, profile))
        s = _scores("random", S, nc, rng)
        e = min(8, nc)
        for mix, shrink, jitter in ((0.0, 1.0, 0.0), (1.0, 1.0, 0.0), (1.0, 0.75, 1e-10), (0.25, 0.5, 1e-6)):
            want_c, _ = _check_update(probe, s, d, cov, e, mix, shrink, jitter, (S, nc, mix, shrink, jitter))
            if mix == 0.0:
                assert _same(want_c, cov)                                       # mix 0, shrink 1, jitter 0: C stays


def test_update_ties_within_and_across_lanes(request, probe):
    """Equal scores at j, j + 64, j + 128 (one lane) and at neighbouring j (other lanes): the elite takes them by ascending j."""
    if _delegated(request):
        return
    rng = np.random.default_rng(12)
    S, nc = 3, 200
    d = rng.normal(size=(S, nc, 6))
    s = np.full((S, nc), -1.0)
    s[0, [5, 69, 133, 197, 6, 70]] = 2.0
    s[1, :] = 2.0
    s[2, [199, 64, 0, 128]] = [2.0, 2.0, 1.0, 1.0]
    assert rt.elite_order(s[0], 5).tolist() == [5, 6, 69, 70, 133] and rt.elite_order(s[1], 4).tolist() == [0, 1, 2, 3]
    assert rt.elite_order(s[2], 4).tolist() == [64, 199, 0, 128]
    for elite in (1, 4, 5, 6, 64):
        _check_update(probe, s, d, _spd(S, rng), elite, 1.0, 1.0, 0.0, elite)


def test_update_when_no_child_has_a_number_leaves_c_alone(request, probe):
    if _delegated(request):
        return
    rng = np.random.default_rng(3)
    S, nc = 7, 65
    cov = _spd(S, rng)
    got_c, got_l = probe.update(np.full((S, nc), np.nan), rng.normal(size=(S, nc, 6)), cov, 8, 0.5, 0.5, 1e-3)
    assert _same(got_c[:S], cov.reshape(S, 36)) and untouched(got_c[S:])            # neither shrink nor jitter
    assert _same(got_l[:S], np.stack([rt.factor(c, 1e-3) for c in cov]).reshape(S, 36))


def test_factor_fallbacks(request, probe):
    """C = 0; a C whose third pivot is exactly 0; one whose third pivot is negative; NaN and inf on the diagonal: the factor after
    an update that leaves C as it is (mix 0, shrink 1, jitter 0 in the update; the jitter only in the fallback's max)."""
    if _delegated(request):
        return
    rng = np.random.default_rng(9)
    L = np.tril(rng.integers(1, 4, size=(6, 6)).astype(np.float64))
    L[2, 2] = 0.0
    flat = L @ L.T                                                                  # small integers: exact, the third pivot 0
    neg = flat.copy()
    neg[2, 2] -= 1.0
    good = np.tril(rng.integers(1, 4, size=(6, 6)).astype(np.float64))
    good = good @ good.T                                                            # every pivot a positive integer
    cov = np.stack([np.zeros((6, 6)), flat, neg, good, np.diag([1.0, -2.0, np.nan, np.inf, 0.0, 4.0]), 1e-300 * good])
    S, nc = len(cov), 4
    s, d = rng.normal(size=(S, nc)), rng.normal(size=(S, nc, 6))
    for jitter in (0.0, 1e-10, 0.25):
        got_c, got_l = probe.update(s, d, cov, 2, 0.0, 1.0, 0.0)
        assert _same(got_c[:S], cov.reshape(S, 36))
        # (the probe's jitter is the update's too, so the fallback's jitter is exercised with mix 0 and a C that takes it)
        got_c, got_l = probe.update(np.full((S, nc), np.nan), d, cov, 2, 0.0, 1.0, jitter)
        want = np.stack([rt.factor(c, jitter) for c in cov])
        assert _same(got_c[:S], cov.reshape(S, 36)) and _same(got_l[:S], want.reshape(S, 36)), jitter
        assert np.array_equal(want[0], np.sqrt(jitter) * np.eye(6))
        for k in (1, 2, 4):
            assert np.array_equal(want[k], np.diag(np.diag(want[k])))               # the fallback: a diagonal
        assert want[3][1, 0] != 0.0 and np.array_equal(want[3] @ want[3].T, good)   # ... and a proper factor where C has one


# ---------------------------------------------------------------- the children kernel
CHILD_SHAPES = [(1, 1), (1, 2), (7, 65), (64, 64), (2, 4096)]


def _sample_pairs(S, n_children, rng, m=10):
    edge = [(k, j) for k in {0, S - 1} for j in {0, 1, n_children - 1} if j < n_children]
    rand = [(int(rng.integers(S)), int(rng.integers(n_children))) for _ in range(m)]
    return sorted(set(edge + rand))


@pytest.mark.parametrize("rnd", [0, 1, 63])
@pytest.mark.parametrize("seed", [0, BIG_SEED, 2 ** 64 - 1], ids=["seed0", "seedmixed", "seedones"])
def test_children_through_the_factor(request, probe, seed, rnd):
    if _delegated(request):
        return
    rng = np.random.default_rng([rnd, seed & 0xFFFF])
    worst = 0.0
    for S, nc in CHILD_SHAPES:
        tag = (S, nc, rnd, hex(seed))
        m = S * nc
        surv = _random_poses(S, rng)
        eye = np.repeat(np.eye(6)[None], S, 0)
        # L = 1: d is the normals themselves (0 n_b + ... + 1 n_a), child 0 the survivor with d = 0
        out, dd, _ = probe.children(surv, nc, rnd, seed, factors=eye)
        nz = dd[:m].reshape(S, nc, 6).copy()
        assert untouched(out[m:]) and untouched(dd[m:]), tag
        assert _same(out[:m].reshape(S, nc, 12)[:, 0], surv) and _same(nz[:, 0], np.zeros((S, 6))), tag
        ref = tw.child_normals_array(seed, rnd, S, nc)
        if nc > 1:
            assert np.abs(nz[:, 1:] - ref[:, 1:]).max() <= CHILD_BAR, tag
        # a diagonal factor: d_a = L_aa n_a exactly
        diag = rng.uniform(0.001, 0.5, (S, 6))
        out, dd, _ = probe.children(surv, nc, rnd, seed, factors=np.stack([np.diag(v) for v in diag]))
        assert _same(dd[:m].reshape(S, nc, 6), nz * diag[:, None, :]), tag
        # the factors the device makes of the initial covariance are the twin's, and give the same children as handing them in
        sa, st = 0.4363323129985824, 0.015
        out0, dd0, cov0 = probe.children(surv, nc, rnd, seed, sigma_angle=sa, sigma_translation=st, jitter=1e-10)
        C0 = rt.initial_covariance(sa, st)
        assert _same(cov0[:S], np.repeat(C0.reshape(1, 36), S, 0)) and untouched(cov0[S:]), tag
        out1, dd1, _ = probe.children(surv, nc, rnd, seed, factors=np.repeat(rt.factor(C0, 1e-10)[None], S, 0))
        assert _same(out0, out1) and _same(dd0, dd1), tag
        # the general case: full lower factors
        fac = np.stack([rt.factor(c, 0.0) for c in _spd(S, rng, 1e-3)])
        fac[:, 3:] *= 0.05                                                          # (translations: centimetres)
        out, dd, _ = probe.children(surv, nc, rnd, seed, factors=fac)
        got, gd = out[:m].reshape(S, nc, 12), dd[:m].reshape(S, nc, 6)
        assert untouched(out[m:]) and untouched(dd[m:]) and _same(got[:, 0], surv) and _same(gd[:, 0], np.zeros((S, 6))), tag
        if nc > 1:
            want_d = np.stack([rt.perturb(fac[k], nz[k]) for k in range(S)])        # from the device's own normals: exact
            assert _same(gd[:, 1:], want_d[:, 1:]), tag
        rp, rd = rt.children(surv, fac, nc, rnd, seed)
        assert np.abs(gd - rd).max() <= CHILD_BAR and np.abs(got - rp).max() <= CHILD_BAR, tag
        pairs = _sample_pairs(S, nc, rng)
        ep, ed = rt.children_ext(surv, fac, nc, rnd, seed, pairs)
        dp = float(np.abs(np.stack([got[k, j] for k, j in pairs]) - ep).max())
        d6 = float(np.abs(np.stack([gd[k, j] for k, j in pairs]) - ed).max())
        worst = max(worst, dp, d6)
        assert dp <= CHILD_BAR and d6 <= CHILD_BAR, (tag, dp, d6)
    print(f"children, device - extended twin: {worst:.3e} (bar {CHILD_BAR:g})")


def test_refinement_probes_refuse_bad_arguments(request, probe):
    if _delegated(request):
        return
    import ctypes as C
    lib = probe.lib
    i32, i64, f64, u64 = C.c_int32, C.c_int64, C.c_double, C.c_uint64
    a = fp.sentinel(4096, np.float64)
    p = fp._p(a)
    bad = fp.RBS_ERR_INVALID_ARGUMENT
    upd = lib.rbs_test_findr_update
    assert upd(None, p, i32(1), i32(4), i32(2), f64(0.5), f64(1.0), f64(0.0), p, p, i64(0)) == bad
    for S, nc, elite in ((-1, 4, 2), (65, 4, 2), (1, 0, 1), (1, 4097, 1), (1, 4, 0), (1, 4, 5), (1, 100, 65)):
        assert upd(p, p, i32(S), i32(nc), i32(elite), f64(0.5), f64(1.0), f64(0.0), p, p, i64(0)) == bad, (S, nc, elite)
    assert upd(p, p, i32(1), i32(4), i32(2), f64(0.5), f64(1.0), f64(0.0), p, p, i64(-1)) == bad
    assert upd(p, p, i32(0), i32(4), i32(2), f64(0.5), f64(1.0), f64(0.0), p, p, i64(0)) == fp.RBS_OK
    ch = lib.rbs_test_findr_children
    assert ch(p, None, i32(1), i32(4), i32(0), u64(0), f64(0.1), f64(0.1), f64(0.0), None, p, p, i64(0)) == bad     # neither factors nor cov
    for S, nc, rnd in ((-1, 4, 0), (65, 4, 0), (1, 0, 0), (1, 4097, 0), (1, 4, -1), (1, 4, 64)):
        assert ch(p, p, i32(S), i32(nc), i32(rnd), u64(0), f64(0.1), f64(0.1), f64(0.0), p, p, p, i64(0)) == bad, (S, nc, rnd)
    assert ch(p, p, i32(0), i32(4), i32(0), u64(0), f64(0.1), f64(0.1), f64(0.0), p, p, p, i64(0)) == fp.RBS_OK
    assert untouched(a)
