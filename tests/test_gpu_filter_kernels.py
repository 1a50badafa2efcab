"""The particle filter's kernels (dbot_ros_amd/csrc/rbsensor_tracker.hip) ON THE DEVICE, array by array, along every
launch chain rbs_tracker_submit takes, against the plain reference tests/filter_twin.py.

The test build of the library (librbsensor_mi355x_hooks.so) has rbs_test_filter: it builds the kernels' argument block from
host arrays, launches a caller-chosen order of the frame's steps through the launch helpers rbs_tracker_submit itself uses,
and hands every array back.  Chains (DESIGN.md "The filter's launch chains"):

  A  weights, resample_gather, mean, recentre       n < 8192: single-block kernels; from 8192 on: w1..w4 / m1..m3
  B  filter_tail, gather, recentre                  n < 8192
  C  filter_step                                    n <= 512

Bars.  logw, ll, idx, the transition, every gathered row, flag: exact.  KL decision: the twin's, max_kl at least 1e-6 off
the twin's KL.  cdf: (n + 4) 2^-53, the sequential worst case of a sum of n positive terms each within an ulp or two.
parents: the twin's search over the device's own cdf, as integers.  mean: 4 n 2^-53 sum |w_i p_i| per component.
Rotations as matrices: max(1e-12, 8 2^-53 / sn) where the angle is beyond pi / 2 (sn: the norm of the antisymmetric part,
what limits the axis near pi), 1e-12 below.  Translations and velocities: 4 ulp.  Chains A, B, C: bit-identical.

The probe exists in the hooks build only, and two builds of the library do not share a process: outside a process that has
loaded the hooks build, the first test here re-runs this file once in a child with RBS_LIB_PATH set to it, and every test
reports its own outcome of that run."""
import ctypes as C
import os

import numpy as np
import pytest

import filter_probes as fp
import filter_twin as ft
from dbot_ros_amd import _capi, pose
from filter_probes import (FILTER_STEP, FILTER_TAIL, GATHER, MEAN, PROPAGATE, RECENTRE, RESAMPLE_GATHER, SWAP, WEIGHTS, step)

pytestmark = pytest.mark.gpu

HOOKS = fp.hooks_path(_capi.LIB_PATH)
IN_HOOKS_PROCESS = os.path.abspath(_capi.LIB_PATH) == os.path.abspath(HOOKS)
SIZES = [1, 63, 64, 65, 1023, 1024, 1025, 4097, 8191, 8192, 8193, 12289]
PARTS = [1, 3]
EPS = 2.0 ** -53
MULTI_BLOCK_FROM, FUSED_MAX = 8192, 512     # kMultiBlockFrom, kFusedFilterMax
SEED = 0xC0FFEE1234ABCDEF                     # both halves set
_child = {}
worst = {}                                     # the largest differences seen, printed by the last test


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
    return fp.FilterProbe(HOOKS) if IN_HOOKS_PROCESS else None


def _note(key, value):
    worst[key] = max(worst.get(key, 0.0), float(value))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _untouched(a):
    return bool(np.all(a == (fp.ISENTINEL if a.dtype == np.int32 else fp.SENTINEL)))


def _ulps(got, ref):
    return float((np.abs(got - ref) / np.spacing(np.maximum(np.abs(ref), np.finfo(np.float64).tiny))).max())


def _rotation_bar(R):
    """Per matrix [...,3,3]: how far two evaluations of the rotation-vector round trip may differ, as matrices."""
    s = 0.5 * np.stack([R[..., 2, 1] - R[..., 1, 2], R[..., 0, 2] - R[..., 2, 0], R[..., 1, 0] - R[..., 0, 1]], -1)
    sn = np.linalg.norm(s, axis=-1)
    cs = 0.5 * (np.trace(R, axis1=-2, axis2=-1) - 1.0)
    with np.errstate(divide="ignore"):
        return np.where(cs > 0.0, 1e-12, np.maximum(1e-12, 8.0 * EPS / sn))


# ---------------------------------------------------------------- weight profiles
def _boundaries(n):
    """Index 0, n - 1, and both sides of every thread, wave and chunk boundary n has: the single-block kernels give a thread
    ceil(n / 1024) consecutive particles and a wave 64 threads; the grid kernels give a thread 4 and a block 4096."""
    per = (n + 1023) // 1024
    cuts = {0, n - 1}
    for edge in (per, 64 * per, 4, 256, 1024, 4096, 8192, 12288):
        cuts.update((edge - 1, edge))
    return sorted(k for k in cuts if 0 <= k < n)


def _profiled(st, profile, dominant=0):
    """ll_new (and for the Gaussian spread a log-weight carried in) of the state's profile; max_kl is set by the caller."""
    n = st["n"]
    rng = np.random.default_rng([n, st["parts"], 99])
    st = dict(st)
    if profile == "flat":
        pass
    elif profile in ("gauss", "tenth"):
        st["logw"] = rng.normal(0.0, 0.1, n)
        st["ll_new"] = st["ll"] + 3.0 * rng.standard_normal(n)
        if profile == "tenth" and n >= 10:
            st["ll_new"][rng.permutation(n)[:n // 10]] = -np.inf
    elif profile == "dominant":
        st["ll_new"] = st["ll"] - 800.0
        st["ll_new"][dominant] = st["ll"][dominant]
    return st


def _planted_uniforms(cdf, u):
    """Random uniforms with the edges planted: u == cdf[k] for a dozen k, 0, the last double below 1, and one above cdf[n-1]."""
    n = cdf.size
    u = u.copy()
    ks = np.unique(np.linspace(0, n - 1, 12).astype(int))
    plant = np.concatenate([cdf[ks], [0.0, np.nextafter(1.0, 0.0), np.nextafter(cdf[n - 1], 2.0)]])
    m = min(n, plant.size)
    u[:m] = plant[:m]
    return u, ks[:m]


# ---------------------------------------------------------------- one chain against the twin
def _chain_a(b, updated):
    return [step(WEIGHTS, updated=updated), step(RESAMPLE_GATHER, b=b), step(SWAP), step(MEAN), step(RECENTRE)]


def _chain_b(b, updated):
    return [step(FILTER_TAIL, b=b, updated=updated), step(GATHER), step(SWAP), step(RECENTRE)]


def _chain_c(b, updated):
    return [step(FILTER_STEP, b=b, updated=updated, last=1), step(SWAP)]


def _check_against_twin(st, out, b, updated, expect_resample, tag):
    n, parts = st["n"], st["parts"]
    D = parts * ft.BODY
    logw1, ll1 = ft.weight_update(st["logw"], st["ll"], st["ll_new"])
    idx1 = np.arange(n, dtype=np.int32) if updated else st["idx"]
    w, kl, cdf = ft.weights_kl_cdf(logw1)
    assert abs(float(kl) - st["max_kl"]) >= 1e-6 and bool(kl > st["max_kl"]) == expect_resample, (tag, float(kl), st["max_kl"])
    assert out["flag"].tolist() == [int(expect_resample), 5 + int(expect_resample)], (tag, out["flag"], float(kl))
    bar = (n + 4) * EPS
    if expect_resample:
        d = float(np.abs(out["cdf"].astype(np.longdouble) - cdf).max())
        _note("cdf / its bar", d / bar)
        assert d <= bar and np.all(np.diff(out["cdf"]) >= 0.0) and abs(out["cdf"][n - 1] - 1.0) <= bar, (tag, d, bar, out["cdf"][n - 1])
        par = ft.parents_of(out["cdf"], st["uniforms"][b])
        assert np.array_equal(out["parents"], par), (tag, np.flatnonzero(out["parents"] != par)[:8])
    else:
        par = np.arange(n, dtype=np.int32)
        assert np.array_equal(out["parents"], par), tag
        assert n >= MULTI_BLOCK_FROM or _untouched(out["cdf"]), tag
    # the weight step and the gather: exact
    assert _same(out["logw"], np.zeros(n) if expect_resample else logw1), tag
    assert _same(out["ll"], ll1[par]) and _same(out["idx"], idx1[par]), tag
    assert _same(out["part_old"], st["part_old"][par]) and _same(out["noise"], st["noise"][par]), tag
    # ... whose sources are the gather targets after the exchange: as they were (ll and idx after the weight step)
    assert _same(out["part_old2"], st["part_old"]) and _same(out["part_new2"], st["part_new"]) and _same(out["noise2"], st["noise"]), tag
    assert _same(out["ll2"], ll1) and _same(out["idx2"], idx1), tag
    assert _untouched(out["poses"]) and _same(out["ll_new"], st["ll_new"]), tag
    # the mean of the (resampled) particles
    moved = st["part_new"][par]
    w2 = np.full(n, 1.0 / np.longdouble(n)) if expect_resample else w
    mean = ft.weighted_mean(w2, moved)
    mbar = 4 * n * EPS * ft.mean_magnitude(w2, moved)
    dm = np.abs(out["mean"][:D] - mean)
    _note("mean / its bar", (dm / np.maximum(mbar, 1e-300)).max())
    assert np.all(dm <= mbar), (tag, dm.max(), mbar.min())
    # the default pose, from the device's own mean
    mu = out["mean"][:D]
    z, Rz = ft.fold_mean(st["deflt"], mu, parts)
    zd, zt = out["deflt"].reshape(parts, ft.BODY), z.reshape(parts, ft.BODY)
    dR = np.abs(pose.rotvec_to_matrix(zd[:, 3:6]) - Rz).max(axis=(-1, -2))
    _note("default rotation / its bar", (dR / _rotation_bar(Rz)).max())
    assert np.all(dR <= _rotation_bar(Rz)), (tag, dR)
    assert _ulps(zd[:, 0:3], zt[:, 0:3]) <= 4 and _ulps(zd[:, 6:12], zt[:, 6:12]) <= 4, tag
    RmT = np.swapaxes(pose.rotvec_to_matrix(mu.reshape(parts, ft.BODY)[:, 3:6]), -1, -2)
    assert np.abs(out["mean"][D:].reshape(parts, 3, 3) - RmT).max() <= 1e-12, tag
    # the re-centred particles
    got, ref = out["part_new"].reshape(n, parts, ft.BODY), moved.reshape(n, parts, ft.BODY)
    Rp = ft.recentred_rotations(moved, mu, parts)
    dP = np.abs(pose.rotvec_to_matrix(got[..., 3:6]) - Rp).max(axis=(-1, -2))
    _note("re-centred rotation / its bar", (dP / _rotation_bar(Rp)).max())
    assert np.all(dP <= _rotation_bar(Rp)), (tag, dP.max())
    assert _ulps(got[..., 0:3], ref[..., 0:3] - mu.reshape(parts, ft.BODY)[None, :, 0:3]) <= 4, tag
    assert _same(got[..., 6:12].copy(), ref[..., 6:12].copy()), tag
    # publish_result: the estimate, the two flags, the frame's number behind them
    assert _same(out["host_state"], out["deflt"]), tag
    assert out["host_flags"].tolist() == out["flag"].tolist() + [int((st["frame"] + 1) & 0xFFFFFFFF)], tag


def _check_chains_agree(probe, st, ref_out, b, updated, tag):
    """Below 8192 particles the chains promise the same operations in the same order: the same bits in every array."""
    n = st["n"]
    chains = [("B", _chain_b(b, updated))] if n < MULTI_BLOCK_FROM else []
    if n <= FUSED_MAX:
        chains.append(("C", _chain_c(b, updated)))
    for name, steps in chains:
        out = probe.run(st, steps)
        differ = [k for k in fp.ARRAYS if not _same(out[k], ref_out[k])]
        assert not differ, (tag, "chain " + name, differ,
                            [float(np.abs(out[k].astype(np.float64) - ref_out[k]).max()) for k in differ])


# ---------------------------------------------------------------- the entry point itself
def test_filter_probe_refuses_bad_arguments(request, probe):
    if _delegated(request):
        return
    assert all(hasattr(probe.lib, s) for s in fp.FILTER_SYMBOLS)
    st = fp.make_state(5, 2, SEED)
    good = [step(WEIGHTS)]
    io, arr, out = probe.pack(st, good)
    assert probe.raw(None, arr, 1) == fp.RBS_ERR_INVALID_ARGUMENT and probe.raw(C.byref(io), None, 1) == fp.RBS_ERR_INVALID_ARGUMENT
    assert probe.raw(C.byref(io), arr, -1) == fp.RBS_ERR_INVALID_ARGUMENT
    for field, bad in (("n", 0), ("n", -3), ("parts", 0), ("parts", -1), ("part_new", None), ("cdf", None), ("flag", None),
                       ("host_state", None), ("host_flags", None), ("ll_new", None)):
        io, arr, out = probe.pack(st, good)
        setattr(io, field, bad)
        assert probe.raw(C.byref(io), arr, 1) == fp.RBS_ERR_INVALID_ARGUMENT, field
    for bad in (step(9), step(-1), step(RESAMPLE_GATHER, b=2), step(PROPAGATE, b=-1)):
        io, arr, out = probe.pack(st, [bad])
        assert probe.raw(C.byref(io), arr, 1) == fp.RBS_ERR_INVALID_ARGUMENT, bad
        assert all(_same(out[k], np.asarray(st[k], dtype=out[k].dtype)) for k in fp.ARRAYS)      # nothing was written
    io, arr, out = probe.pack(st, [])
    assert probe.raw(C.byref(io), arr, 0) == fp.RBS_OK                                           # no step: every array comes back as it went
    assert all(_same(out[k], np.asarray(st[k], dtype=out[k].dtype)) for k in fp.ARRAYS)


# ---------------------------------------------------------------- the filter step, every size, every profile
@pytest.mark.parametrize("parts", PARTS)
@pytest.mark.parametrize("n", SIZES)
def test_filter_step_matches_the_twin_on_every_chain(request, probe, n, parts):
    """Flat (no resampling), a Gaussian spread of 3 nats on either side of max_kl, a tenth of the particles at -inf:
    chain A against the twin, chains B and C against chain A bit for bit; random uniforms, then the planted ones."""
    if _delegated(request):
        return
    base = fp.make_state(n, parts, SEED, frame=41)
    outcomes = set()
    for profile, side, updated, b in (("flat", None, 0, 0), ("gauss", -1, 1, parts - 1), ("gauss", +1, 0, parts - 1), ("tenth", -1, 1, 0)):
        st = _profiled(base, profile)
        kl = float(ft.weights_kl_cdf(ft.weight_update(st["logw"], st["ll"], st["ll_new"])[0])[1])
        st["max_kl"] = 2.0 if side is None else kl + side * 2e-6        # (flat: KL = 0)
        expect = kl > st["max_kl"]
        outcomes.add(expect)
        tag = (n, parts, profile, side)
        out = probe.run(st, _chain_a(b, updated))
        _check_against_twin(st, out, b, updated, expect, tag)
        _check_chains_agree(probe, st, out, b, updated, tag)
        if expect:
            st2 = dict(st)
            u, ks = _planted_uniforms(out["cdf"], st["uniforms"][b])
            st2["uniforms"] = st["uniforms"].copy()
            st2["uniforms"][b] = u
            out2 = probe.run(st2, _chain_a(b, updated))
            assert _same(out2["cdf"], out["cdf"]), tag
            _check_against_twin(st2, out2, b, updated, expect, tag + ("planted",))
            _check_chains_agree(probe, st2, out2, b, updated, tag + ("planted",))
            cdf, par = out2["cdf"], out2["parents"]
            for j, k in enumerate(ks):      # u == cdf[k]: the next particle, where the cdf steps up there
                if k + 1 < n and cdf[k + 1] > cdf[k]:
                    assert par[j] == k + 1, (tag, j, k, par[j])
            if n >= 15:
                assert par[14] == n - 1, (tag, par[12:15])                           # above cdf[n-1]: the last particle, not one past it
                assert cdf[par[12]] > 0.0 and (par[12] == 0 or cdf[par[12] - 1] == 0.0), tag   # u = 0: the first particle with weight
    assert outcomes == {True, False}, (n, outcomes)


@pytest.mark.parametrize("parts", PARTS)
@pytest.mark.parametrize("n", SIZES)
def test_one_dominant_particle_on_every_boundary(request, probe, n, parts):
    """Every other weight 800 nats lower -- they underflow to zero -- with the dominant one at index 0, at n - 1 and on both
    sides of each thread, wave and chunk boundary n has: the cdf is one step, every child descends from that particle."""
    if _delegated(request):
        return
    base = fp.make_state(n, parts, SEED, frame=2)
    for k in _boundaries(n):
        st = _profiled(base, "dominant", k)
        st["max_kl"] = float(np.log(n)) - 2e-6      # KL = log n
        tag = (n, parts, "dominant", k)
        out = probe.run(st, _chain_a(parts - 1, 1))
        step_cdf = (np.arange(n) >= k).astype(np.float64)
        assert np.array_equal(out["cdf"], step_cdf) and np.all(out["parents"] == k), (tag, np.flatnonzero(out["cdf"] != step_cdf)[:8])
        _check_against_twin(st, out, parts - 1, 1, True, tag)
        _check_chains_agree(probe, st, out, parts - 1, 1, tag)


# ---------------------------------------------------------------- the transition, and the deferred re-centring
@pytest.mark.parametrize("parts", PARTS)
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1025, 8193])
def test_transition_has_the_twin_bits(request, probe, n, parts):
    """propagate_kernel (256 threads a block) with host normals: the new particle and the stored noise bit for bit, the
    absolute poses R(delta) R(default) | t(delta) + t(default) to 64 roundings of entries below 1."""
    if _delegated(request):
        return
    st = fp.make_state(n, parts, SEED)
    for b in sorted({0, parts - 1}):
        out = probe.run(st, [step(PROPAGATE, b=b)])
        new, noise = ft.transition(st["part_old"], st["noise"], st["normals"][b], b, st["sigma"], st["vf"])
        assert _same(out["part_new"], new) and _same(out["noise"], noise) and _same(out["part_old"], st["part_old"]), (n, parts, b)
        ref = pose.compose_with_default(new, st["deflt"], parts)
        d = np.abs(out["poses"] - ref)
        _note("poses, in 2^-53", d[..., :9].max() / EPS)
        assert d[..., :9].max() <= 64 * EPS and _ulps(out["poses"][..., 9:], ref[..., 9:]) <= 4, (n, parts, b, d.max())


@pytest.mark.parametrize("n", [65, 1025])
def test_deferred_recentring_has_the_bits_of_the_separate_launch(request, probe, n):
    """The re-centring that rides in the next frame's first transition launch against recentre_kernel, from the same mean."""
    if _delegated(request):
        return
    parts = 3
    st = _profiled(fp.make_state(n, parts, SEED), "gauss")
    st["max_kl"] = 0.5
    chain = [step(WEIGHTS, updated=1), step(RESAMPLE_GATHER, b=1), step(SWAP), step(MEAN)]
    now = probe.run(st, chain + [step(RECENTRE)])
    later = probe.run(st, chain)
    nxt = dict(st, part_old=later["part_new"], mean=later["mean"], deflt=later["deflt"])
    out = probe.run(nxt, [step(PROPAGATE, b=0, recentre=1)])
    assert _same(out["part_old"], now["part_new"])


# ---------------------------------------------------------------- the mean rotation near pi
def test_default_pose_update_near_pi(request, probe):
    """Default poses whose composition with the mean rotation has the angle pi - {0, 1e-9, 1e-7, 1e-3}, and a zero rotation:
    the second branch of matrix_to_rotvec (the axis from the symmetric part) and the ill-conditioned end of the first."""
    if _delegated(request):
        return
    n, parts = 65, 3
    rng = np.random.default_rng(5)
    for deltas in ((0.0, 1e-9, 1e-7), (1e-3, None, 1e-9)):
        st = fp.make_state(n, parts, SEED, max_kl=1e9)
        p = st["part_new"].reshape(n, parts, ft.BODY)
        z = st["deflt"].reshape(parts, ft.BODY)
        for b, delta in enumerate(deltas):
            axis = rng.standard_normal(3)
            axis /= np.linalg.norm(axis)
            if delta is None:                       # zero mean rotation on a zero default rotation
                p[:, b, 3:6], z[b, 3:6] = 0.0, 0.0
            else:                                   # every particle the same rotation 0.3 about the axis, the default the rest to pi - delta
                p[:, b, 3:6], z[b, 3:6] = 0.3 * axis, (np.pi - delta - 0.3) * axis
        out = probe.run(st, _chain_a(0, 0))
        _check_against_twin(st, out, 0, 0, False, ("near pi", deltas))
        _check_chains_agree(probe, st, out, 0, 0, ("near pi", deltas))
        zd = out["deflt"].reshape(parts, ft.BODY)
        for b, delta in enumerate(deltas):
            ang = np.linalg.norm(zd[b, 3:6])
            print(f"near pi: delta {delta}: angle of the new default rotation pi - {np.pi - ang:.3e}")
            assert np.isfinite(ang) and abs(ang - (0.0 if delta is None else np.pi - delta)) <= 1e-12 + 8 * EPS


# ---------------------------------------------------------------- the device generator
@pytest.mark.parametrize("b", [0, 2])
@pytest.mark.parametrize("frame", [0, 1, 2 ** 24 + 3])
def test_device_generator_draws_the_twin_streams(request, probe, frame, b):
    """normals and uniforms null: Box-Muller on Philox4x32-10 with the counter (frame << 8 | b, i << 2 | pair) -- at
    frame 2^24 + 3 the shift reaches the fourth counter word -- and the resampling uniforms under the key seed ^ 0x5bd1e995."""
    if _delegated(request):
        return
    n, parts = 1025, 3
    st = _profiled(fp.make_state(n, parts, SEED, frame=frame), "gauss")
    st["max_kl"] = 0.5
    st["normals"] = st["uniforms"] = None
    out = probe.run(st, [step(PROPAGATE, b=b), step(WEIGHTS), step(RESAMPLE_GATHER, b=b), step(SWAP)])
    assert out["flag"][0] == 1
    nz = ft.device_normals(SEED, frame, b, n)
    d = np.abs(out["noise2"][:, b] - nz).max()          # (after the exchange noise2 is the array the transition wrote)
    _note("device normals", d)
    assert d <= 1e-13, (frame, b, d)
    keep = [bb for bb in range(parts) if bb != b]
    assert _same(out["noise2"][:, keep].copy(), st["noise"][:, keep].copy())
    new, _ = ft.transition(st["part_old"], st["noise"], out["noise2"][:, b], b, st["sigma"], st["vf"])
    assert _same(out["part_new2"], new)
    par = ft.parents_of(out["cdf"], ft.device_uniforms(SEED, frame, b, n))
    assert np.array_equal(out["parents"], par), np.flatnonzero(out["parents"] != par)[:8]
    assert _same(out["part_new"], new[par])


def test_report_the_largest_differences(request, probe):
    if _delegated(request):
        return
    for k, v in sorted(worst.items()):
        print(f"largest difference, {k}: {v:.3e}")
