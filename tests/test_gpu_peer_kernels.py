"""The four kernels behind rbs_peer_resample (dbot_ros_amd/csrc/rbsensor_peers.hip: resampling across processes) ON THE DEVICE,
against the plain reference tests/peer_twin.py, on the planted inputs of tests/peer_cases.py (held to their own conditions,
without a device, by tests/test_peer_twin_cpu.py).

Every call goes through RbSensor.peer_resample on a sensor of max_particles = 2 n; the test build's rbs_test_peer_scratch then hands
back what the call left in the handle's scratch block: the cumulative weights inside each tile of 2048 particles, the tiles' maxima
(above 16 tiles) and totals, the rank's parents.  Layers:

  exact      weights exactly 1 or 0, uniforms on, just below and just above j / W, 0 and 1 - 2^-53: parents by counting, the scratch
             arrays as exact integers and the exact maximum; no tolerance
  maximum    one particle, the others 800 T below, at the array's and a tile's first and last index, both routes of the maximum
  cdf        seven weight profiles against the exact cumulative weights in np.longdouble and the first-order bar E of peer_twin
             (D = 64 additions); parents inside the band E leaves open, at most 1 child in 10 000 with a band of more than one parent
  tail       64 jobs whose last 1 to 5 particles are NaN and whose last uniform is 1 - 2^-53: no child inherits from a particle
             that weighs nothing
  plan       planted parents (equal weights, u = (p + 0.5) / N): parent_idx, stage_src, stage_dst, parents_local and the counts
             against peer_twin.plan, as integers, each call made twice into sentinel-filled outputs
  arguments  every refusal returns its error and writes nothing

The probe exists in the hooks build only, and two builds of the library do not share a process: outside a process that has loaded
the hooks build, the first test here re-runs this file once in a child with RBS_LIB_PATH set to it, and every test reports its own
outcome of that run."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import peer_cases as pc
import peer_probes as pp
import peer_twin as pt
import scenarios as sc
from dbot_ros_amd import RbSensor, _capi
from dbot_ros_amd.sensor import RbSensorError

pytestmark = pytest.mark.gpu

HOOKS = pp.hooks_path(_capi.LIB_PATH)
IN_HOOKS_PROCESS = os.path.abspath(_capi.LIB_PATH) == os.path.abspath(HOOKS)
LD = np.longdouble
COLS, ROWS = 80, 60
_child = {}
worst = {}


def _delegated(request):
    """True: this process has not loaded the hooks build -- the test's outcome is the one of the child run."""
    if IN_HOOKS_PROCESS:
        return False
    if not _child:
        assert os.path.exists(HOOKS), "build() makes librbsensor_mi355x_hooks.so"
        _child["outcome"], _child["out"] = pp.child_outcomes(__file__, HOOKS, 900)
    assert _child["outcome"].get(request.node.name) == "PASSED", _child["out"]
    return True


@pytest.fixture(scope="module")
def probe(gpu_lib):
    return pp.PeerProbe(HOOKS) if IN_HOOKS_PROCESS else None


@pytest.fixture(scope="module")
def sensor_of(gpu_lib):
    """n -> a sensor of max_particles = 2 n on the small camera, made once per n."""
    made = {}

    def get(n, max_particles=None):
        cap = 2 * n if max_particles is None else max_particles
        if cap not in made:
            om, cam, P = sc.make_scene(("m1_l2",), COLS, ROWS, max_particles=cap)
            made[cap] = RbSensor(om, cam, P, max_particles=cap)
        return made[cap]
    yield get
    for s in made.values():
        s.close()


def _bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def _same_scratch(a, b):
    return _bits_equal(a["cdf"], b["cdf"]) and _bits_equal(a["tile_total"], b["tile_total"]) and \
        (a["tile_max"] is None) == (b["tile_max"] is None) and (a["tile_max"] is None or _bits_equal(a["tile_max"], b["tile_max"]))


def _run_ranks(probe, call, ranks, plan_of=None, repeats=1):
    """Every rank's call: parents_local == the scratch block's `mine`, the scratch arrays the same bits on every rank, the plan
    the twin's plan of the parents the device itself chose (plan_of: of these parents instead).
    -> the parents of the ranks run, concatenated; the scratch arrays."""
    parents, first = [], None
    for rank in ranks:
        pidx, src, dst, loc, counts = call.run(rank, repeats)
        got = probe.scratch(call.s, call.N, call.n)
        assert np.array_equal(got["mine"], loc), rank
        first = first or got
        assert _same_scratch(first, got), rank
        assert loc.min() >= 0 and loc.max() < call.N, rank
        every = np.zeros(call.N, dtype=np.int64)
        every[rank * call.n:(rank + 1) * call.n] = loc
        t_pidx, t_src, t_dst, t_cnt = pt.plan(every if plan_of is None else plan_of, call.n, 2 * call.n, rank, call.min_share)
        assert np.array_equal(pidx, t_pidx) and np.array_equal(src, t_src) and np.array_equal(dst, t_dst), rank
        assert counts.tolist() == [repeats * c for c in t_cnt], (rank, counts.tolist(), t_cnt)
        parents.append(loc)
    return np.concatenate(parents), first


# ---------------------------------------------------------------- the probe itself
def test_peer_probe_refuses_bad_arguments(request, probe, sensor_of):
    if _delegated(request):
        return
    assert all(hasattr(probe.lib, s) for s in pp.PEER_SYMBOLS)
    om, cam, P = sc.make_scene(("m1_l2",), COLS, ROWS, max_particles=8)
    a = [np.full(4, pp.SENTINEL) for _ in range(3)] + [np.full(4, pp.ISENTINEL, dtype=np.int32)]
    with RbSensor(om, cam, P, max_particles=8) as s:
        h = C.c_void_p(s._h.value)
        assert probe.raw(None, *[pp._p(x) for x in a]) == pp.RBS_ERR_INVALID_ARGUMENT
        assert probe.raw(h, *[pp._p(x) for x in a]) == pp.RBS_ERR_INVALID_ARGUMENT          # no call yet
        call = pp.PeerCall(s, np.zeros(4), np.array([0.1, 0.3, 0.6, 0.9]), 4)
        call.run(0)
        for k in range(4):
            args = [pp._p(x) for x in a]
            args[k] = None
            assert probe.raw(h, *args) == pp.RBS_ERR_INVALID_ARGUMENT, k
        assert all(np.all(x == (pp.ISENTINEL if x.dtype == np.int32 else pp.SENTINEL)) for x in a)
        got = probe.scratch(s, 4, 4)
        assert got["tile_max"] is None and got["cdf"].tolist() == [1.0, 2.0, 3.0, 4.0] and got["tile_total"].tolist() == [4.0]
        assert got["mine"].tolist() == [0, 1, 2, 3]


# ---------------------------------------------------------------- a. exact layer
@pytest.mark.parametrize("N,world", pc.EXACT_JOBS)
@pytest.mark.parametrize("power_of_two", [True, False])
def test_exact_weights_give_the_counted_parents_and_integer_sums(request, probe, sensor_of, N, world, power_of_two):
    if _delegated(request):
        return
    n = N // world
    ll, pos, u, kind, tj = pc.exact_case(N, power_of_two)
    expected = pc.exact_expected(N, pos, u)
    e_cdf, e_tot, e_max = pc.exact_scratch(N, ll, pos)
    call = pp.PeerCall(sensor_of(n), ll, u, n)
    ranks = pc.EXACT_RANKS.get(N, range(world))
    parents, got = _run_ranks(probe, call, ranks)
    want = np.concatenate([expected[r * n:(r + 1) * n] for r in ranks])
    bad = np.flatnonzero(parents != want)
    assert bad.size == 0, (bad[:8], parents[bad[:8]], want[bad[:8]])
    assert _bits_equal(got["cdf"], e_cdf) and _bits_equal(got["tile_total"], e_tot)
    assert (got["tile_max"] is not None) == (e_tot.size > pt.OWN_MAX_TILES)
    assert got["tile_max"] is None or _bits_equal(got["tile_max"], e_max)


# ---------------------------------------------------------------- b. where the maximum sits
@pytest.mark.parametrize("N,world", pc.MAX_JOBS)
def test_one_particle_at_every_edge_is_every_childs_parent(request, probe, sensor_of, N, world):
    """A missed maximum overflows exp.  (The parents alone would not show one missed at N - 1 -- tests/test_peer_twin_cpu.py -- so
    the scratch arrays are held to their exact values as well: the one particle weighs 1, exp(-800) is 0.)"""
    if _delegated(request):
        return
    n = N // world
    for T in pc.MAX_TEMPERATURES:
        for at in pc.max_positions(N):
            ll, u = pc.max_case(N, at, T)
            call = pp.PeerCall(sensor_of(n), ll, u, n, temperature=T)
            parents, got = _run_ranks(probe, call, range(world))
            assert np.all(parents == at), (T, at, np.flatnonzero(parents != at)[:8])
            e_cdf, e_tot = pc.max_scratch(N, at)
            assert _bits_equal(got["cdf"], e_cdf) and _bits_equal(got["tile_total"], e_tot), (T, at)
            assert (got["tile_max"] is not None) == (N > pt.OWN_MAX_TILES * pt.TILE)
            if got["tile_max"] is not None:
                e_max = np.full(e_tot.size, pc.C0 - 800.0 * T)
                e_max[at // pt.TILE] = pc.C0
                assert _bits_equal(got["tile_max"], e_max), (T, at)


# ---------------------------------------------------------------- c. weights and cumulative sums against the exact reference
@pytest.mark.parametrize("N,world", pc.CDF_JOBS)
@pytest.mark.parametrize("profile", pc.CDF_PROFILES)
def test_cumulative_weights_within_the_bar_and_parents_within_its_band(request, probe, sensor_of, profile, N, world):
    if _delegated(request):
        return
    n = N // world
    ll, T, u = pc.cdf_case(profile, N)
    S, E = pt.exact_cdf(ll, T)
    ok = pt.weighs(ll, T)
    lo, hi = pt.parents_band(S, E, u, ok)
    assert int((hi > lo).sum()) <= N * pc.AMBIGUOUS_CAP
    call = pp.PeerCall(sensor_of(n), ll, u, n, temperature=T)
    parents, got = _run_ranks(probe, call, range(world))
    cdf, ttot = got["cdf"], got["tile_total"]
    tiles = ttot.size
    before = np.concatenate([[LD(0)], np.cumsum(ttot.astype(LD))[:-1]])
    x = np.repeat(before, pt.TILE)[:N] + cdf.astype(LD)
    ratio = float((np.abs(x - S) / E).max())
    S_tile, E_tile = pt.exact_tiles(ll, T)
    ratio_t = float((np.abs(ttot.astype(LD) - S_tile) / E_tile).max())
    print(f"peer cdf / E: {profile} N={N}: cumulative {ratio:.3f}, tile totals {ratio_t:.3f}")
    worst[profile] = max(worst.get(profile, 0.0), ratio, ratio_t)
    assert ratio <= 1.0 and ratio_t <= 1.0, (ratio, ratio_t)
    for k in range(tiles):
        assert np.all(np.diff(cdf[k * pt.TILE:(k + 1) * pt.TILE]) >= 0.0), k
    bad = np.flatnonzero((parents < lo) | (parents > hi))
    assert bad.size == 0, (bad[:8], parents[bad[:8]], lo[bad[:8]], hi[bad[:8]])
    assert ok[parents].all()
    assert np.all(np.diff(parents) >= 0)
    if (N, world) == pc.CDF_JOBS[-1]:
        print(f"peer cdf / E: worst over the sizes, {profile}: {worst[profile]:.3f}")


# ---------------------------------------------------------------- d. no child inherits from a weightless particle
def test_no_child_inherits_from_a_weightless_particle(request, probe, sensor_of):
    """The last cumulative value and the total are the same sum in two associations, so 1 - 2^-53 can lie at or beyond the former;
    the search used to clamp such a child to particle N - 1 whatever it weighed (in a CPU restatement of the kernels' order, two
    of these 64 jobs).  peer_search_kernel now steps back to the last particle that weighs anything."""
    if _delegated(request):
        return
    for seed in range(pc.TAIL_SEEDS):
        N, n, ll, u, tail = pc.tail_case(seed)
        call = pp.PeerCall(sensor_of(n), ll, u, n)
        parents, got = _run_ranks(probe, call, range(N // n))
        assert not np.isnan(ll[parents]).any(), (seed, np.flatnonzero(np.isnan(ll[parents]))[:8])
        assert parents[-1] == N - tail - 1, (seed, int(parents[-1]), N, tail)
        assert np.all(np.diff(parents) >= 0), seed


def test_a_job_in_which_nobody_weighs_anything(request, probe, sensor_of):
    """Every log-likelihood NaN: the call succeeds, the parents are valid indices and the plan is the plan of those parents.
    PINNED, not specified: every child's parent is particle 0 (every comparison against 0 / 0 fails), as before this file existed."""
    if _delegated(request):
        return
    N, world = 2049, 3
    n = N // world
    u = np.sort(np.random.default_rng(5).random(N))
    call = pp.PeerCall(sensor_of(n), np.full(N, np.nan), u, n)
    parents, got = _run_ranks(probe, call, range(world))          # (RBS_OK, indices in [0, N), the twin's plan: inside)
    assert np.all(parents == 0)
    assert np.all(got["cdf"] == 0.0) and np.all(got["tile_total"] == 0.0)


# ---------------------------------------------------------------- e. the plan, on planted parents
_PLAN_CASES = pc.plan_cases()


@pytest.mark.parametrize("case", range(len(_PLAN_CASES)), ids=[c[0] for c in _PLAN_CASES])
def test_plan_of_planted_parents(request, probe, sensor_of, case):
    if _delegated(request):
        return
    name, world, n, shares, p, check = _PLAN_CASES[case]
    check(p)
    N = world * n
    for min_share in shares:
        call = pp.PeerCall(sensor_of(n), np.full(N, pc.C0), pc.uniforms_for(p, N), n, min_share=min_share)
        parents, got = _run_ranks(probe, call, range(world), plan_of=p, repeats=2)
        assert np.array_equal(parents, p), (min_share, np.flatnonzero(parents != p)[:8])


# ---------------------------------------------------------------- f. argument checks
def test_refused_calls_return_their_error_and_write_nothing(request, probe, sensor_of):
    if _delegated(request):
        return
    n = 2048
    s = sensor_of(n)
    big = (1 << 21) + 2048
    d_ll = torch.full((big,), pc.C0, dtype=torch.float64, device="cuda")
    d_u = torch.linspace(0.0, 0.999, big, dtype=torch.float64, device="cuda")
    good = dict(N=4 * n, n=n, rank=1, min_share=2, T=1.0)
    refusals = [("N = 2^21 + 2048", dict(N=big), pp.RBS_ERR_UNSUPPORTED), ("N no multiple of n", dict(N=4 * n + 1), pp.RBS_ERR_INVALID_ARGUMENT),
                ("rank = world", dict(rank=4), pp.RBS_ERR_INVALID_ARGUMENT), ("rank < 0", dict(rank=-1), pp.RBS_ERR_INVALID_ARGUMENT),
                ("T = 0", dict(T=0.0), pp.RBS_ERR_INVALID_ARGUMENT), ("T < 0", dict(T=-1.0), pp.RBS_ERR_INVALID_ARGUMENT),
                ("T NaN", dict(T=float("nan")), pp.RBS_ERR_INVALID_ARGUMENT), ("min_share 0", dict(min_share=0), pp.RBS_ERR_INVALID_ARGUMENT),
                ("max_particles < 2 n", dict(N=4 * (n + 1), n=n + 1), pp.RBS_ERR_INVALID_ARGUMENT)]
    for what, change, code in refusals:
        a = dict(good, **change)
        out = [torch.full((a["n"],), pp.ISENTINEL, dtype=torch.int32, device="cuda") for _ in range(4)]
        counts = torch.full((4,), pp.ISENTINEL, dtype=torch.int64, device="cuda")
        with pytest.raises(RbSensorError) as e:
            s.peer_resample(d_ll.data_ptr(), d_u.data_ptr(), a["N"], a["n"], a["rank"], a["min_share"], a["T"], out[0].data_ptr(),
                            out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), counts.data_ptr())
        assert e.value.code == code, (what, e.value.code)
        s.synchronize()
        torch.cuda.synchronize()
        assert all(bool((o == pp.ISENTINEL).all()) for o in out + [counts]), what
    # ... and the handle still serves the call as given
    call = pp.PeerCall(s, np.full(4 * n, pc.C0), pc.uniforms_for(np.arange(4 * n), 4 * n), n)
    parents, got = _run_ranks(probe, call, range(4))
    assert np.array_equal(parents, np.arange(4 * n))
