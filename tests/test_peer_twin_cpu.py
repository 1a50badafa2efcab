"""tests/peer_twin.py, the reference the device tests of resampling across processes compare with, and the planted inputs of those
tests (tests/peer_cases.py), WITHOUT a device:

  - the twin against the tensor path (dbot_ros_amd.dist.global_resample / plan_shard) on the ten parameter sets of
    tests/test_gpu_peers.py::test_peer_resample_matches_tensor_arithmetic;
  - the planted inputs meet the conditions their expected values rest on;
  - the bar E holds a binary64 restatement of the kernels' summation order, and each of four subtly broken kernels leaves the check
    that is there for it: a tie taken to the left, a maximum missed in a partial tile, a staging index not carried across the
    4096-child tile of the one-sweep plan, the clamp to N - 1 of a child whose uniform lies at or beyond the last cumulative value."""
import numpy as np
import pytest
import torch

import peer_cases as pc
import peer_twin as pt
from dbot_ros_amd import dist as rdist

LD = np.longdouble
TENSOR_SETS = [(2, 48, 2, 1.0, 3.0), (4, 500, 2, 1.0, 0.05), (8, 2000, 2, 50.0, 30.0), (3, 1111, 3, 1.0, 1.0), (2, 25000, 2, 1.0, 200.0),
               (1, 64, 2, 1.0, 1.0), (4, 3000, 2, 1.0, 6.0), (8, 25000, 2, 1.0, 2.0), (2, 5000, 3, 1.0, 4.0), (4, 6250, 2, 1.0, 40.0)]


def _tensor_inputs(world, n, spread):
    """The inputs of test_peer_resample_matches_tensor_arithmetic."""
    N = world * n
    rng = np.random.default_rng(world * 1000 + n)
    ll = rng.normal(-3000.0, spread, N)
    ll[rng.integers(0, N, 3)] = np.nan if n > 100 else ll[0]
    g = torch.Generator().manual_seed(n)
    return ll, torch.sort(torch.rand(N, dtype=torch.float64, generator=g)).values


@pytest.mark.parametrize("world,n,min_share,temp,spread", TENSOR_SETS)
def test_twin_agrees_with_the_tensor_path(world, n, min_share, temp, spread):
    ll, u = _tensor_inputs(world, n, spread)
    ps = rdist.global_resample(torch.from_numpy(np.where(np.isnan(ll), -np.inf, ll)), u, temp)
    S, E = pt.exact_cdf(ll, temp)
    lo, hi = pt.parents_band(S, E, u.numpy(), pt.weighs(ll, temp))
    one = lo == hi
    assert one.mean() >= 1.0 - pc.AMBIGUOUS_CAP
    assert np.array_equal(ps.numpy()[one], lo[one])
    assert np.all((ps.numpy() >= lo) & (ps.numpy() <= hi))
    for rank in range(world):
        pidx, src, dst, cnt = rdist.plan_shard(ps, n, 2 * n, rank, min_share)
        t_pidx, t_src, t_dst, t_cnt = pt.plan(ps.numpy(), n, 2 * n, rank, min_share)
        assert np.array_equal(pidx.numpy(), t_pidx) and np.array_equal(src.numpy(), t_src) and np.array_equal(dst.numpy(), t_dst), rank
        mine = ps[rank * n:(rank + 1) * n]
        assert list(t_cnt) == [int(c) for c in cnt] + [int((mine[1:] != mine[:-1]).sum()) + 1], rank


def test_tensor_path_never_hands_a_child_to_a_weightless_particle():
    """global_resample on the inputs of the device's sweep: its own last value normalises it, and its step back (the rule of
    peer_search_kernel) covers a parallel cumsum, which is flat over a weightless particle only up to its last bit."""
    for seed in range(pc.TAIL_SEEDS):
        N, n, ll, u, tail = pc.tail_case(seed)
        ps = rdist.global_resample(torch.from_numpy(np.where(np.isnan(ll), -np.inf, ll)), torch.from_numpy(u))
        assert int(ps[-1]) == N - tail - 1 and not np.isnan(ll[ps.numpy()]).any(), seed


# ---------------------------------------------------------------- the planted inputs
@pytest.mark.parametrize("N,world", pc.EXACT_JOBS)
@pytest.mark.parametrize("power_of_two", [True, False])
def test_exact_layer_inputs(N, world, power_of_two):
    ll, pos, u, kind, tj = pc.exact_case(N, power_of_two)
    W = pos.size
    assert N % world == 0 and u.size == N and np.all(np.diff(u) >= 0) and u[0] == 0.0 and (N == 1 or u[-1] == pc.BELOW_ONE)
    assert set(np.unique(ll[~np.isnan(ll)])) <= {pc.C0, -np.inf} and np.array_equal(np.flatnonzero(ll == pc.C0), pos)
    tie = kind == 2
    assert np.array_equal(u[tie].view(np.uint64), (tj[tie].astype(np.float64) / float(W)).view(np.uint64))     # bit-equal to j / W
    if N > 1:
        assert tie.sum() >= min(W - 1, 100) and (kind == 1).any() and (kind == 3).any()
        assert {0, W - 1} <= set(tj[tie].tolist()) | {0}
    expected = pc.exact_expected(N, pos, u)
    assert np.array_equal(expected[tie], pos[tj[tie]])                            # a tie goes right: the (j + 1)-th that weighs
    if N > 8:                                                                     # the weightless stretches
        tiles = (N + pc.TILE - 1) // pc.TILE
        assert pos[0] >= 4 and pos[-1] <= N - 5
        if tiles >= 2:
            assert not np.isin(np.arange(pc.TILE - 3, min(N, pc.TILE + 2)), pos).any()
        if tiles >= 4:
            k = tiles // 2
            assert not np.isin(np.arange(k * pc.TILE, (k + 1) * pc.TILE), pos).any() and {k * pc.TILE - 1, (k + 1) * pc.TILE} <= set(pos.tolist())
    # the restatement of the kernels' order gives the counted parents; a search that takes ties to the left does not
    cdf, ttot, _ = pt.kernel_order_cdf(ll, 1.0)
    e_cdf, e_tot, _ = pc.exact_scratch(N, ll, pos)
    assert np.array_equal(cdf, e_cdf) and np.array_equal(ttot, e_tot)
    assert np.array_equal(pt.kernel_order_parents(ll, 1.0, cdf, ttot, u)[0], expected)
    if N > 1:
        left = pt.kernel_order_parents(ll, 1.0, cdf, ttot, u, tie_left=True)[0]
        assert np.all(left[tie] != expected[tie])


def test_steered_uniforms_keep_clear_of_every_cumulative_value():
    for name, world, n, shares, p, check in pc.plan_cases():
        N = world * n
        check(p)
        u = pc.uniforms_for(p, N)
        assert np.all(np.diff(u) >= 0)
        S, E = pt.exact_cdf(np.full(N, pc.C0), 1.0)
        c = (S / S[N - 1]).astype(LD)
        at = np.searchsorted(c, u.astype(LD))
        near = np.minimum(np.abs(c[np.minimum(at, N - 1)] - u), np.abs(c[np.maximum(at - 1, 0)] - u))
        assert float(near.min()) >= 0.25 / N, name
        lo, hi = pt.parents_band(S, E, u)
        assert np.array_equal(lo, p) and np.array_equal(hi, p), name
        cdf, ttot, _ = pt.kernel_order_cdf(np.full(N, pc.C0), 1.0)
        assert np.array_equal(pt.kernel_order_parents(np.full(N, pc.C0), 1.0, cdf, ttot, u)[0], p), name


@pytest.mark.parametrize("profile", pc.CDF_PROFILES)
def test_random_cases_are_decided_and_the_bar_holds_the_kernels_order(profile):
    for N, world in pc.CDF_JOBS:
        ll, T, u = pc.cdf_case(profile, N)
        S, E = pt.exact_cdf(ll, T)
        ok = pt.weighs(ll, T)
        lo, hi = pt.parents_band(S, E, u, ok)
        assert N % world == 0 and int((hi > lo).sum()) <= N * pc.AMBIGUOUS_CAP, (N, int((hi > lo).sum()))
        cdf, ttot, _ = pt.kernel_order_cdf(ll, T)
        before = np.concatenate([[LD(0)], np.cumsum(ttot.astype(LD))[:-1]])
        x = np.repeat(before, pc.TILE)[:N] + cdf.astype(LD)
        S_tile, E_tile = pt.exact_tiles(ll, T)
        assert float((np.abs(x - S) / E).max()) < 1.0 and float((np.abs(ttot.astype(LD) - S_tile) / E_tile).max()) < 1.0
        assert all(np.all(np.diff(cdf[k:k + pc.TILE]) >= 0) for k in range(0, N, pc.TILE))
        par = pt.kernel_order_parents(ll, T, cdf, ttot, u)[0]
        assert np.all((par >= lo) & (par <= hi)) and ok[par].all()
        # a cumulative sum wrong by 1e-9 relative leaves the bar
        assert float((np.abs(x * (1 + LD(1e-9)) - S) / E).max()) > 1.0


# ---------------------------------------------------------------- broken kernels leave their checks
def test_a_maximum_missed_in_a_partial_tile_is_seen():
    """peer_max_kernel without its second element in the last, partial tile (index N - 1 of an even N in a tile that is not full):
    the tile's maximum is not the exact one, the others weigh 1 instead of nothing and the one particle's exp overflows -- which
    the PARENTS alone would not show (every comparison against inf / inf fails and the search still ends at N - 1): the device
    test therefore holds tile_max, the weights' cumulative sums and the tiles' totals to their exact values as well."""
    for N, world in pc.MAX_JOBS:
        for T in pc.MAX_TEMPERATURES:
            ll, u = pc.max_case(N, N - 1, T)
            e_cdf, e_tot = pc.max_scratch(N, N - 1)
            cdf, ttot, m = pt.kernel_order_cdf(ll, T)
            assert m == pc.C0 and np.array_equal(cdf, e_cdf) and np.array_equal(ttot, e_tot)
            assert np.all(pt.kernel_order_parents(ll, T, cdf, ttot, u)[0] == N - 1)
            cdf, ttot, m = pt.kernel_order_cdf(ll, T, miss_max_beyond=N - 1)
            assert m != pc.C0 and not np.array_equal(cdf, e_cdf) and not np.array_equal(ttot, e_tot)
    assert any(N % 2 == 0 and N % pc.TILE for N, _ in pc.MAX_JOBS) and any(N % 2 == 1 for N, _ in pc.MAX_JOBS)
    assert any(N <= 32768 for N, _ in pc.MAX_JOBS) and any(N > 32768 for N, _ in pc.MAX_JOBS)


def test_a_staging_index_not_carried_across_the_tile_is_seen():
    """The one-sweep plan numbers staged windows tile by tile of 4096 children and carries the count.  A plan that starts every tile
    from zero differs from the twin's in the cases built for it."""
    seen = 0
    for name, world, n, shares, p, check in pc.plan_cases():
        if n <= 4096:
            continue
        pidx, src, dst, cnt = pt.plan(p, n, 2 * n, 1, 2)
        starts_before = np.cumsum(dst >= 0)[4095]
        broken = np.where(np.arange(n) >= 4096, np.where(dst >= 0, dst - starts_before, dst), dst)
        if name.startswith("run_"):
            assert starts_before > 0 and (dst[4096:] >= 0).any() and not np.array_equal(broken, dst), name
            # ... and the run that crosses the edge reads the window its first child staged
            assert pidx[4096] == 1 * 2 * n + dst[:4097][dst[:4097] >= 0][-1], name
            seen += 1
    assert seen >= 3


def test_the_clamp_hands_children_to_weightless_particles_and_the_step_back_does_not():
    taken = 0
    for seed in range(pc.TAIL_SEEDS):
        N, n, ll, u, tail = pc.tail_case(seed)
        assert 100 <= N <= 9000 and N % n == 0 and np.isnan(ll[N - tail:]).all() and not np.isnan(ll[:N - tail]).any() and u[-1] == pc.BELOW_ONE
        cdf, ttot, _ = pt.kernel_order_cdf(ll, 1.0, in_order=False)
        old = pt.kernel_order_parents(ll, 1.0, cdf, ttot, u, step_back=False)[0]
        taken += bool(old[-1] != N - tail - 1 or np.isnan(ll[old]).any())
        cdf, ttot, _ = pt.kernel_order_cdf(ll, 1.0)
        new = pt.kernel_order_parents(ll, 1.0, cdf, ttot, u)[0]
        assert new[-1] == N - tail - 1 and not np.isnan(ll[new]).any(), seed
    assert taken >= 1, taken           # (two of these 64 seeds)


def test_plan_twin_on_a_hand_worked_example():
    """n = 4, cap = 8, rank 1 of 2, parents 1 1 1 2 | 2 2 5 6: rank 1's children share remote parent 2 twice, then own 5 and 6."""
    p = np.array([1, 1, 1, 2, 2, 2, 5, 6])
    pidx, src, dst, cnt = pt.plan(p, 4, 8, 1, 2)
    assert pidx.tolist() == [8 + 4, 8 + 4, 8 + 1, 8 + 2] and src.tolist() == [2, -1, -1, -1] and dst.tolist() == [4, -1, -1, -1]
    assert cnt == (2, 2, 1, 3)
    pidx, src, dst, cnt = pt.plan(p, 4, 8, 1, 3)
    assert pidx.tolist() == [2, 2, 8 + 1, 8 + 2] and src.tolist() == [-1] * 4 and dst.tolist() == [-1] * 4 and cnt == (2, 0, 0, 3)
    pidx, src, dst, cnt = pt.plan(p, 4, 8, 0, 1)
    assert pidx.tolist() == [1, 1, 1, 2] and cnt == (0, 0, 0, 2)
