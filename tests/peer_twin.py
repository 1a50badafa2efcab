"""The plain reference of resampling across processes (dbot_ros_amd/csrc/rbsensor_peers.hip, rbs_peer_resample): numpy and
Python loops, written from the comment block at the head of that file and from nothing in dbot_ros_amd.dist.

exact_cdf      the cumulative weights in np.longdouble and the first-order bar E on the device's value of each
exact_tiles    the same for each tile's own weight
parents_band   per child the interval of parents that bar leaves open
plan           one rank's plan of its children, run by run
kernel_order_* a binary64 restatement of the kernels' SUMMATION ORDER (two particles a thread, Hillis-Steele wave scans, sixteen wave
               totals in order, the tiles' totals scanned the same way) with switches that break it on purpose:
               tests/test_peer_twin_cpu.py shows that the bar holds the restatement and that each broken version leaves it.  The
               device tests never compare against it.

The bar.  With m the largest log-likelihood (NaN dropped), x_j = (l_j - m) / T, w_j = exp(x_j) (NaN: 0), S_i = sum_{j <= i} w_j,

    E_i = 2^-53 ( sum_{j <= i} w_j (2 |x_j| + 2) + D S_i ) + 2^-1073 (i + 1)

bounds |device value of (weight of the tiles before i's + cumulative weight inside the tile) - S_i| to first order: the
subtraction and the division each round the argument once (2 |x_j|, as exp' = exp), exp itself is allowed two units, and every
weight passes through at most D additions on its way into a value.  Counted from the kernels: the pair add w0 + w1 (1), six levels
of the wave scan (6), sixteen wave totals (16), base + exc (1), before + w (1) -- 25 inside a tile; a weight of an EARLIER tile
reaches the tile's total after 1 + 6 + 16 = 23, then passes the tiles' scan (6 + 16 + 1), the carry (1) and tile_before + cdf (1):
48.  D = 64, the next power of two.  The last term is for weights in the subnormal range, where exp's error is absolute (sums of
subnormals are exact)."""
import numpy as np

import gauss_reference as gr

LD = np.longdouble
U = 2.0 ** -53
D_ADDS = 64
TILE, THREADS, WAVE = 2048, 1024, 64
OWN_MAX_TILES, SAMPLES, LDS_CHILDREN, MAX_TILES = 16, 2048, 4096, 1024


# ---------------------------------------------------------------- the exact cumulative weights and their bar
def weighs(ll, temperature):
    """Which particles weigh anything in binary64: not NaN, and exp((l - m) / T) does not underflow to zero."""
    ll = np.asarray(ll, dtype=np.float64)
    ok = ~np.isnan(ll)
    if not ok.any():
        return ok
    m = ll[ok].max()
    with np.errstate(invalid="ignore", under="ignore"):
        return ok & (np.exp((np.where(ok, ll, m) - m) / temperature) > 0.0)


def _terms(ll, temperature):
    """-> w_j and w_j (2 |x_j| + 2), np.longdouble."""
    gr.require_extended()
    ll = np.asarray(ll, dtype=np.float64)
    ok = ~np.isnan(ll)
    if not ok.any():
        return np.zeros(ll.size, dtype=LD), np.zeros(ll.size, dtype=LD)
    m = LD(ll[ok].max())
    with np.errstate(invalid="ignore", under="ignore", over="ignore"):
        x = (np.where(ok, ll, m).astype(LD) - m) / LD(temperature)
        w = np.where(ok, np.exp(x), LD(0))
        ax = np.where(w > 0, np.abs(x), LD(0))           # (-inf weighs nothing and errs by nothing)
    return w, w * (2 * ax + 2)


def exact_cdf(ll, temperature):
    """-> S [N] np.longdouble, E [N] np.longdouble (see the module's docstring; D = 64 additions)."""
    w, e = _terms(ll, temperature)
    S = np.cumsum(w)                                       # (sequential, in 64-bit significands: N 2^-64 relative, far below the bar)
    return S, LD(U) * (np.cumsum(e) + D_ADDS * S) + LD(2.0) ** -1073 * np.arange(1, w.size + 1).astype(LD)


def exact_tiles(ll, temperature):
    """-> the weight of each tile of 2048 particles and the same bar over the tile's own terms (summed per tile, not differences
    of the cumulative values, whose own rounding is not small beside one tile's bar)."""
    w, e = _terms(ll, temperature)
    at = np.arange(0, w.size, TILE)
    S = np.add.reduceat(w, at)
    count = np.minimum(at + TILE, w.size) - at
    return S, LD(U) * (np.add.reduceat(e, at) + D_ADDS * S) + LD(2.0) ** -1073 * count.astype(LD)


def parents_band(S, E, u, weighing=None):
    """Per child the acceptable parents [lo, hi] (int64 arrays): lo = upper_bound over the largest values the device's normalised
    cumulative weights may take, hi = over the smallest.  The relative bar at a position is E_i / S_i plus E_N / S_N for the
    division by the total ("doubled").  Both are clamped to the last particle that weighs anything."""
    S, E, u = np.asarray(S, dtype=LD), np.asarray(E, dtype=LD), np.asarray(u, dtype=np.float64)
    N = S.size
    tot = S[N - 1]
    assert tot > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.where(S > 0, E / np.where(S > 0, S, LD(1)), LD(0)) + E[N - 1] / tot
    c = S / tot
    upper = np.maximum.accumulate(c * (1 + rel))
    lower = np.maximum.accumulate(c * (1 - rel))
    lo = np.searchsorted(upper, u.astype(LD), side="right")
    hi = np.searchsorted(lower, u.astype(LD), side="right")
    pos = np.flatnonzero(np.diff(np.concatenate([[LD(0)], S])) > 0) if weighing is None else np.flatnonzero(weighing)
    last = int(pos[-1])
    return np.minimum(lo, last).astype(np.int64), np.minimum(hi, last).astype(np.int64)


# ---------------------------------------------------------------- the plan of one rank
def plan(parents_sorted, n, cap, rank, min_share):
    """Rank `rank` evaluates children [rank n, (rank + 1) n) of the sorted parents.  Child k inherits from the GLOBAL slot
    owner * cap + local slot of its parent -- unless the parent lives on another rank and at least min_share of THIS rank's
    children share it: then the run's first child stages the parent's window into the local staging slot n + j (j: staged windows
    so far) and every child of the run reads slot rank * cap + n + j.
    -> parent_idx, stage_src, stage_dst [n] int32; (remote children, of them served from staging, windows staged, runs)."""
    mine = [int(p) for p in np.asarray(parents_sorted)[rank * n:(rank + 1) * n]]
    assert len(mine) == n
    parent_idx, stage_src, stage_dst = [0] * n, [-1] * n, [-1] * n
    remote = shared = staged = runs = 0
    k = 0
    while k < n:
        e = k
        while e + 1 < n and mine[e + 1] == mine[k]:
            e += 1
        runs += 1
        p = mine[k]
        owner = p // n
        slot = owner * cap + (p - owner * n)
        length = e - k + 1
        if owner != rank:
            remote += length
        if owner != rank and length >= min_share:
            stage_src[k], stage_dst[k] = slot, n + staged
            for c in range(k, e + 1):
                parent_idx[c] = rank * cap + n + staged
            shared += length
            staged += 1
        else:
            for c in range(k, e + 1):
                parent_idx[c] = slot
        k = e + 1
    as32 = lambda a: np.asarray(a, dtype=np.int32)   # noqa: E731
    return as32(parent_idx), as32(stage_src), as32(stage_dst), (remote, shared, staged, runs)


# ---------------------------------------------------------------- the kernels' summation order in binary64 (CPU checks only)
def _block_exscan_add(v):
    """block_exscan(OpAdd) over one value per thread [blocks][1024] -> (exclusive [blocks][1024], total [blocks])."""
    B = v.shape[0]
    inc = v.reshape(B, THREADS // WAVE, WAVE).copy()
    off = 1
    while off < WAVE:
        nxt = inc.copy()
        nxt[..., off:] = inc[..., :-off] + inc[..., off:]
        inc = nxt
        off <<= 1
    base = np.zeros((B, THREADS // WAVE))
    tot = np.zeros(B)
    for k in range(THREADS // WAVE):
        base[:, k] = tot
        tot = tot + inc[:, k, WAVE - 1]
    exc = np.zeros_like(inc)
    exc[..., 1:] = inc[..., :-1]
    return (base[:, :, None] + exc).reshape(B, THREADS), tot


def kernel_order_cdf(ll, temperature, miss_max_beyond=None, in_order=True):
    """peer_max_kernel / peer_weights_kernel -> cdf [N] (within tiles), tile_total [tiles], m.
    miss_max_beyond = i: a broken kernel whose maximum ignores the particles from index i on.  in_order = False: the partial sums as
    the scan leaves them, not raised to the largest before them (the kernel as it stood before that step)."""
    ll = np.asarray(ll, dtype=np.float64)
    N = ll.size
    tiles = (N + TILE - 1) // TILE
    seen = ll if miss_max_beyond is None else ll[:miss_max_beyond]
    seen = seen[~np.isnan(seen)]
    m = seen.max() if seen.size else -np.inf
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        w = np.where(np.isnan(ll), 0.0, np.exp((ll - m) / temperature))
    w = np.concatenate([w, np.zeros(tiles * TILE - N)]).reshape(tiles, THREADS, 2)
    with np.errstate(invalid="ignore", over="ignore"):
        pair = w[..., 0] + w[..., 1]
        before, total = _block_exscan_add(pair)
        cdf = np.stack([before + w[..., 0], before + pair], -1).reshape(tiles, TILE)
        if in_order:
            cdf = np.maximum.accumulate(cdf, axis=1)
        cdf = cdf.reshape(-1)[:N]
    return cdf, total, m


def kernel_order_parents(ll, temperature, cdf, tile_total, u, tie_left=False, step_back=True):
    """peer_search_kernel: child g's parent at the sorted uniforms u [N] (every rank's children at once).
    tie_left: a broken search whose comparison is cdf < u.  step_back = False: the search as it stood before a child was kept from
    inheriting from a particle that weighs nothing (the clamp to N - 1 alone)."""
    N = cdf.size
    tiles = tile_total.size
    before, total = _block_exscan_add(np.concatenate([tile_total, np.zeros(MAX_TILES - tiles)])[None, :])
    tile_before, total = 0.0 + before[0, :tiles], 0.0 + total[0]
    with np.errstate(invalid="ignore", divide="ignore"):
        c = (np.repeat(tile_before, TILE)[:N] + cdf) / total
    if not total > 0.0:
        return np.zeros(N, dtype=np.int32), c            # (every comparison with NaN fails: the search ends at particle 0)
    p = np.minimum(np.searchsorted(c, u, side="left" if tie_left else "right"), N - 1)
    if step_back:
        ok = weighs(ll, temperature)
        last = np.maximum.accumulate(np.where(ok, np.arange(N), -1))
        p = np.where(last[p] >= 0, last[p], p)
    return p.astype(np.int32), c
