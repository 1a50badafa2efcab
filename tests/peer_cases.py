"""The planted inputs of tests/test_gpu_peer_kernels.py (numpy only, no device), so that tests/test_peer_twin_cpu.py can hold them
to their own conditions without a GPU.  Test infrastructure."""
import numpy as np

TILE = 2048
C0 = -3000.0                                 # the log-likelihood of a particle that weighs 1
BELOW_ONE = float(np.nextafter(1.0, 0.0))    # 1 - 2^-53, the largest uniform there is


# ---------------------------------------------------------------- 4a: weights that are exactly 1 or 0
# (N, world): n = N / world.  Around stride 1 -> 2 of the sampled search and one tile -> two; 16 tiles and 17 (peer_max_kernel);
# the largest job accepted.
EXACT_JOBS = [(1, 1), (2047, 23), (2048, 2), (2049, 3), (4095, 3), (32768, 4), (34816, 4), (1 << 21, 1024)]
EXACT_RANKS = {1 << 21: (0, 511, 1023)}


def exact_case(N, power_of_two):
    """-> ll [N] drawn from {C0, NaN, -inf}, pos (the particles that weigh 1), u [N] sorted, kind [N] (what each uniform is:
    0 zero, 1 below a tie, 2 the tie, 3 above it, 4 the last double below 1), tie_j [N] (the j of a tie's j / W, else -1).
    Weightless stretches: the first particles, the last ones, one whole tile, both sides of a tile edge."""
    rng = np.random.default_rng([N, int(power_of_two), 41])
    on = rng.random(N) < 0.7
    tiles = (N + TILE - 1) // TILE
    if N > 8:
        on[:min(5, N // 4)] = False
        on[N - min(7, N // 4):] = False
    if tiles >= 2:
        on[TILE - 3:TILE + 2] = False                        # both sides of the first tile edge
        on[TILE - 4] = True
        if TILE + 9 < N:
            on[TILE + 2] = True
    if tiles >= 4:
        k = tiles // 2
        on[k * TILE:(k + 1) * TILE] = False                  # a whole tile
        on[k * TILE - 1] = on[(k + 1) * TILE] = True
    if not on.any():
        on[N // 2] = True
    pos = np.flatnonzero(on)
    W = pos.size
    p2 = 1 << (W.bit_length() - 1)
    want = p2 if power_of_two else (W - 1 if W == p2 and W > 2 else W)
    if want != W:                                            # switch surplus particles off, none of the planted ones next to an edge
        keep = np.ones(W, dtype=bool)
        inner = np.arange(1, W - 1)
        planted = np.isin(pos[inner], [TILE - 4, TILE + 2]) | ((pos[inner] % TILE == 0) | (pos[inner] % TILE == TILE - 1))
        keep[rng.permutation(inner[~planted])[:W - want]] = False
        pos = pos[keep]
        W = pos.size
    assert W == want and ((W & (W - 1)) == 0) == bool(power_of_two or W <= 2), (N, W)
    ll = np.where(rng.random(N) < 0.5, np.nan, -np.inf)
    ll[pos] = C0
    # the uniforms: every j when three of each fit, else the first and last hundred and a random draw
    room = (N - 2) // 3
    if W <= room:
        js = np.arange(W)
    else:
        edge = np.concatenate([np.arange(min(W, 100)), np.arange(max(0, W - 100), W)])
        js = np.unique(np.concatenate([edge, rng.integers(0, W, max(0, room - edge.size))]))[:max(room, 0)]
    if js.size == 0:
        js = np.zeros(1, dtype=np.int64)
    ties = js.astype(np.float64) / float(W)
    u = [np.zeros(1), ties[1:], np.nextafter(ties[1:], -1.0), np.nextafter(ties, 2.0), np.array([BELOW_ONE])]
    kind = [np.zeros(1), np.full(ties.size - 1, 2), np.full(ties.size - 1, 1), np.full(ties.size, 3), np.array([4])]
    tj = [np.full(1, -1), js[1:], np.full(ties.size - 1, -1), np.full(ties.size, -1), np.full(1, -1)]
    u, kind, tj = (np.concatenate(a) for a in (u, kind, tj))
    u, kind, tj = u[:N], kind[:N], tj[:N]                     # (N = 1: the zero alone)
    if u.size < N:                                            # fill up with repeats
        again = rng.integers(0, u.size, N - u.size)
        u, kind, tj = (np.concatenate([a, a[again]]) for a in (u, kind, tj))
    order = np.argsort(u, kind="stable")
    return ll, pos, u[order], kind[order].astype(np.int64), tj[order].astype(np.int64)


def exact_expected(N, pos, u):
    """By counting: the i-th particle that weighs 1 (i = 1 .. W) has cumulative value i / W, one correctly rounded division of two
    integers on the device as here; the parent of u is the first of them whose value exceeds u."""
    W = pos.size
    c = np.arange(1, W + 1, dtype=np.float64) / float(W)
    return pos[np.minimum(np.searchsorted(c, u, side="right"), W - 1)].astype(np.int32)


def exact_scratch(N, ll, pos):
    """-> cdf [N] (counts within the tile), tile_total, tile_max [tiles]: the exact integers and the exact maximum."""
    tiles = (N + TILE - 1) // TILE
    on = np.zeros(tiles * TILE)
    on[pos] = 1.0
    cdf = np.cumsum(on.reshape(tiles, TILE), axis=1)
    padded = np.concatenate([np.where(np.isnan(ll), -np.inf, ll), np.full(tiles * TILE - N, -np.inf)])
    return cdf.reshape(-1)[:N], cdf[:, -1].copy(), padded.reshape(tiles, TILE).max(axis=1)


# ---------------------------------------------------------------- 4b: one particle, everybody else 800 T below
# (N, world): both routes of the maximum, even and odd N, a partial last tile (all but 34816)
MAX_JOBS = [(5096, 8), (5097, 3), (34816, 4), (34818, 6), (34817, 37)]
MAX_TEMPERATURES = [0.5, 1.0, 50.0]


def max_positions(N):
    tiles = (N + TILE - 1) // TILE
    k = tiles // 2
    return sorted({0, N - 1, k * TILE, (k + 1) * TILE - 1})


def max_case(N, at, T):
    ll = np.full(N, C0 - 800.0 * T)
    ll[at] = C0
    rng = np.random.default_rng([N, at])
    u = np.sort(rng.random(N))
    u[0], u[N - 1] = 0.0, BELOW_ONE
    return ll, u


def max_scratch(N, at):
    """-> cdf [N], tile_total [tiles]: the one particle weighs exactly 1 and exp(-800) is exactly 0."""
    tiles = (N + TILE - 1) // TILE
    cdf = np.zeros(N)
    cdf[at:min(N, (at // TILE + 1) * TILE)] = 1.0
    tot = np.zeros(tiles)
    tot[at // TILE] = 1.0
    return cdf, tot


# ---------------------------------------------------------------- 4c: weights against the exact reference
# (N, world): 1111 x 3, 2049, 34816 (17 tiles), 200 000 = 8 x 25 000
CDF_JOBS = [(3333, 3), (2049, 3), (34816, 4), (200000, 8)]
CDF_PROFILES = ["spread0.05", "spread3", "spread200", "flat50", "dominant", "decay600", "scattered"]
AMBIGUOUS_CAP = 1e-4                          # at most 1 child in 10 000 may have a band of more than one parent


def cdf_case(profile, N):
    """-> ll [N], temperature, u [N] sorted (random: the planted ones are the other layers')."""
    rng = np.random.default_rng([N, CDF_PROFILES.index(profile), 7])
    T = 1.0
    if profile.startswith("spread"):
        ll = rng.normal(C0, float(profile[6:]), N)
    elif profile == "flat50":
        ll, T = rng.normal(C0, 30.0, N), 50.0
    elif profile == "dominant":
        ll = rng.normal(C0 - 40.0, 3.0, N)
        ll[(2 * N) // 3] = C0
    elif profile == "decay600":                       # late terms are absorbed by the sum before them
        ll = C0 - 600.0 * np.arange(N) / N
    else:
        ll = rng.normal(C0, 3.0, N)
        ll[rng.random(N) < 0.05] = np.nan
        ll[rng.random(N) < 0.05] = -np.inf
    return ll, T, np.sort(rng.random(N))


# ---------------------------------------------------------------- 4d: a weightless tail and the largest uniform
TAIL_SEEDS = 64
TAIL_LOCAL = (97, 100, 101, 128)


def tail_case(seed):
    """-> N, n, ll (normal, the last 1 to 5 NaN), u sorted with the last one 1 - 2^-53.  N is random in [100, 9000]."""
    rng = np.random.default_rng([seed, 4])
    n = TAIL_LOCAL[seed % len(TAIL_LOCAL)]
    world = int(rng.integers((100 + n - 1) // n, 9000 // n + 1))
    N = world * n
    ll = rng.normal(C0, 3.0, N)
    tail = int(rng.integers(1, 6))
    ll[N - tail:] = np.nan
    u = np.sort(rng.random(N))
    u[N - 1] = BELOW_ONE
    return N, n, ll, u, tail


# ---------------------------------------------------------------- 4e: the plan on planted parents
def uniforms_for(parents, N):
    """With N equal log-likelihoods particle p has the cumulative value (p + 1) / N, so u = (p + 0.5) / N has parent p exactly."""
    return (np.asarray(parents, dtype=np.float64) + 0.5) / float(N)


def run_lengths(n, rng, lens, forced=()):
    """Run lengths that sum to n: every forced (first child, last child) run in its place, the rest drawn from `lens` in shuffled rounds."""
    out, k, bag = [], 0, []
    for a, b in list(forced) + [(n, n)]:
        while k < a:
            if not bag:
                bag = [int(L) for L in rng.permutation(lens)]     # (every length comes round)
            L = min(bag.pop(), a - k)
            out.append(L)
            k += L
        if a < n:
            out.append(b - a + 1)
            k = b + 1
    assert sum(out) == n
    return out


def parents_from_runs(world, n, lens_per_rank, remote_share=0.5, share_across=False):
    """The sorted parents of all world * n children: rank r's runs take increasing parents, the first remote_share of them on
    earlier ranks' particles (rank 0: its own), the rest from r n on -- its own, until they run out.  share_across: every rank's
    first run continues the previous rank's last parent."""
    p, nxt = [], 0
    for r, lens in enumerate(lens_per_rank):
        h = int(len(lens) * remote_share)
        for j, L in enumerate(lens):
            if j == h:
                nxt = max(nxt, r * n)
            if j == 0 and r > 0 and share_across:
                parent = p[-1]
            else:
                parent, nxt = nxt, nxt + 1
            p += [parent] * L
    p = np.asarray(p, dtype=np.int64)
    assert p.size == world * n and np.all(np.diff(p) >= 0) and p[-1] < world * n
    return p


def runs_of(p, n, rank):
    """[(first child, last child, parent, remote)] of rank `rank`, children numbered within the rank."""
    mine = p[rank * n:(rank + 1) * n]
    cut = np.flatnonzero(np.diff(mine) != 0)
    a = np.concatenate([[0], cut + 1])
    b = np.concatenate([cut, [n - 1]])
    return [(int(x), int(y), int(mine[x]), int(mine[x]) // n != rank) for x, y in zip(a, b)]


def plan_cases():
    """-> [(name, world, n, [min_share, ...], parents [world n], check)]: check(p) asserts on the host that the structure the
    case is named after is there."""
    cases = []

    def add(name, world, n, shares, p, check):
        check(p)
        cases.append((name, world, n, shares, p, check))

    for ms in (1, 2, 3, 5):                               # runs of min_share - 1, min_share, min_share + 1, remote and local
        lens = [L for L in (ms - 1, ms, ms + 1) if L > 0]
        rng = np.random.default_rng([ms, 1])
        n = 96
        p = parents_from_runs(3, n, [run_lengths(n, rng, lens) for _ in range(3)])

        def check(p, n=n, lens=lens):
            for r in (1, 2):
                for remote in (False, True):
                    assert {b - a + 1 for a, b, _, rm in runs_of(p, n, r) if rm == remote} >= set(lens), (r, remote)
        add(f"lengths_around_min_share_{ms}", 3, n, [ms], p, check)

    def forced_case(name, n, run, shares, remote=True):
        rng = np.random.default_rng([n, run[0]])
        lens = [run_lengths(n, rng, (2, 3)), run_lengths(n, rng, (1, 2, 3), forced=[run])]
        p = parents_from_runs(2, n, lens, remote_share=1.0 if remote else 0.5)

        def check(p, n=n, run=run, remote=remote):
            rs = runs_of(p, n, 1)
            assert (run[0], run[1]) in {(a, b) for a, b, _, rm in rs if rm == remote}
            assert sum(1 for a, b, _, rm in rs if rm and b > a and a < run[0]) > 0                 # windows are staged before it
        add(name, 2, n, shares, p, check)

    forced_case("run_4095_to_4097", 6250, (4095, 4097), [2, 3])
    forced_case("run_4000_to_8200", 8300, (4000, 8200), [2, 3])
    forced_case("run_from_4096", 6250, (4096, 4098), [2, 3])
    forced_case("local_run_4095_to_4097", 6250, (4095, 4097), [2], remote=False)

    rng = np.random.default_rng(11)                       # the one-sweep plan's thread edge: every fourth child
    n = 203
    p = parents_from_runs(2, n, [run_lengths(n, rng, (1, 2, 3)) for _ in range(2)], remote_share=1.0)

    def check(p, n=n):
        shared = [(a, b) for a, b, _, rm in runs_of(p, n, 1) if rm and b > a]
        assert {a % 4 for a, b in shared} == {0, 1, 2, 3} and {b % 4 for a, b in shared} == {0, 1, 2, 3}
        assert any(a % 4 == 3 for a, b in shared) and any(a % 4 == 2 and b % 4 == 0 for a, b in shared)   # runs across an edge
    add("ends_around_every_fourth_child", 2, n, [2], p, check)

    for n in (1030, 4096, 4097):                          # the general plan: empty chunks from thread 515 on; LDS / memory
        rng = np.random.default_rng(n)
        p = parents_from_runs(2, n, [run_lengths(n, rng, (1, 2, 3, 4)) for _ in range(2)], remote_share=0.7)

        def check(p, n=n):
            ls = {b - a + 1 for a, b, _, rm in runs_of(p, n, 1) if rm}
            assert ls >= {2, 3, 4}
        add(f"general_plan_n_{n}", 2, n, [3], p, check)

    n = 4500                                              # all of rank 1's children on one remote parent
    p = np.zeros(2 * n, dtype=np.int64)

    def check(p, n=n):
        assert runs_of(p, n, 1) == [(0, n - 1, 0, True)]
    add("one_remote_parent", 2, n, [2, 3], p, check)
    n = 100                                               # every child its own slot's
    p = np.arange(3 * n, dtype=np.int64)

    def check(p, n=n):
        assert all(not rm for r in range(3) for *_, rm in runs_of(p, n, r))
    add("all_local", 3, n, [2, 3], p, check)
    n = 300
    rng = np.random.default_rng(300)
    p = parents_from_runs(1, n, [run_lengths(n, rng, (1, 2, 3))])

    def check(p, n=n):
        assert all(not rm for *_, rm in runs_of(p, n, 0))
    add("world_1", 1, n, [2, 3], p, check)
    n = 96                                                # runs are per rank: a parent's children on two ranks are two runs
    rng = np.random.default_rng(96)
    p = parents_from_runs(3, n, [run_lengths(n, rng, (1, 2, 3)) for _ in range(3)], share_across=True)

    def check(p, n=n):
        assert p[n - 1] == p[n] and p[2 * n - 1] == p[2 * n]
    add("parent_shared_across_ranks", 3, n, [2, 3], p, check)
    return cases
