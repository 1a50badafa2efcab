"""The object finder's kernels (dbot_ros_amd/csrc/rbsensor_find.hip) ON THE DEVICE, one by one, on planted inputs, against
the plain reference tests/find_twin.py.

The test build of the library (librbsensor_mi355x_hooks.so) has rbs_test_find_*: one entry point per launch helper of
rbsensor_find.hip (the helpers rbs_find_run itself calls; no kernel body and no launch geometry is restated), host arrays
in and out, every output a sentinel-filled tail longer than the kernel may write (tests/find_probes.py).

Bars.  Everything integer or copied is exact: seeds, cells, info, top-k indices and scores (scores as bits where they are
numbers, as isnan where they are not), kept positions and the keep kernel's rows, select, order, subsample, gather against
hyp, child 0.  The suppression's decisions are the twin's, which evaluates d2 and the trace in the kernel's operation order in
binary64.  Transcendental outputs are held to the extended-precision twin (find_twin.*_ext: mpmath at 40 digits where it
is installed, long double otherwise):
  children and their normals   1e-14 absolute (the bar of test_stages_match_the_twin); measured 3.2e-16 and 1.4e-15, the binary64
                               twin 3.2e-16 and 1.4e-15
  hypotheses                   1e-15 absolute where the binary64 twin itself is that close to the extended one; else twice the
                               binary64 twin's own distance from it at that size (the rule of
                               test_f32_pixel_term_stays_within_twice_the_twin_error): the spiral's angles 2 pi (i + 1/2) / sqrt 2
                               reach 4 600 rad at 1 024 rotations and 4.7e6 rad at 2^20, and one rounding of such an angle is
                               5e-13 and 5e-10 rad.  Measured figures: HYP_MEASURED below.

The probes exist in the hooks build only, and two builds of the library do not share a process: outside a process that has
loaded the hooks build, the first test here re-runs this file once in a child with RBS_LIB_PATH set to it, and every test
reports its own outcome of that run."""
import math
import os

import numpy as np
import pytest

import find_probes as fp
import find_twin as tw
from dbot_ros_amd import _capi
from find_probes import TAIL, untouched

pytestmark = pytest.mark.gpu

HOOKS = fp.hooks_path(_capi.LIB_PATH)
IN_HOOKS_PROCESS = os.path.abspath(_capi.LIB_PATH) == os.path.abspath(HOOKS)
BIG_SEED = 0xC0FFEE1234ABCDEF
_child = {}
worst = {}                                     # the largest differences seen, printed by the last test

# n_rot: (device against the extended twin, binary64 twin against the extended twin), rotation entries, as measured on one
# MI355X by test_hypotheses_match_the_extended_twin (it prints them); the bar is max(1e-15, twice the second figure).
HYP_MEASURED = {1: (4.017e-16, 4.017e-16), 2: (4.682e-16, 4.682e-16), 127: (1.838e-13, 1.838e-13), 1024: (9.649e-13, 9.649e-13),
                1 << 20: (1.480e-09, 1.480e-09)}    # translations: 2.2e-16 both, at every size; device - binary64 twin: 4.4e-16


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
    return fp.FindProbe(HOOKS) if IN_HOOKS_PROCESS else None


def _note(key, value):
    worst[key] = max(worst.get(key, 0.0), float(value))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _same_scores(a, b):
    """Bits where both are numbers, isnan where they are not."""
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(_bits(a[~na]), _bits(b[~nb]))


def _random_rotations(n, rng):
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return tw.quat_xyzw_to_matrix(q)


def _random_poses(n, rng):
    return np.concatenate([_random_rotations(n, rng), rng.uniform(-0.5, 0.5, (n, 3)) + [0.0, 0.0, 1.0]], axis=1)


# ---------------------------------------------------------------- the entry points themselves
def test_find_probes_refuse_bad_arguments(request, probe):
    """Null pointers and negative counts are RBS_ERR_INVALID_ARGUMENT, a count of zero is RBS_OK; neither touches an array."""
    if _delegated(request):
        return
    import ctypes as C
    lib = probe.lib
    assert all(hasattr(lib, s) for s in fp.FIND_SYMBOLS)
    i32, i64, f64, u64 = C.c_int32, C.c_int64, C.c_double, C.c_uint64
    d = fp.sentinel(64 * 12, np.float64)
    f = fp.sentinel(64, np.float32)
    i = fp.sentinel(128, np.int32)
    ll = np.zeros(64, dtype=np.int64)
    p = fp._p
    bad, ok = fp.RBS_ERR_INVALID_ARGUMENT, fp.RBS_OK
    assert lib.rbs_test_find_subsample(None, i32(4), i32(4), i32(1), p(f), i64(0)) == bad
    assert lib.rbs_test_find_subsample(p(f), i32(-1), i32(4), i32(1), p(f), i64(0)) == bad
    assert lib.rbs_test_find_subsample(p(f), i32(0), i32(4), i32(1), p(f), i64(0)) == ok
    assert lib.rbs_test_find_seeds(p(f), i32(4), i32(4), i32(1), f64(0.25), f64(3.0), i32(4), None, p(d), p(i), i64(0)) == bad
    assert lib.rbs_test_find_seeds(p(f), i32(4), i32(-4), i32(1), f64(0.25), f64(3.0), i32(4), p(i), p(d), p(i), i64(0)) == bad
    assert lib.rbs_test_find_seeds(p(f), i32(4), i32(0), i32(1), f64(0.25), f64(3.0), i32(4), p(i), p(d), p(i), i64(0)) == ok
    assert lib.rbs_test_find_hyp(p(d), i32(2), i32(4), f64(1), f64(1), f64(0), f64(0), f64(0), i64(0), None, i32(-1), p(d), i64(0)) == bad
    assert lib.rbs_test_find_hyp(p(d), i32(2), i32(4), f64(1), f64(1), f64(0), f64(0), f64(0), i64(7), None, i32(2), p(d), i64(0)) == bad   # past H
    assert lib.rbs_test_find_hyp(p(d), i32(2), i32(4), f64(1), f64(1), f64(0), f64(0), f64(0), i64(0), None, i32(0), p(d), i64(0)) == ok
    assert lib.rbs_test_find_topk(p(d), None, i64(-1), i32(4), p(d), p(ll), p(d), p(ll), i64(0), None) == bad
    assert lib.rbs_test_find_topk(p(d), None, i64(8), i32(4), None, p(ll), p(d), p(ll), i64(0), None) == bad
    assert lib.rbs_test_find_topk(p(d), None, i64(8), i32(1025), p(d), p(ll), p(d), p(ll), i64(0), None) == bad
    assert lib.rbs_test_find_topk(p(d), None, i64(0), i32(4), p(d), p(ll), p(d), p(ll), i64(0), None) == ok
    assert lib.rbs_test_find_nms(p(d), p(d), p(ll), i32(-2), f64(0.1), f64(0.1), i32(4), p(i), p(i), p(d), p(d), p(ll), i64(0)) == bad
    assert lib.rbs_test_find_nms(p(d), p(d), p(ll), i32(2), f64(0.1), f64(0.1), i32(65), p(i), p(i), p(d), p(d), p(ll), i64(0)) == bad
    assert lib.rbs_test_find_nms(p(d), p(d), p(ll), i32(0), f64(0.1), f64(0.1), i32(4), p(i), p(i), p(d), p(d), p(ll), i64(0)) == ok
    assert lib.rbs_test_find_children(p(d), i32(-1), i32(4), i32(0), u64(0), f64(0), f64(0), p(d), i64(0)) == bad
    assert lib.rbs_test_find_children(None, i32(1), i32(4), i32(0), u64(0), f64(0), f64(0), p(d), i64(0)) == bad
    assert lib.rbs_test_find_children(p(d), i32(0), i32(4), i32(0), u64(0), f64(0), f64(0), p(d), i64(0)) == ok
    assert lib.rbs_test_find_select(p(d), p(d), i32(-1), i32(4), p(d), p(d), i64(0)) == bad
    assert lib.rbs_test_find_select(p(d), p(d), i32(0), i32(4), p(d), p(d), i64(0)) == ok
    assert lib.rbs_test_find_order(p(d), p(d), p(ll), i32(-1), p(d), p(d), i64(0)) == bad
    assert lib.rbs_test_find_order(p(d), p(d), None, i32(2), p(d), p(d), i64(0)) == bad
    assert lib.rbs_test_find_order(p(d), p(d), p(ll), i32(0), p(d), p(d), i64(0)) == ok
    assert untouched(d) and untouched(f) and untouched(i) and not ll.any()


# ---------------------------------------------------------------- subsample, order
@pytest.mark.parametrize("cols,rows", [(7, 5), (322, 241), (64, 64)])
def test_subsample_is_exact(request, probe, cols, rows):
    if _delegated(request):
        return
    rng = np.random.default_rng([cols, rows])
    frame = rng.uniform(0.1, 4.0, rows * cols).astype(np.float32)
    frame[rng.random(frame.size) < 0.1] = np.nan
    for f in (1, 2, 4):
        ref, r, c = tw.subsample(frame, rows, cols, f)
        got = probe.subsample(frame, rows, cols, f)
        assert _same(got[: r * c], ref.ravel()) and untouched(got[r * c:]), (cols, rows, f)


@pytest.mark.parametrize("S", [1, 64])
def test_order_gathers_by_position(request, probe, S):
    if _delegated(request):
        return
    rng = np.random.default_rng(S)
    surv, score = _random_poses(S, rng), rng.normal(size=S)
    score[S // 2] = np.nan
    for order in (rng.permutation(S), np.arange(S)[::-1], np.zeros(S, dtype=np.int64)):
        pose, sc = probe.order(surv, score, order)
        assert _same(pose[:S], surv[order]) and _same_scores(sc[:S], score[order]), S
        assert untouched(pose[S:]) and untouched(sc[S:])


# ---------------------------------------------------------------- seeds
DMIN, DMAX = np.float32(0.25), np.float32(3.0)       # exactly representable
# (rows, cols, stride) -> cells; rows and cols are multiples of the stride only where the stride is 1
GRIDS = {1: (3, 2, 5), 63: (13, 17, 2), 64: (22, 23, 3), 65: (17, 50, 4), 1023: (31, 33, 1), 1024: (156, 158, 5), 1025: (49, 81, 2),
         2049: (7, 2047, 3), 3000: (197, 238, 4)}
INVALID = [np.nan, np.inf, -np.inf, 0.0, np.nextafter(DMIN, np.float32(0)), np.nextafter(DMAX, np.float32(4)), -1.0]
EDGE_VALID = [DMIN, DMAX, np.nextafter(DMIN, np.float32(1)), np.nextafter(DMAX, np.float32(0))]


def _validity(profile, ncell, rng):
    c = np.arange(ncell)
    return {"none": c < 0, "all": c >= 0, "first": c == 0, "last": c == ncell - 1, "every64": c % 64 == 0, "every65": c % 65 == 0,
            "half": rng.random(ncell) < 0.5}[profile]


@pytest.mark.parametrize("ncell", sorted(GRIDS))
def test_seeds_compact_and_thin_exactly(request, probe, ncell):
    """Every validity profile on a grid of `ncell` cells, the planted depths on both sides of each limit, every max_seeds
    around the valid count: seeds, both info words and the compacted cells are the twin's, the rest keeps its sentinel."""
    if _delegated(request):
        return
    rows, cols, stride = GRIDS[ncell]
    assert -(-rows // stride) * -(-cols // stride) == ncell
    rng = np.random.default_rng(ncell)
    gi, gj = np.meshgrid(np.arange(0, rows, stride), np.arange(0, cols, stride), indexing="ij")
    grid_px = (gi * cols + gj).ravel()
    for profile in ("none", "all", "first", "last", "every64", "every65", "half"):
        ok = _validity(profile, ncell, rng)
        frame = np.full(rows * cols, 1.5, dtype=np.float32)             # (off the grid: valid depths, never to be read)
        depth = rng.uniform(0.3, 2.9, ncell).astype(np.float32)
        nv = int(ok.sum())
        depth[np.flatnonzero(ok)[: len(EDGE_VALID)]] = EDGE_VALID[: min(nv, len(EDGE_VALID))]
        bad = np.resize(np.array(INVALID, dtype=np.float32), ncell)
        frame[grid_px] = np.where(ok, depth, bad)
        coarse = frame.reshape(rows, cols)
        all_cells = tw.seeds(coarse, stride, float(DMIN), float(DMAX), 1 << 30)[0][:, 3].astype(np.int32)
        assert len(all_cells) == nv, (profile, len(all_cells), nv)      # the planted depths fall on the side they were planted on
        for max_seeds in sorted({m for m in (1, nv - 1, nv, nv + 1, -(-nv // 2), 1 << 20) if m >= 1}):
            tag = (ncell, profile, max_seeds)
            ref, n = tw.seeds(coarse, stride, float(DMIN), float(DMAX), max_seeds)
            cells, seeds, info = probe.seeds(frame, rows, cols, stride, float(DMIN), float(DMAX), max_seeds)
            kept = len(ref)
            assert info[:2].tolist() == [kept, nv] and n == nv and untouched(info[2:]), (tag, info)
            assert _same(seeds[:kept], ref) and untouched(seeds[kept:]), tag
            assert np.array_equal(cells[:nv], all_cells) and untouched(cells[nv:]), (tag, np.flatnonzero(cells[:nv] != all_cells)[:8])


# ---------------------------------------------------------------- top-k
def _scores(profile, n, rng):
    if profile == "distinct":
        return rng.permutation(n).astype(np.float64) - n / 3.0
    if profile == "equal":
        return np.full(n, 2.5)
    if profile == "eight":
        return rng.choice(np.array([-np.inf, -3.0, -0.0, 0.0, 1.0, 1.0 + 2.0 ** -52, 7.0, np.inf]), n)
    if profile == "nan10":
        s = rng.normal(size=n)
        s[rng.random(n) < 0.1] = np.nan
        return s
    if profile == "allnan":
        return np.full(n, np.nan)
    if profile == "inf":
        s = rng.normal(size=n)
        s[rng.random(n) < 0.2] = np.inf
        s[rng.random(n) < 0.2] = -np.inf
        return s
    assert profile == "zeros"
    return rng.choice(np.array([-0.0, 0.0]), n)


def _index(mode, n, rng):
    if mode == "none":
        return None
    perm = rng.permutation(n).astype(np.int64)
    return perm if mode == "perm" else perm * 3 + (1 << 31)         # (at or above 2^31, distinct)


PROFILES = ("distinct", "equal", "eight", "nan10", "allnan", "inf", "zeros")
TOPK_SIZES = [1, 2, 1023, 1024, 1025, 2047, 2048, 2049, 4097, 3 * 2048 + 5]


def _check_topk(probe, n, combos, ks, rng):
    for profile, mode in combos:
        s, idx = _scores(profile, n, rng), _index(mode, n, rng)
        ref_s, ref_i = tw.topk(s, idx, max(ks))                     # one sort; a smaller k is its prefix (the order is total)
        for k in ks:
            got_s, got_i, tail_s, tail_i, passes = probe.topk(s, idx, k)
            tag = (n, k, profile, mode, passes)
            assert np.array_equal(got_i, ref_i[:k]), (tag, np.flatnonzero(got_i != ref_i[:k])[:8])
            assert _same_scores(got_s, ref_s[:k]), tag
            assert untouched(tail_s) and untouched(tail_i), tag
            if n > (1 << 21) and k >= 7:
                assert passes >= 3, tag


@pytest.mark.parametrize("n", TOPK_SIZES)
def test_topk_has_the_twin_order(request, probe, n):
    """Every score profile and index mode at chunk edges, k from 1 to 1 024 and, where n < 1 024, beyond n (the padding)."""
    if _delegated(request):
        return
    rng = np.random.default_rng(n)
    ks = sorted({1, 7, 64, 1024, min(n, 1024)} if n >= 1024 else {k for k in (1, 7, 64, 1024, n) if k <= n} | {min(n + 2, 1024), 64})
    _check_topk(probe, n, [(p, m) for p in PROFILES for m in ("none", "perm", "big")], ks, rng)


@pytest.mark.parametrize("profile, mode, ks", [("eight", "none", [1, 7, 64, 1024]), ("nan10", "big", [7, 1024]), ("distinct", "perm", [64])])
def test_topk_of_two_million_items_takes_three_passes(request, probe, profile, mode, ks):
    if _delegated(request):
        return
    _check_topk(probe, (1 << 21) + 1, [(profile, mode)], ks, np.random.default_rng(21))


# ---------------------------------------------------------------- the suppression and the keep kernel
def _identity_poses(translations):
    t = np.asarray(translations, dtype=np.float64)
    P = np.zeros((len(t), 12))
    P[:, [0, 4, 8]] = 1.0
    P[:, 9:] = t
    return P


def _check_nms(probe, poses, nms_t, nms_a, max_keep, scores=None, tag=None):
    n = len(poses)
    scores = -np.arange(n, dtype=np.float64) if scores is None else scores
    idx = (np.arange(n, dtype=np.int64) * 7 + (1 << 31))
    ref = tw.nms(poses, nms_t, nms_a, max_keep, scores)
    kept, count, surv, surv_score, surv_idx = probe.nms(poses, scores, idx, nms_t, nms_a, max_keep)
    m = len(ref)
    assert count[0] == m and kept[:m].tolist() == ref, (tag, count[0], kept[:m + 2], ref[:8])
    assert untouched(kept[m:]) and untouched(count[1:]), tag
    assert _same(surv[:m], poses[ref]) and _same(surv_score[:m], scores[ref]) and _same(surv_idx[:m], idx[ref]), tag
    assert untouched(surv[m:]) and untouched(surv_score[m:]) and untouched(surv_idx[m:]), tag
    return ref


def test_nms_at_its_thresholds(request, probe):
    """d2 == t2 exactly (binary fractions), one ulp inside and outside; the trace exactly at trace_min (identity rotations,
    nms_angle 0: 3.0) and nms_angle pi (-1.0); nms_translation 0 on duplicates; a first candidate that suppresses the rest."""
    if _delegated(request):
        return
    up, down = np.nextafter(0.25, 1.0), np.nextafter(0.25, 0.0)
    P = _identity_poses([[0, 0, 1], [0.25, 0, 1], [up, 0, 1], [down, 0, 1], [0, 0.25, 1]])
    for angle in (0.0, 0.3, math.pi):
        assert _check_nms(probe, P, 0.25, angle, 64, tag=("d2 == t2", angle)) == [0, 2]
    # the trace: identity against identity is 3.0 == 1 + 2 cos 0; a rotation by 1e-4 about z falls below it
    Q = _identity_poses([[0, 0, 1]] * 3)
    c, s = math.cos(1e-4), math.sin(1e-4)
    Q[2, :9] = [c, -s, 0, s, c, 0, 0, 0, 1]
    assert _check_nms(probe, Q, 0.25, 0.0, 64, tag="trace == trace_min") == [0, 2]
    assert _check_nms(probe, Q, 0.25, math.pi, 64, tag="angle pi") == [0]
    R = _identity_poses([[0, 0, 1]] * 2)
    R[1, :9] = [-1, 0, 0, 0, -1, 0, 0, 0, 1]                       # a half turn: trace -1.0 == 1 + 2 cos pi
    assert 1.0 + 2.0 * math.cos(math.pi) == -1.0
    assert _check_nms(probe, R, 0.25, math.pi, 64, tag="half turn") == [0]
    assert _check_nms(probe, R, 0.25, 3.0, 64, tag="half turn, below pi") == [0, 1]
    # nms_translation 0: only a duplicate is near
    D = _identity_poses([[0, 0, 1], [0, 0, 1], [2.0 ** -40, 0, 1], [0, 0, 1], [2.0 ** -40, 0, 1]])
    assert _check_nms(probe, D, 0.0, 0.5, 64, tag="duplicates") == [0, 2]
    # the first candidate suppresses all the others
    rng = np.random.default_rng(3)
    for n in (1, 2, 63, 64, 65, 1024):
        A = _identity_poses(rng.uniform(-0.1, 0.1, (n, 3)))
        A[0, 9:] = 0.0
        for max_keep in (1, 2, 63, 64):
            assert _check_nms(probe, A, 0.25, 0.5, max_keep, tag=("one keeps all", n, max_keep)) == [0]


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1024])
def test_nms_fills_every_lane_and_stops_at_nan(request, probe, n):
    """No suppression: lanes 0 .. max_keep - 2 all hold a kept pose when the last is accepted (n = 1 024, max_keep = 64: all 64
    lanes).  A NaN score at position 0, 1 and n - 1 ends the candidates there.  Random clusters against the twin."""
    if _delegated(request):
        return
    rng = np.random.default_rng(n)
    far = _identity_poses(np.stack([np.arange(n, dtype=np.float64), np.zeros(n), np.ones(n)], -1))
    for max_keep in (1, 2, 63, 64):
        assert _check_nms(probe, far, 0.25, 0.5, max_keep, tag=("far", n, max_keep)) == list(range(min(n, max_keep)))
        for pos in sorted({0, min(1, n - 1), n - 1}):
            scores = -np.arange(n, dtype=np.float64)
            scores[pos] = np.nan
            ref = _check_nms(probe, far, 0.25, 0.5, max_keep, scores, tag=("nan", n, max_keep, pos))
            assert ref == list(range(min(pos, max_keep)))
        # clusters: a few centres, members within and beyond the radius, rotations within and beyond the angle
        centres = rng.uniform(-0.3, 0.3, (max(1, n // 8), 3))
        member = rng.integers(0, len(centres), n)
        P = _random_poses(n, rng)
        P[:, 9:] = centres[member] + rng.normal(0.0, 0.01, (n, 3))
        base = _random_rotations(len(centres), rng).reshape(-1, 3, 3)
        small = np.stack([tw.rotvec_matrix(v) for v in rng.normal(0.0, 0.3, (n, 3))])
        P[:, :9] = (small @ base[member]).reshape(n, 9)
        for nms_t, nms_a in ((0.02, math.radians(30)), (0.01, math.radians(10)), (0.05, math.pi)):
            ref = _check_nms(probe, P, nms_t, nms_a, max_keep, tag=("clusters", n, max_keep, nms_t))
            _note("suppressed candidates in a cluster case", (ref[-1] + 1 - len(ref)) if ref else 0)


# ---------------------------------------------------------------- children
CHILD_SHAPES = [(S, c) for S in (1, 7, 64) for c in (1, 2, 63, 64, 65, 257)] + [(2, 4096)]
CHILD_BAR = 1e-14


def _sample_pairs(S, n_children, rng, m=24):
    edge = [(k, j) for k in {0, S - 1} for j in {0, 1, n_children - 1} if j < n_children]
    rand = [(int(rng.integers(S)), int(rng.integers(n_children))) for _ in range(m)]
    return sorted(set(edge + rand))


@pytest.mark.parametrize("rnd", [0, 1, 63])
@pytest.mark.parametrize("seed", [0, BIG_SEED, 2 ** 64 - 1], ids=["seed0", "seedmixed", "seedones"])
def test_children_draw_the_twin_normals(request, probe, seed, rnd):
    """Child 0 and, with both sigmas 0, every child: the survivor bit for bit.  sigma_angle 0, sigma_translation 1 on zero
    translations: the translation columns are the normals themselves -- the counter packing (round << 32 | k, j << 2 | pair) at
    k up to 63, j up to 4 095, round up to 63, under keys with either word set.  Then the general case."""
    if _delegated(request):
        return
    rng = np.random.default_rng([rnd, seed & 0xFFFF])
    for S, nc in CHILD_SHAPES:
        tag = (S, nc, rnd, hex(seed))
        surv = _random_poses(S, rng)
        m = S * nc
        out = probe.children(surv, nc, rnd, seed, 0.0, 0.0)
        assert untouched(out[m:]) and _same(out[:m].reshape(S, nc, 12), np.repeat(surv[:, None], nc, 1)), tag
        # the normals
        zero = surv.copy()
        zero[:, 9:] = 0.0
        out = probe.children(zero, nc, rnd, seed, 1.0, 0.0)
        got = out[:m].reshape(S, nc, 12)
        assert untouched(out[m:]) and _same(got[:, 0].copy(), zero) and _same(got[..., :9].copy(), np.repeat(zero[:, None, :9], nc, 1)), tag
        nz = tw.child_normals_array(seed, rnd, S, nc)
        if nc > 1:
            d = np.abs(got[:, 1:, 9:] - nz[:, 1:, 3:]).max()
            _note("normals, device - binary64 twin", d)
            assert d <= CHILD_BAR, (tag, d)
        pairs = [q for q in _sample_pairs(S, nc, rng) if q[1] > 0]
        for k, j in pairs:
            ext = tw.child_normals_ext(seed, rnd, k, j)
            d = float(np.abs(got[k, j, 9:] - ext[3:]).max())
            _note("normals, device - extended twin", d)
            _note("normals, binary64 twin - extended twin", np.abs(nz[k, j] - ext).max())
            assert d <= CHILD_BAR, (tag, k, j, d)
        # the general case
        st, sa = 0.01, math.radians(10.0)
        out = probe.children(surv, nc, rnd, seed, st, sa)
        got = out[:m].reshape(S, nc, 12)
        assert untouched(out[m:]) and _same(got[:, 0].copy(), surv), tag
        ref = tw.children_array(surv, nc, rnd, seed, st, sa)
        d = np.abs(got - ref).max()
        _note("children, device - binary64 twin", d)
        assert d <= CHILD_BAR, (tag, d)
        pairs = _sample_pairs(S, nc, rng, 12)
        ext = tw.children_ext(surv, nc, rnd, seed, st, sa, pairs)
        gsel = np.stack([got[k, j] for k, j in pairs])
        d = float(np.abs(gsel - ext).max())
        _note("children, device - extended twin", d)
        _note("children, binary64 twin - extended twin", np.abs(np.stack([ref[k, j] for k, j in pairs]) - ext).max())
        assert d <= CHILD_BAR, (tag, d)


# ---------------------------------------------------------------- select
def _child_scores(profile, S, nc, rng):
    s = rng.normal(size=(S, nc))
    if profile == "equal":
        s[:] = 1.5
    elif profile == "max first":
        s[:, 0] = 9.0
    elif profile == "max last":
        s[:, nc - 1] = 9.0
    elif profile == "max twice":
        s[:, rng.integers(0, nc, 2)] = 9.0
    elif profile == "nan first":
        s[:, 0] = np.nan
    elif profile == "all nan":
        s[:] = np.nan
    elif profile == "all -inf":
        s[:] = -np.inf
    elif profile == "nan then -inf":
        s[:] = -np.inf
        s[:, 0] = np.nan
    elif profile == "one +inf":
        s[np.arange(S), rng.integers(0, nc, S)] = np.inf
    elif profile == "nan mixed":
        s[rng.random((S, nc)) < 0.3] = np.nan
    return s


@pytest.mark.parametrize("nc", [1, 2, 64, 4096])
@pytest.mark.parametrize("S", [1, 63, 64])
def test_select_keeps_the_best_child(request, probe, S, nc):
    if _delegated(request):
        return
    rng = np.random.default_rng([S, nc])
    child = rng.normal(size=(S * nc, 12))
    for profile in ("random", "equal", "max first", "max last", "max twice", "nan first", "all nan", "all -inf", "nan then -inf",
                    "one +inf", "nan mixed"):
        s = _child_scores(profile, S, nc, rng)
        b = tw.best_child(s)
        if profile in ("equal", "all nan", "all -inf", "max first"):
            assert not b.any(), profile
        if profile == "nan then -inf" and nc > 1:
            assert np.all(b == 1), profile
        surv, score = probe.select(child, s.ravel(), S, nc)
        tag = (S, nc, profile)
        assert _same(surv[:S], child.reshape(S, nc, 12)[np.arange(S), b]), tag
        assert _same_scores(score[:S], s[np.arange(S), b]), tag
        assert untouched(surv[S:]) and untouched(score[S:]), tag


def test_a_survivor_whose_children_all_score_nan_stays_and_sorts_last(request, probe):
    """The decision of include/rbsensor_mi355x.h, step 6: such a survivor keeps child 0 -- itself -- with a NaN score, and the
    final sort puts it after every survivor that has a number, in survivor order."""
    if _delegated(request):
        return
    S, nc = 7, 5
    rng = np.random.default_rng(0)
    child = rng.normal(size=(S * nc, 12))
    s = rng.normal(size=(S, nc))
    s[2] = np.nan
    s[5] = np.nan
    surv, score = probe.select(child, s.ravel(), S, nc)
    assert np.isnan(score[[2, 5]]).all() and _same(surv[[2, 5]], child.reshape(S, nc, 12)[[2, 5], 0])
    top_s, top_i, _, _, _ = probe.topk(score[:S], None, S)
    order = tw.result_order(score[:S])
    assert np.array_equal(top_i, order) and order[-2:].tolist() == [2, 5] and not np.isnan(score[order[:-2]]).any()
    pose, sc = probe.order(surv[:S], score[:S], top_i)
    assert _same(pose[:S], surv[:S][order]) and np.isnan(sc[S - 2:S]).all() and np.all(np.diff(sc[:S - 2]) <= 0)


# ---------------------------------------------------------------- hypotheses
COLS, ROWS = 160, 120
KC = np.array([[285.15, 0.0, 79.5], [0.0, 285.15, 59.5], [0.0, 0.0, 1.0]])
N_SEEDS = 2048


def _seed_array(rng):
    u = rng.integers(0, COLS, N_SEEDS).astype(np.float64)
    v = rng.integers(0, ROWS, N_SEEDS).astype(np.float64)
    d = rng.uniform(0.25, 3.0, N_SEEDS).astype(np.float32).astype(np.float64)
    planted = [(KC[0, 2], KC[1, 2]), (0, 0), (COLS - 1, 0), (0, ROWS - 1), (COLS - 1, ROWS - 1)]
    for where in (0, N_SEEDS - len(planted)):                     # at both ends of the seed list
        for q, (pu, pv) in enumerate(planted):
            u[where + q], v[where + q] = pu, pv
    return np.stack([u, v, d, v * COLS + u], -1)


@pytest.mark.parametrize("n_rot", [1, 2, 127, 1024, 1 << 20])
def test_hypotheses_match_the_extended_twin(request, probe, n_rot):
    """rbs_find_hyp_kernel at launch sizes around one block of 256, from h0 = 0, 255 and (2^20 rotations) 2^31 - 300;
    rbs_find_gather_kernel at listed hypotheses from 0 to the last one (at 2^20 rotations: 2^31 - 1) with the hyp kernel's bits."""
    if _delegated(request):
        return
    rng = np.random.default_rng(n_rot)
    seeds = _seed_array(rng)
    H = N_SEEDS * n_rot
    offset = 0.0431
    starts = [0, 255] + ([(1 << 31) - 300] if n_rot == 1 << 20 else [])
    listed = {}
    for h0 in starts:
        full = probe.hyp(seeds, n_rot, KC, offset, h0=h0, n=257)
        assert untouched(full[257:])
        for n in (1, 255, 256):
            part = probe.hyp(seeds, n_rot, KC, offset, h0=h0, n=n)
            assert _same(part[:n], full[:n]) and untouched(part[n:]), (n_rot, h0, n)
        for i in range(257):
            listed[h0 + i] = full[i]
    idx = np.array(sorted(set(listed) | {0, H - 1, H - 2, H // 2} | set(int(h) for h in rng.integers(0, H, 64))), dtype=np.int64)
    if n_rot == 1 << 20:
        assert idx[-1] == (1 << 31) - 1 and (1 << 31) - 2 in idx
    rng.shuffle(idx)
    got = probe.hyp(seeds, n_rot, KC, offset, idx=idx)
    assert untouched(got[len(idx):])
    got = got[: len(idx)]
    mine = [q for q, h in enumerate(idx) if int(h) in listed]
    assert _same(got[mine], np.stack([listed[int(idx[q])] for q in mine])), n_rot         # gather == hyp, bit for bit
    again = probe.hyp(seeds, n_rot, KC, offset, idx=idx[:3])                              # (a launch of 3 of a block of 256)
    assert _same(again[:3], got[:3])
    ext = tw.hypotheses_ext(seeds, n_rot, KC, offset, idx)
    twin = tw.hypotheses(seeds, n_rot, KC, offset, idx)
    twin_R, twin_t = float(np.abs(twin[:, :9] - ext[:, :9]).max()), float(np.abs(twin[:, 9:] - ext[:, 9:]).max())
    dev_R, dev_t = float(np.abs(got[:, :9] - ext[:, :9]).max()), float(np.abs(got[:, 9:] - ext[:, 9:]).max())
    bar_R, bar_t = max(1e-15, 2.0 * twin_R), max(1e-15, 2.0 * twin_t)
    print(f"hypotheses, {n_rot} rotations: rotation entries device {dev_R:.3e}, binary64 twin {twin_R:.3e} (bar {bar_R:.3e}); "
          f"translations device {dev_t:.3e}, twin {twin_t:.3e} (bar {bar_t:.3e}); device - twin {np.abs(got - twin).max():.3e}")
    _note(f"hypotheses at {n_rot} rotations / their bar", max(dev_R / bar_R, dev_t / bar_t))
    assert dev_R <= bar_R and dev_t <= bar_t, (n_rot, dev_R, bar_R, dev_t, bar_t)


def test_report_the_largest_differences(request, probe):
    if _delegated(request):
        return
    for k, v in sorted(worst.items()):
        print(f"largest difference, {k}: {v:.3e}")
