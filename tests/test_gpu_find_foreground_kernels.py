"""The kernels of the object finder's step 1b, the foreground (rbs_findfg_*_kernel, dbot_ros_amd/csrc/rbsensor_find.hip) ON
THE DEVICE, one by one, on planted inputs, against the numpy twin tests/find_fg_twin.py.

The test build of the library (librbsensor_mi355x_hooks.so) has rbs_test_findfg_trials / _count / _best / _mask: one entry
point per launch helper, the helpers rbs_find_run itself calls; host arrays in and out, every output with a sentinel-filled
tail (tests/find_fg_probes.py).

Bar: EXACT.  The stage is binary64 with + - * / and comparisons only, and the library is built without contraction, so planes
are compared as bits, counts as integers, records as bits and seeding frames as bits (a kept pixel keeps its bits, NaN payload
included; a masked one is the quiet NaN 0x7FC00000).

The probes exist in the hooks build only, and two builds of the library do not share a process: outside a process that has
loaded the hooks build, the first test here re-runs this file once in a child with RBS_LIB_PATH set to it, and every test
reports its own outcome of that run."""
import ctypes as C
import os

import numpy as np
import pytest

import find_fg_probes as fp
import find_fg_twin as fg
import find_twin as tw
from dbot_ros_amd import _capi
from find_fg_probes import TAIL, untouched

pytestmark = pytest.mark.gpu

HOOKS = fp.hooks_path(_capi.LIB_PATH)
IN_HOOKS_PROCESS = os.path.abspath(_capi.LIB_PATH) == os.path.abspath(HOOKS)
_child = {}
DMIN, DMAX = 0.25, 3.0                          # (both float32 numbers: a depth can sit exactly on either)
MS, SF = 0.003, 0.0014247                       # the sensor's defaults
SEED = 0xC0FFEE1234ABCDEF
TRIALS = (1, 255, 256, 257, 4096)
F32 = np.float32


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
    return fp.ForegroundProbe(HOOKS) if IN_HOOKS_PROCESS else None


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _up(x):
    return np.nextafter(F32(x), F32(np.inf))


def _down(x):
    return np.nextafter(F32(x), F32(-np.inf))


def _scene_frame(rows, cols, seed):
    """A tilted background plane at ~1.5 m with a blob 0.6 m in front, noise and drop-outs, float32 [rows, cols]."""
    rng = np.random.default_rng(seed)
    cc, rr = np.meshgrid(np.arange(cols), np.arange(rows))
    z = 1.5 + 0.2 * (cc / cols - 0.5) + 0.1 * (rr / rows - 0.5)
    blob = (cc - 0.4 * cols) ** 2 + (rr - 0.55 * rows) ** 2 <= (0.12 * rows) ** 2
    z = np.where(blob, 0.9 - 0.0004 * (cc - 0.4 * cols), z)
    z = z + rng.normal(size=z.shape) * (MS + SF * z * z)
    z = z.astype(F32)
    z[rng.random(z.shape) < 0.05] = np.nan
    return z


def _frames():
    return {(1, 1): np.array([[0.8]], dtype=F32), (1, 3): np.array([[0.8, 0.9, 1.0]], dtype=F32), (5, 7): _scene_frame(5, 7, 1),
            (120, 160): _scene_frame(120, 160, 2)}


_twin_planes = {}


def _planes_of(shape):
    """The twin's planes of 4 096 trials on the frame of this shape, computed once (trial t does not depend on the count)."""
    if shape not in _twin_planes:
        _twin_planes[shape] = fg.trials(_frames()[shape], shape[0], shape[1], DMIN, DMAX, SEED, 4096)
    return _twin_planes[shape]


# ---------------------------------------------------------------- the entry points themselves
def test_foreground_probes_refuse_bad_arguments(request, probe):
    """Null pointers, negative counts and more than 4 096 trials are RBS_ERR_INVALID_ARGUMENT, an empty frame or no trial is
    RBS_OK; neither touches an array."""
    if _delegated(request):
        return
    lib = probe.lib
    assert all(hasattr(lib, s) for s in fp.FINDFG_SYMBOLS)
    i32, i64, f64, u64 = C.c_int32, C.c_int64, C.c_double, C.c_uint64
    d, f, i, p = fp.sentinel(64, np.float64), fp.sentinel(64, F32), fp.sentinel(64, np.int32), fp._p
    bad, ok = fp.RBS_ERR_INVALID_ARGUMENT, fp.RBS_OK
    tr = lambda fr, rows, cols, T, out, tail=0: lib.rbs_test_findfg_trials(fr, i32(rows), i32(cols), f64(DMIN), f64(DMAX), u64(1), i32(T), out, i64(tail))
    assert tr(None, 2, 2, 1, p(d)) == bad and tr(p(f), 2, 2, 1, None) == bad and tr(p(f), -1, 2, 1, p(d)) == bad
    assert tr(p(f), 2, 2, -1, p(d)) == bad and tr(p(f), 2, 2, 4097, p(d)) == bad and tr(p(f), 2, 2, 1, p(d), -1) == bad
    assert tr(p(f), 0, 2, 1, p(d)) == ok and tr(p(f), 2, 2, 0, p(d)) == ok
    ct = lambda fr, rows, pl, T, out: lib.rbs_test_findfg_count(fr, i32(rows), i32(2), f64(DMIN), f64(DMAX), f64(MS), f64(SF), pl, i32(T), f64(2), out, i64(0))
    assert ct(None, 2, p(d), 1, p(i)) == bad and ct(p(f), 2, None, 1, p(i)) == bad and ct(p(f), 2, p(d), 1, None) == bad
    assert ct(p(f), 2, p(d), 4097, p(i)) == bad and ct(p(f), 0, p(d), 1, p(i)) == ok
    bs = lambda pl, cn, T, out: lib.rbs_test_findfg_best(pl, cn, i32(T), f64(0.2), out, i64(0))
    assert bs(None, p(i), 1, p(d)) == bad and bs(p(d), None, 1, p(d)) == bad and bs(p(d), p(i), 1, None) == bad
    assert bs(p(d), p(i), -1, p(d)) == bad and bs(p(d), p(i), 0, p(d)) == ok
    mk = lambda fr, rows, rec, out: lib.rbs_test_findfg_mask(fr, i32(rows), i32(2), f64(MS), f64(SF), rec, f64(5), out, i64(0))
    f2 = fp.sentinel(64, F32)
    assert mk(None, 2, p(d), p(f2)) == bad and mk(p(f), 2, None, p(f2)) == bad and mk(p(f), 2, p(d), None) == bad and mk(p(f), 0, p(d), p(f2)) == ok
    assert untouched(d) and untouched(f) and untouched(i) and untouched(f2)


# ---------------------------------------------------------------- trials
@pytest.mark.parametrize("shape", [(1, 1), (1, 3), (5, 7), (120, 160)])
def test_trials_are_the_twins_bit_for_bit(request, probe, shape):
    if _delegated(request):
        return
    rows, cols = shape
    frame, want = _frames()[shape], _planes_of(shape)
    for T in TRIALS:
        got = probe.trials(frame, rows, cols, DMIN, DMAX, SEED, T)
        assert _same(got[:T], want[:T]), (shape, T)
        assert untouched(got[T:])
    if rows * cols <= 3:         # one to three pixels: a pixel repeats or the three lie in a row, so every trial is void
        assert np.all(want[:, 3] == 1.0) and not want[:, :3].any()
    else:
        assert 0 < (want[:, 3] == 0.0).sum() < 4096


def test_collinear_picks_and_exactly_three_valid_pixels(request, probe):
    if _delegated(request):
        return
    nan = F32(np.nan)
    # 3 x 3 with the diagonal valid: distinct valid pixels are always collinear
    diag = np.full((3, 3), nan, dtype=F32)
    diag[0, 0], diag[1, 1], diag[2, 2] = 0.5, 0.7, 0.9
    px = [fg.trial_pixels(SEED, t, 9) for t in range(4096)]
    assert any(sorted(p) == [0, 4, 8] for p in px)                      # three distinct valid pixels, D == 0
    got = probe.trials(diag, 3, 3, DMIN, DMAX, SEED, 4096)
    assert _same(got[:4096], fg.trials(diag, 3, 3, DMIN, DMAX, SEED, 4096)) and np.all(got[:4096, 3] == 1.0) and untouched(got[4096:])
    # 2 x 2 with exactly three valid pixels: a plane whenever the draw is those three
    three = np.array([[0.5, 0.625], [nan, 0.75]], dtype=F32)
    want = fg.trials(three, 2, 2, DMIN, DMAX, SEED, 4096)
    got = probe.trials(three, 2, 2, DMIN, DMAX, SEED, 4096)
    assert _same(got[:4096], want) and untouched(got[4096:])
    live = want[:, 3] == 0.0
    assert 100 < live.sum() < 1000 and all(sorted(fg.trial_pixels(SEED, t, 4)) == [0, 1, 3] for t in np.nonzero(live)[0])
    # ... and every such plane passes through the three pixels: 3 inliers of 3 valid, accepted
    cnt = probe.counts(three, 2, 2, DMIN, DMAX, MS, SF, want, 2.0)
    assert np.array_equal(cnt[:4097], fg.counts(three, 2, 2, DMIN, DMAX, MS, SF, want, 2.0)) and untouched(cnt[4097:])
    assert cnt[4096] == 3 and set(cnt[:4096][live]) == {3} and set(cnt[:4096][~live]) == {-1}
    rec = probe.best(want, cnt[:4097], 0.2)
    assert _same(rec[:8], fg.best(want, cnt[:4097], 0.2)) and rec[0] == 1.0 and rec[6] == np.nonzero(live)[0][0] and untouched(rec[8:])


def test_frames_of_nan_inf_and_zero(request, probe):
    if _delegated(request):
        return
    rows, cols = 5, 7
    vals = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0], dtype=F32)
    frame = vals[np.arange(rows * cols) % 5].reshape(rows, cols).copy()
    frame.view(np.uint32)[0, 0] = 0x7FC00001                            # NaN with a payload
    frame.view(np.uint32)[0, 5] = 0xFFC00000                            # -NaN
    for T in (1, 257):
        planes = probe.trials(frame, rows, cols, DMIN, DMAX, SEED, T)
        assert np.all(planes[:T, 3] == 1.0) and not planes[:T, :3].any() and untouched(planes[T:])
        cnt = probe.counts(frame, rows, cols, DMIN, DMAX, MS, SF, planes[:T], 2.0)
        assert cnt[:T + 1].tolist() == [-1] * T + [0] and untouched(cnt[T + 1:])
        rec = probe.best(planes[:T], cnt[:T + 1], 0.2)
        assert rec[:8].tolist() == [0.0, 0.0, 0.0, 0.0, -1.0, 0.0, 0.0, 0.0] and untouched(rec[8:])
        out = probe.mask(frame, rows, cols, MS, SF, rec, 5.0)
        assert _same(out[:rows * cols], frame.ravel()) and untouched(out[rows * cols:])      # nothing accepted: every bit as it was
    # an accepted plane at 1 m: NaN (any payload), +inf stay or become NaN, -inf and 0 are "in front"
    rec = np.array([1.0, 0.0, 0.0, 1.0, 10.0, 20.0, 0.0, 0.0])
    out = probe.mask(frame, rows, cols, MS, SF, rec, 5.0)
    want = fg.mask(frame, rows, cols, MS, SF, rec, 5.0)
    assert _same(out[:rows * cols], want) and untouched(out[rows * cols:])
    o = out[:rows * cols].reshape(rows, cols)
    assert o.view(np.uint32)[0, 0] == 0x7FC00000 and np.isnan(o[0, 1]) and o[0, 2] == -np.inf and _bits(o[0, 3:5]).tolist() == [0, 0x80000000]


def test_depths_at_the_limits_and_one_float_either_side(request, probe):
    if _delegated(request):
        return
    edge = np.array([_down(DMIN), DMIN, _up(DMIN), _down(DMAX), DMAX, _up(DMAX)], dtype=F32)
    ok = [False, True, True, True, True, False]
    assert fg.valid(edge, DMIN, DMAX).tolist() == ok
    cnt = probe.counts(edge, 1, 6, DMIN, DMAX, MS, SF, np.zeros((0, 4)), 2.0)
    assert cnt[0] == 4 and untouched(cnt[1:])
    # 2 x 2 frames of three pixels on the limits and one just outside: the trials that draw the outsider are void
    for outsider, inside in ((_down(DMIN), DMIN), (_up(DMAX), DMAX)):
        frame = np.array([[inside, 1.0], [outsider, inside]], dtype=F32)
        want = fg.trials(frame, 2, 2, DMIN, DMAX, SEED, 256)
        got = probe.trials(frame, 2, 2, DMIN, DMAX, SEED, 256)
        assert _same(got[:256], want) and untouched(got[256:])
        live = np.nonzero(want[:, 3] == 0.0)[0]
        assert len(live) > 5 and all(2 not in fg.trial_pixels(SEED, t, 4) for t in live)
        n = probe.counts(frame, 2, 2, DMIN, DMAX, MS, SF, want, 2.0)
        assert np.array_equal(n[:257], fg.counts(frame, 2, 2, DMIN, DMAX, MS, SF, want, 2.0)) and n[256] == 3 and untouched(n[257:])


# ---------------------------------------------------------------- counts
@pytest.mark.parametrize("shape, T", [((1, 1), 1), ((1, 3), 257), ((5, 7), 4096), ((5, 7), 255), ((120, 160), 256), ((120, 160), 257)])
def test_counts_are_the_twins(request, probe, shape, T):
    if _delegated(request):
        return
    rows, cols = shape
    frame, planes = _frames()[shape], _planes_of(shape)[:T]
    got = probe.counts(frame, rows, cols, DMIN, DMAX, MS, SF, planes, 2.0)
    want = fg.counts(frame, rows, cols, DMIN, DMAX, MS, SF, planes, 2.0)
    assert np.array_equal(got[:T + 1], want) and untouched(got[T + 1:])
    assert got[T] == fg.valid(frame, DMIN, DMAX).sum()
    if shape == (120, 160):
        assert got[:T].max() > 0.5 * got[T]                                # some trial found the background plane


def test_a_steep_plane_whose_w_crosses_zero_inside_the_image(request, probe):
    if _delegated(request):
        return
    rows, cols = 6, 160
    a, b, c = -0.01, 0.002, 0.8                                           # w = 0 near u = 80
    w = fg._w(a, b, c, rows, cols).reshape(rows, cols)
    assert (w > 0).any() and (w < 0).any()
    with np.errstate(all="ignore"):
        frame = np.where((w > 1 / DMAX) & (w < 1 / DMIN), 1.0 / w, 1.0).astype(F32)
    frame[:, ::7] -= F32(0.05)                                           # some pixels in front
    planes = np.array([[a, b, c, 0.0], [a, -b, c, 0.0], [0.0, 0.0, -1.0, 0.0]])      # the last: w < 0 everywhere
    got = probe.counts(frame, rows, cols, DMIN, DMAX, MS, SF, planes, 2.0)
    want = fg.counts(frame, rows, cols, DMIN, DMAX, MS, SF, planes, 2.0)
    assert np.array_equal(got[:4], want) and untouched(got[4:]) and want[0] > 100 and want[2] == 0
    for pl in planes:
        rec = np.array([1.0, pl[0], pl[1], pl[2], 200.0, 960.0, 0.0, 0.0])
        out = probe.mask(frame, rows, cols, MS, SF, rec, 5.0)
        assert _same(out[:rows * cols], fg.mask(frame, rows, cols, MS, SF, rec, 5.0)) and untouched(out[rows * cols:])
    behind = fg._w(a, b, c, rows, cols) <= 0.0
    out = probe.mask(frame, rows, cols, MS, SF, np.array([1.0, a, b, c, 200.0, 960.0, 0.0, 0.0]), 5.0)[:rows * cols]
    assert behind.sum() > 300 and _same(out[behind], frame.ravel()[behind])                 # kept where the plane is behind the camera
    assert np.isnan(out[~behind]).sum() > 100 and (~np.isnan(out[~behind])).sum() > 30


def test_residuals_on_both_thresholds_and_one_float_either_side(request, probe):
    """sigma_factor 0 and model_sigma 2^-8: with the plane z = 1 both thresholds are float32 numbers."""
    if _delegated(request):
        return
    ms, rs, mk = 2.0 ** -8, 2.0, 5.0
    lo, hi, front = F32(1.0 - rs * ms), F32(1.0 + rs * ms), F32(1.0 - mk * ms)
    assert float(lo) == 1.0 - rs * ms and float(hi) == 1.0 + rs * ms and float(front) == 1.0 - mk * ms
    frame = np.array([[_down(lo), lo, _up(lo), 1.0, _down(hi), hi, _up(hi), _down(front), front, _up(front)]], dtype=F32)
    plane = np.array([[0.0, 0.0, 1.0, 0.0]])
    cnt = probe.counts(frame, 1, 10, DMIN, DMAX, ms, 0.0, plane, rs)
    assert cnt[:2].tolist() == [5, 10] and untouched(cnt[2:])             # lo, lo+, 1, hi-, hi: |d - z| <= 2 sigma includes equality
    assert np.array_equal(cnt[:2], fg.counts(frame, 1, 10, DMIN, DMAX, ms, 0.0, plane, rs))
    for k, want_in in enumerate([0, 1, 1, 1, 1, 1, 0, 0, 0, 0]):
        one = probe.counts(frame[:, k:k + 1], 1, 1, DMIN, DMAX, ms, 0.0, plane, rs)
        assert one[:2].tolist() == [want_in, 1], k
    rec = np.array([1.0, 0.0, 0.0, 1.0, 5.0, 10.0, 0.0, 0.0])
    out = probe.mask(frame, 1, 10, ms, 0.0, rec, mk)
    assert _same(out[:10], fg.mask(frame, 1, 10, ms, 0.0, rec, mk)) and untouched(out[10:])
    # strictly in front only: front - one float stays; front itself (z - d == 5 sigma) and everything behind it goes
    assert (~np.isnan(out[:10])).tolist() == [False] * 7 + [True, False, False] and _same(out[7:8], frame[0, 7:8])


# ---------------------------------------------------------------- the choice
def test_equal_counts_go_to_the_lowest_trial(request, probe):
    if _delegated(request):
        return
    for T, ties, winner in ((257, (256, 0), 0), (257, (129, 65), 65), (257, (70, 3, 200), 3), (4096, (4095, 64), 64), (255, (254,), 254),
                            (1, (0,), 0)):
        planes = np.zeros((T, 4))
        planes[:, 0] = np.arange(T) + 0.5
        cnt = np.full(T + 1, 7, dtype=np.int32)
        cnt[list(ties)] = 40
        cnt[::9][1:] = -1                                                    # void trials in between (never a tied one)
        cnt[list(ties)] = 40
        cnt[T] = 100
        rec = probe.best(planes, cnt, 0.2)
        assert _same(rec[:8], fg.best(planes, cnt, 0.2)) and untouched(rec[8:])
        assert rec[:8].tolist() == [1.0, winner + 0.5, 0.0, 0.0, 40.0, 100.0, float(winner), 0.0], (T, ties)


def test_acceptance_at_the_fraction_and_one_below(request, probe):
    if _delegated(request):
        return
    planes = np.array([[0.001, 0.002, 0.7, 0.0], [0.0, 0.0, 0.9, 0.0]])
    for cnt, frac, accepted in (([9, 4, 36], 0.25, 1.0), ([8, 4, 36], 0.25, 0.0), ([9, 4, 37], 0.25, 0.0), ([2, 1, 4], 0.25, 0.0),
                                ([3, 1, 4], 0.25, 1.0), ([3, -1, 3], 1.0, 1.0), ([-1, -1, 0], 0.0, 0.0), ([40, 41, 205], 0.2, 1.0),
                                ([40, 40, 201], 0.2, 0.0)):
        cnt = np.array(cnt, dtype=np.int32)
        rec = probe.best(planes, cnt, frac)
        assert _same(rec[:8], fg.best(planes, cnt, frac)) and rec[0] == accepted and untouched(rec[8:]), (cnt, frac)


# ---------------------------------------------------------------- the chain
@pytest.mark.parametrize("shape, T", [((5, 7), 257), ((120, 160), 256)])
def test_the_four_kernels_in_a_row_are_the_twins_foreground(request, probe, shape, T):
    if _delegated(request):
        return
    rows, cols = shape
    frame = _frames()[shape]
    planes = probe.trials(frame, rows, cols, DMIN, DMAX, SEED, T)[:T]
    cnt = probe.counts(frame, rows, cols, DMIN, DMAX, MS, SF, planes, 2.0)[:T + 1]
    rec = probe.best(planes, cnt, 0.2)[:8]
    out = probe.mask(frame, rows, cols, MS, SF, rec, 5.0)
    after = probe.counts(out[:rows * cols], rows, cols, DMIN, DMAX, MS, SF, np.zeros((0, 4)), 2.0)
    wrec, wout = fg.foreground(frame, rows, cols, DMIN, DMAX, MS, SF, SEED, plane_trials=T)
    rec[7] = rec[5] - after[0]
    assert _same(rec, wrec) and _same(out[:rows * cols], wout.ravel()) and untouched(out[rows * cols:]) and untouched(after[1:])
    if shape == (120, 160):
        valid = fg.valid(frame, DMIN, DMAX)
        cc, rr = np.meshgrid(np.arange(cols), np.arange(rows))
        blob = ((cc - 0.4 * cols) ** 2 + (rr - 0.55 * rows) ** 2 <= (0.12 * rows) ** 2).ravel()
        kept = fg.valid(out[:rows * cols], DMIN, DMAX)
        assert rec[0] == 1.0 and (kept & ~blob).sum() <= 0.001 * (valid & ~blob).sum() and (kept & blob).sum() >= 0.95 * (valid & blob).sum()
