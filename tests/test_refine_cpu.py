"""CPU-side checks of the pose refiner (rbs_refine_*, include/rbsensor_mi355x.h): the numpy twin
(tests/refine_twin.py) held to its own conditions on planted planes and on the oracle's renders, its chain on the scenes
of tests/assess_scenes.py against its own stored figures, what the library answers without a device, and the Python and
yaml plumbing with a faked refiner."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import assess_scenes as asc
import refine_twin as rt
from dbot_ros_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# a noise model and a camera whose values are exact in binary; a plane tilted in x and y that fills a 14 x 12 image
MS, SF = 2.0 ** -8, 2.0 ** -10
COLS, ROWS = 14, 12
CAM = (64.0, 64.0, 6.5, 5.5)
INF = np.float32(np.inf)


def planted():
    xs, ys = np.meshgrid(np.arange(COLS), np.arange(ROWS))
    d = (1.0 + xs / 256.0 + ys / 512.0).astype(np.float32)
    frame = (d + np.float32(2.0 ** -9)).astype(np.float32)            # 0.4 sigma behind the plane everywhere
    return d.reshape(1, -1).copy(), frame.reshape(-1).copy()


def sums_of(planes, frame, b=0, t=(0.0, 0.0, 1.0), **p):
    pixel, T, det = rt.terms(planes, frame, t, b, CAM, MS, SF, ROWS, COLS, **p)
    S, E, N = rt.exact_sums(T)
    return pixel, S.astype(np.float64), N, det


def at(x, y):
    return y * COLS + x


# ---------------------------------------------------------------------------------------------- the twin, planted inputs
def test_the_border_is_skipped_and_every_decision_has_a_margin():
    planes, frame = planted()
    pixel, S, N, det = sums_of(planes, frame)
    assert N == (COLS - 2) * (ROWS - 2)
    assert set(pixel // COLS) == set(range(1, ROWS - 1)) and set(pixel % COLS) == set(range(1, COLS - 1))
    # no planted decision sits near a rounding: gate and Huber margins of whole sigmas, normals of length far from 0
    assert det["gate_margin"].min() > 9.0 * det["sigma"].min() and det["huber_margin"].min() > 2.0 * det["sigma"].min()
    assert det["quad"].all() and det["flip"].all() and det["s"].min() > 1e-6 and np.abs(det["facing"]).min() > 1e-6
    assert (S[[0, 6, 11, 15, 18, 20, 27]] > 0).all()


def test_the_gate_drops_a_pixel():
    planes, frame = planted()
    _, base, N, _ = sums_of(planes, frame)
    frame[at(5, 5)] = planes[0, at(5, 5)] + np.float32(0.0625)          # 12.7 sigma: outside the gate of 10
    _, S, n, det = sums_of(planes, frame)
    assert n == N - 1 and not np.array_equal(S, base)
    ae, gs = det["ae"][5, 5], det["gs"][5, 5]
    assert ae - gs > 2.0 * (gs / 10.0) and not det["use"][5, 5]           # 2 sigma past the gate
    _, wide, n2, _ = sums_of(planes, frame, gate_sigmas=20.0)
    assert n2 == N and not np.array_equal(wide, S)


def test_the_huber_branch_weighs_a_pixel_down():
    planes, frame = planted()
    frame[at(5, 5)] = planes[0, at(5, 5)] + np.float32(0.0234375)         # 4.8 sigma: inside the gate, past huber_sigmas = 3
    _, S, N, det = sums_of(planes, frame)
    assert det["use"][5, 5] and det["ae"][5, 5] - det["hs"][5, 5] > det["hs"][5, 5] / 3.0      # a whole sigma past the bend
    assert (~det["quad"]).sum() == 1
    _, quad, n2, det2 = sums_of(planes, frame, huber_sigmas=6.0)
    assert n2 == N and det2["quad"].all() and not np.array_equal(S, quad)
    assert S[27] < quad[27] and S[20] < quad[20]                          # q and H_55 = sum w n2 n2 both lose weight


def test_the_neighbour_rule_and_the_owner_rule():
    planes, frame = planted()
    _, base, N, _ = sums_of(planes, frame)
    holed = planes.copy()
    holed[0, at(7, 6)] = INF                                              # a hole: the pixel and its four neighbours go
    pixel, S, n, _ = sums_of(holed, frame)
    assert n == N - 5 and not np.array_equal(S, base)
    assert not set(pixel) & {at(7, 6), at(6, 6), at(8, 6), at(7, 5), at(7, 7)}
    two = np.concatenate([planes, np.full_like(planes, INF)])
    two[1, at(3, 3)] = np.float32(0.5)                                    # a second body in front at one pixel owns it
    pixel, S2, n, _ = sums_of(two, frame, b=0)
    assert n == N - 5 and not set(pixel) & {at(3, 3), at(2, 3), at(4, 3), at(3, 2), at(3, 4)}
    assert sums_of(two, frame, b=1)[2] == 0                               # ... and a lone pixel has no neighbours of its own
    tie = np.concatenate([planes, planes])                                # a tie stays with the lowest body
    assert sums_of(tie, frame, b=0)[2] == N and sums_of(tie, frame, b=1)[2] == 0
    edge = planes.copy()
    edge[0, at(0, 4)] = INF                                               # a hole in the skipped border costs its one inner neighbour
    assert sums_of(edge, frame)[2] == N - 1


def test_the_sign_flip_is_taken_on_the_unnormalised_normal_and_changes_no_sum():
    """Two facts the rule's step 3 rests on, and why no input can make the flip change a sum.
    (1) With rho(x +- 1) = rho +- e_x / fx and rho(y +- 1) = rho +- e_y / fy,  (a x c) . m = D (D_r + D_l) (D_d + D_u) / (fx fy):
    positive for every surface in front of the camera, so on rendered planes the flip is always taken and n faces the camera.
    Only depths of mixed or negative sign leave it out -- planted here as a plane BEHIND the camera, which the rasterizer
    never draws -- with a margin on both sides.
    (2) Every term is even in n: w J J^T, w J r and w r r each hold n twice, and a negation is exact.  The flip decides the
    direction of n and no bit of any sum; the terms with every normal negated by hand are asserted equal, term by term."""
    planes, frame = planted()
    _, _, _, det = sums_of(planes, frame)
    assert det["flip"].all() and det["facing"].min() > 1e-6 and (det["n"][:, 2] < -0.9).all()   # in front: flipped, n towards the camera
    behind = (-planes).astype(np.float32)
    fr = (behind[0] + np.float32(2.0 ** -9)).astype(np.float32)
    pixel, S, N, det = sums_of(behind, fr, t=(0.0, 0.0, -1.0))
    assert N == (COLS - 2) * (ROWS - 2) and not det["flip"].any() and det["facing"].max() < -1e-6   # behind: not flipped
    _, T, _ = rt.terms(behind, fr, (0.0, 0.0, -1.0), 0, CAM, MS, SF, ROWS, COLS)
    xs, ys = np.meshgrid(np.arange(COLS, dtype=np.float64), np.arange(ROWS, dtype=np.float64))
    D = behind[0].astype(np.float64)
    m = np.stack([(D * ((xs.ravel() - CAM[2]) / CAM[0]))[pixel], (D * ((ys.ravel() - CAM[3]) / CAM[1]))[pixel], D[pixel]], axis=1)
    q = m - np.array([0.0, 0.0, -1.0])
    n, w, r = det["n"], det["w"], det["r"]
    for sign in (1.0, -1.0):
        nn, rr = sign * n, sign * r
        J = np.concatenate([np.stack([q[:, 1] * nn[:, 2] - q[:, 2] * nn[:, 1], q[:, 2] * nn[:, 0] - q[:, 0] * nn[:, 2],
                                      q[:, 0] * nn[:, 1] - q[:, 1] * nn[:, 0]], axis=1), nn], axis=1)
        cols = [(w * J[:, i]) * J[:, j] for i in range(6) for j in range(i, 6)] + [(w * J[:, i]) * rr for i in range(6)] + [(w * rr) * rr]
        assert np.array_equal(np.stack(cols, axis=1), T), sign


def test_the_kernels_summation_order_stays_inside_the_bar():
    rng = np.random.default_rng(2)
    planes, frame = planted()
    frame = (frame + rng.normal(0.0, 0.004, frame.shape).astype(np.float32)).astype(np.float32)
    pixel, T, _ = rt.terms(planes, frame, (0.0, 0.0, 1.0), 0, CAM, MS, SF, ROWS, COLS)
    exact, E, N = rt.exact_sums(T)
    got = rt.kernel_order_sums(pixel, T, (0, 0, COLS, ROWS), COLS)
    assert N > 100 and (np.abs(got.astype(rt.LD) - exact) <= E).all()
    big = np.tile(T, (40, 1))                                            # several parts: 40 x 168 px = 6 720 px -> 7 parts
    px = np.arange(big.shape[0]) + 200
    exact, E, _ = rt.exact_sums(big)
    assert rt.parts_of(100 * 100) == 10 and rt.parts_of(0) == 0 and rt.parts_of(1) == 1 and rt.parts_of(10 ** 6) == 16
    got = rt.kernel_order_sums(px, big, (0, 0, 100, 100), 100)
    assert (np.abs(got.astype(rt.LD) - exact) <= E).all()


def test_the_solve_in_the_devices_order():
    rng = np.random.default_rng(3)
    J = rng.normal(size=(200, 6))
    r = rng.normal(size=200) * 1e-3
    H = J.T @ J
    S = np.array([H[i, j] for i in range(6) for j in range(i, 6)] + list(J.T @ r) + [float(r @ r)])
    status, d = rt.solve(S, 200, damping=0.0, max_rotation=10.0, max_translation=10.0, eps_rotation=0.0, eps_translation=0.0)
    assert status == rt.MAX_ITERATIONS and np.allclose(d, np.linalg.solve(H, J.T @ r), rtol=1e-9, atol=0)
    status, d2 = rt.solve(S, 200, damping=1e-3, max_rotation=10.0, max_translation=10.0, eps_rotation=1.0, eps_translation=1.0)
    assert status == rt.CONVERGED and np.allclose(d2, np.linalg.solve(H + 1e-3 * np.diag(np.diag(H)), J.T @ r), rtol=1e-9, atol=0)
    assert rt.solve(S, 15) == (rt.TOO_FEW_PIXELS, [0.0] * 6) and rt.solve(S, 16)[0] != rt.TOO_FEW_PIXELS
    big = S.copy()
    big[21:27] *= 1e6
    status, d3 = rt.solve(big, 200)
    assert status == rt.MAX_ITERATIONS and abs(np.linalg.norm(d3[:3]) - 0.2) < 1e-15 and abs(np.linalg.norm(d3[3:]) - 0.02) < 1e-16
    flat = S.copy()
    flat[11] = 0.0                                                        # H_22 = 0: the third pivot is not > 0
    assert rt.solve(flat, 200, damping=0.0)[0] == rt.DEGENERATE and rt.solve(flat, 200)[0] == rt.DEGENERATE
    nan = S.copy()
    nan[0] = np.nan
    assert rt.solve(nan, 200)[0] == rt.DEGENERATE
    assert np.array_equal(rt.apply(np.arange(12.0), [0.0] * 6), np.arange(12.0))


# ---------------------------------------------------------------------------------------------- the twin on the oracle's renders
@pytest.fixture(scope="module")
def scenes():
    out = {}
    for name in ("m1m2_161", "m1m2m3_322", "m1_640"):
        meshes, cols, rows = asc.SCENES[name]
        out[name] = asc.Scene(meshes, cols, rows)
    yield out
    for s in out.values():
        s.close()


def cam_of(s):
    K = s.cam.camera_matrix
    return (K[0, 0], K[1, 1], K[0, 2], K[1, 2])


@pytest.mark.parametrize("name", ["m1m2_161", "m1m2m3_322"])
def test_a_noise_free_frame_at_the_pose_itself_and_2_mm_beside_it(scenes, name):
    """At the pose itself every e is 0 exactly: every term, hence every bar E, g and delta are 0 -- the bodies are CONVERGED
    in one iteration.  2 mm along each axis is recovered to 0.012 mm / 0.22 deg at worst (measured with this twin on the two
    scenes); asserted: 0.02 mm and 0.25 deg."""
    s = scenes[name]
    clean = s.planes(s.truth).min(axis=0)
    clean = np.where(np.isfinite(clean), clean, np.float32(np.nan)).astype(np.float32)
    for b, r in enumerate(rt.iteration(s.planes(s.truth), clean, s.truth, cam_of(s), s.ms, s.sf, s.rows, s.cols)):
        assert r["count"] > 100 and r["status"] == rt.CONVERGED
        assert (np.abs(r["S"][21:27].astype(rt.LD)) <= r["E"][21:27]).all() and not r["E"][21:28].any()
        assert not np.abs(r["delta"]).any() and np.array_equal(r["pose"], s.truth[b])
    worst = [0.0, 0.0]
    for axis in range(3):
        dt = [0.0, 0.0, 0.0]
        dt[axis] = 0.002
        pose, rec, _ = rt.chain(s.planes, clean, rt.offset_pose(s.truth, dt, 0.0), cam_of(s), s.ms, s.sf, s.rows, s.cols)
        for b in range(s.B):
            et, er = rt.pose_errors(pose[b], s.truth[b])
            print(name, "axis", axis, "body", b, rec[b]["status"], rec[b]["iterations"], "%.4f mm %.4f deg" % (et * 1e3, er))
            assert rec[b]["status"] == rt.CONVERGED and rec[b]["iterations"] <= 4
            worst = [max(worst[0], et), max(worst[1], er)]
    assert worst[0] <= 0.02e-3 and worst[1] <= 0.25, worst


STARTS = (((0.005, -0.005, 0.005), 5.0), ((0.01, 0.01, -0.01), 10.0), ((0.02, 0.0, 0.02), 20.0))
# the twin's own figures, ten iterations from each start: per body (status, iterations, count first, count last, mm, degrees)
CHAINS = {
    "m1m2m3_322": [[(1, 5, 832, 907, 0.599, 2.020), (1, 5, 732, 794, 0.218, 0.654), (2, 10, 7, 7, 8.660, 5.000)],
                   [(1, 10, 751, 907, 0.598, 2.014), (1, 8, 651, 794, 0.224, 0.655), (2, 10, 0, 0, 17.321, 10.000)],
                   [(1, 10, 625, 907, 0.598, 2.014), (0, 10, 572, 796, 0.167, 0.551), (2, 10, 0, 0, 28.284, 20.000)]],
    "m1_640": [[(1, 4, 2504, 2837, 0.236, 1.116)], [(1, 7, 2139, 2836, 0.233, 1.111)], [(1, 7, 1781, 2835, 0.231, 1.109)]],
}


@pytest.mark.parametrize("name", list(CHAINS))
def test_the_chain_from_the_issues_starts(scenes, name):
    """Noisy frames with a slab occluder and 5 % NaN (tests/assess_scenes.py).  The figures are this twin's, stored to the
    digits printed; half a unit of the last digit is the tolerance (counts, statuses and iterations: exact)."""
    s = scenes[name]
    for (dt, deg), want in zip(STARTS, CHAINS[name]):
        pose, rec, _ = rt.chain(s.planes, s.frame, rt.offset_pose(s.truth, dt, deg), cam_of(s), s.ms, s.sf, s.rows, s.cols)
        for b in range(s.B):
            et, er = rt.pose_errors(pose[b], s.truth[b])
            got = (rec[b]["status"], rec[b]["iterations"], rec[b]["count_first"], rec[b]["count_last"])
            print(name, dt, deg, "body", b, got, "%.3f mm %.3f deg" % (et * 1e3, er))
            assert got == want[b][:4], (dt, deg, b)
            assert abs(et * 1e3 - want[b][4]) <= 0.00051 and abs(er - want[b][5]) <= 0.00051, (dt, deg, b, et * 1e3, er)


# ---------------------------------------------------------------------------------------------- the library, no device
def test_symbols_layouts_and_defaults():
    text = open(os.path.join(ROOT, "include", "rbsensor_mi355x.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = C.CDLL(_capi.LIB_PATH)
    names = ("rbs_refine_default_params", "rbs_refine_check_params", "rbs_refine_poses", "rbs_refine_get_history", "rbs_refine_kernel_ms")
    for s in names:
        assert re.search(r"\b" + s + r"\s*\(", code) and s in _capi.EXPORTS and hasattr(lib, s), s
    assert sorted(set(re.findall(r"\b(rbs_refine_[a-z0-9_]+)\s*\(", code))) == sorted(names)
    for k, name in enumerate(("RBS_REFINE_MAX_ITERATIONS", "RBS_REFINE_CONVERGED", "RBS_REFINE_TOO_FEW_PIXELS", "RBS_REFINE_DEGENERATE", "RBS_REFINE_FROZEN")):
        assert re.search(name + r"\s*=\s*%d\b" % k, code) and getattr(_capi, name) == k
    assert (rt.MAX_ITERATIONS, rt.CONVERGED, rt.TOO_FEW_PIXELS, rt.DEGENERATE, rt.FROZEN) == tuple(range(5))
    assert re.search(r"#define\s+RBS_REFINE_MAX_ITERS\s+32\b", code) and _capi.RBS_REFINE_MAX_ITERS == 32
    assert C.sizeof(_capi.RbsRefineParams) == 64 and _capi.RbsRefineParams.min_pixels.offset == 56
    assert C.sizeof(_capi.RbsRefineBody) == 32 and _capi.RbsRefineBody.rms_first.offset == 16
    assert C.sizeof(_capi.RbsRefineHistory) == 376 and _capi.RbsRefineHistory.sums.offset == 96 and _capi.RbsRefineHistory.count.offset == 368
    src = open(os.path.join(ROOT, "dbot_ros_amd", "csrc", "rbsensor_refine.hip")).read()
    assert re.findall(r"__global__[^\n]*?void\s+(\w+)\s*\(", src) == ["rbs_refine_accumulate_kernel", "rbs_refine_solve_kernel"]
    assert "atomicAdd" not in src                                          # fixed order: no atomics, floating-point or other
    d = _capi.RbsRefineParams()
    _capi.load().rbs_refine_default_params(C.byref(d))
    got = {f: getattr(d, f) for f in rt.DEFAULTS}
    assert got == rt.DEFAULTS
    assert "unmeasured starting value" in text[text.index("typedef struct rbs_refine_params"):text.index("} rbs_refine_params;")]
    from dbot_ros_amd.refine import PoseRefiner
    p = PoseRefiner.Parameters()
    assert {f: getattr(p, f) for f in rt.DEFAULTS} == rt.DEFAULTS
    c = p.c_params()
    assert {f: getattr(c, f) for f in rt.DEFAULTS} == rt.DEFAULTS
    assert (rt.PARTS, rt.PART_PX) == tuple(int(re.search(r"constexpr int %s = (\d+);" % k, src).group(1)) for k in ("kRefineParts", "kRefinePartPx"))


def test_every_refusal_comes_before_a_device_is_touched():
    lib = _capi.load()
    inv = _capi.RBS_ERR_INVALID_ARGUMENT
    poses = np.zeros(12)
    dp = poses.ctypes.data_as(C.POINTER(C.c_double))
    rec = (_capi.RbsRefineBody * 1)()
    assert lib.rbs_refine_poses(None, None, None, dp, 1, dp, rec) == inv
    assert lib.rbs_refine_get_history(None, 0, 0, 0, C.byref(_capi.RbsRefineHistory())) == inv
    assert lib.rbs_refine_kernel_ms(None, (C.c_float * 3)()) == inv
    lib.rbs_refine_default_params(None)   # no-op
    assert lib.rbs_refine_check_params(None) == _capi.RBS_OK
    nan, inf = float("nan"), float("inf")
    bad = (("gate_sigmas", (0.0, -1.0, nan, inf)), ("huber_sigmas", (0.0, -1.0, nan, inf)), ("damping", (-1e-12, nan, inf)),
           ("max_rotation", (0.0, -0.1, nan, inf)), ("max_translation", (0.0, -0.1, nan, inf)), ("eps_rotation", (-1e-12, nan, inf)),
           ("eps_translation", (-1e-12, nan, inf)), ("min_pixels", (0, -5)), ("iters", (0, -1, 33, 1000)))
    for key, values in bad:
        for v in values:
            p = _capi.RbsRefineParams()
            lib.rbs_refine_default_params(C.byref(p))
            assert lib.rbs_refine_check_params(C.byref(p)) == _capi.RBS_OK
            setattr(p, key, v)
            assert lib.rbs_refine_check_params(C.byref(p)) == inv, (key, v)
    for key, v in (("damping", 0.0), ("eps_rotation", 0.0), ("eps_translation", 0.0), ("iters", 1), ("iters", 32), ("min_pixels", 1)):
        p = _capi.RbsRefineParams()
        lib.rbs_refine_default_params(C.byref(p))
        setattr(p, key, v)
        assert lib.rbs_refine_check_params(C.byref(p)) == _capi.RBS_OK, (key, v)


# ---------------------------------------------------------------------------------------------- plumbing, a faked refiner
class FakeTracker:
    """What state_poses / Rt_to_state read of a tracker, with ParticleTracker's own state-to-model rule."""

    def __init__(self, parts=2, center=True):
        from types import SimpleNamespace
        self.parts = parts
        self.centers = np.array([[0.01, -0.02, 0.03], [0.0, 0.05, -0.01]])[:parts]
        self.params = SimpleNamespace(center_object_frame=center)
        self.initialized = None

    def _to_model(self, state):
        from dbot_ros_amd.tracker import ParticleTracker
        return ParticleTracker._to_model(self, state)

    def _from_model(self, state):
        from dbot_ros_amd.tracker import ParticleTracker
        return ParticleTracker._from_model(self, state)


def test_a_pose_goes_to_a_state_and_back():
    from dbot_ros_amd.assess import state_poses
    from dbot_ros_amd.pose import Rt_to_state
    rng = np.random.default_rng(1)
    for center in (True, False):
        tr = FakeTracker(2, center)
        state = rng.normal(size=24) * 0.3
        back = Rt_to_state(tr, state_poses(tr, state)[0])
        s, b = state.reshape(2, 12), back.reshape(2, 12)
        np.testing.assert_allclose(b[:, :6], s[:, :6], rtol=0, atol=1e-14)
        assert not b[:, 6:].any()                                          # velocities: zero
        np.testing.assert_allclose(state_poses(tr, back), state_poses(tr, state), rtol=0, atol=1e-14)


class FakeRefiner:
    """Moves every state 1 mm in x; records what it was asked."""

    def __init__(self):
        self.asked = []

    def refine_state(self, tracker, state, frame=None):
        self.asked.append((np.array(state), frame))
        out = np.array(state, dtype=np.float64)
        out[0] += 0.001
        return out, "record"


def test_the_supervisor_hands_the_refined_state_to_the_assessor_and_the_tracker():
    from types import SimpleNamespace
    from dbot_ros_amd.assess import LOST, SUPPORTED
    from dbot_ros_amd.supervisor import TrackSupervisor

    class Tracker:
        parts = 1

        def __init__(self):
            self.started = []

        def track(self, frame):
            return np.zeros(12)

        def initialize(self, states):
            self.started.append(np.array(states[0]))

    class Assessor:
        def __init__(self):
            self.judged = []

        def assess_state(self, tracker, state, frame=None):
            self.judged.append(np.array(state))
            found = state[1] == 7.0                                          # the finder's states carry a 7
            return SimpleNamespace(verdicts=np.array([[SUPPORTED if found else LOST]]), contour_verdicts=None)

    found = np.zeros(12)
    found[1] = 7.0
    for refiner in (None, FakeRefiner()):
        tr, a = Tracker(), Assessor()
        sup = TrackSupervisor(tr, a, find=lambda fr: found.copy(), lost_frames=2, refine=refiner)
        events = [sup.step("frame %d" % k)[2] for k in range(3)]
        assert events == [None, "lost", "reacquired"]
        want = found.copy()
        if refiner is not None:
            want[0] += 0.001
            assert len(refiner.asked) == 1 and refiner.asked[0][1] == "frame 2" and np.array_equal(refiner.asked[0][0], found)
            assert sup.last_refinement == "record"
        else:
            assert sup.last_refinement is None
        assert np.array_equal(a.judged[-1], want) and np.array_equal(tr.started[-1], want)


def test_yaml_keys():
    from dbot_ros_amd import node
    from dbot_ros_amd.finder import ObjectFinder
    from dbot_ros_amd.refine import PoseRefiner
    sensor = object()
    r = node.build_pose_refiner({"pose_refiner": {"iters": 4, "damping": 0, "min_pixels": "32"}}, sensor)
    assert isinstance(r, PoseRefiner) and r.sensor is sensor
    assert (r.params.iters, r.params.damping, r.params.min_pixels, r.params.gate_sigmas) == (4, 0.0, 32, 10.0)
    assert {f: getattr(node.build_pose_refiner({}, sensor).params, f) for f in rt.DEFAULTS} == rt.DEFAULTS
    with pytest.raises(ValueError, match="pose_refiner/iter"):
        node.build_pose_refiner({"pose_refiner": {"iter": 4}}, sensor)
    assert ObjectFinder.Parameters.from_rosparam({"object_finder": {"refine": True, "rounds": 4}}).refine is True
    assert ObjectFinder.Parameters.from_rosparam({"object_finder": {"rounds": 4}}).refine is False
    assert node._finder_refines({"object_finder": {"refine": True}}) and not node._finder_refines({}) and not node._finder_refines({"object_finder": None})


def test_the_supervisor_with_several_bodies_moves_the_searched_ones_only():
    """find_bodies and refine together: every body goes through the refiner (it moves a pose as a whole), the searched body
    takes its refined pose, the other keeps the state find_bodies returned bit for bit; the assessor judges and the
    tracker restarts from that mix."""
    from types import SimpleNamespace
    from dbot_ros_amd.assess import LOST, SUPPORTED
    from dbot_ros_amd.supervisor import TrackSupervisor

    class Tracker:
        parts = 2

        def __init__(self):
            self.started = []

        def track(self, frame):
            return np.zeros(24)

        def initialize(self, states):
            self.started.append(np.array(states[0]))

    class Assessor:
        def __init__(self):
            self.judged = []

        def assess_state(self, tracker, state, frame=None):
            self.judged.append(np.array(state))
            found = state[13] == 7.0                                        # find_bodies' states carry a 7 in body 1, which must not move
            return SimpleNamespace(verdicts=np.array([[LOST if not found else SUPPORTED, SUPPORTED]]), contour_verdicts=None)

    class MovesAll:
        def refine_state(self, tracker, state, frame=None):
            return np.array(state, dtype=np.float64) + 0.001, "record"

    found = np.arange(24.0)
    found[13] = 7.0
    asked = []

    def find_bodies(frame, lost, estimate):
        asked.append(lost.copy())
        return found.copy()

    tr, a = Tracker(), Assessor()
    sup = TrackSupervisor(tr, a, find_bodies=find_bodies, lost_frames=2, refine=MovesAll())
    events = [sup.step(k)[2] for k in range(3)]
    assert events == [None, "lost", "reacquired"] and asked[0].tolist() == [True, False]
    want = found.copy()
    want[:12] += 0.001                                                    # body 0 was lost and searched: refined; body 1: as found
    assert np.array_equal(a.judged[-1], want) and np.array_equal(tr.started[-1], want)
    assert sup.last_refinement == "record"


def test_the_supervised_replay_knows_the_refine_key():
    from dbot_ros_amd import node
    with pytest.raises(ValueError, match=r"supervisor/lost: unknown key .*'refine'\]"):
        node.replay_dataset_supervised({"supervisor": {"refine": True, "lost": 3}}, None, "")
    import inspect
    from dbot_ros_amd.supervisor import TrackSupervisor
    assert inspect.signature(node.replay_dataset_supervised).parameters["refine"].default is None
    assert inspect.signature(TrackSupervisor.__init__).parameters["refine"].default is None
