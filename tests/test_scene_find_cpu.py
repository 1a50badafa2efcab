"""The scene finder without a GPU (rbs_find_scene_*, dbot_ros_amd/finder.py SceneFinder): the numpy
twin against itself on planted planes and frames, S1's order, the polish's Philox counters, the supervisor's find_bodies,
the rosparam mapping, the exported C-ABI and its parameter checks, the compiler's report for the new kernels, the C++
mirror, and the whole scene find in the twin with the oracle's scores on the scenes the GPU tests use."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import find_twin as tw
import scene_find_scenes as ss
import scene_find_twin as st
from dbot_ros_amd import _capi
from dbot_ros_amd.assess import Assessment, LOST, OCCLUDED, SUPPORTED
from dbot_ros_amd.finder import ObjectFinder, SceneFinder
from dbot_ros_amd.supervisor import TrackSupervisor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
MS, SF = 0.003, 0.0014247
NAN_BITS = 0x7FC00000


def tau(d, sigmas=3.0):
    return sigmas * (MS + SF * (d * d))


def planted(rows=12, cols=16, bg=2.0):
    """One placed body: a 2 x 2 patch at depth 1 in rows 5..6, columns 7..8; the frame shows it in front of a wall."""
    plane = np.full((rows, cols), np.inf, dtype=np.float32)
    plane[5:7, 7:9] = 1.0
    frame = np.full((rows, cols), bg, dtype=np.float32)
    frame[5:7, 7:9] = 1.0
    return plane, frame


def res(planes, placed, frame, radius, sigmas=3.0):
    rows, cols = frame.shape
    planes = np.stack([np.asarray(p, dtype=np.float32).reshape(-1) for p in planes])
    return st.residual(planes, placed, frame.ravel(), rows, cols, MS, SF, sigmas, radius).reshape(rows, cols)


def test_rule_a_alone_at_radius_zero():
    plane, frame = planted()
    frame[5, 8] = 1.0 + 0.9 * tau(1.0)      # inside tau: support
    frame[6, 7] = 1.0 + 1.1 * tau(1.0)      # behind: owned, not support
    frame[6, 8] = 1.0 - 1.1 * tau(1.0)      # in front: owned, not support
    r = res([plane], [0], frame, 0)
    ex = st.bits(r) == NAN_BITS
    assert ex[5, 7] and ex[5, 8] and not ex[6, 7] and not ex[6, 8] and ex.sum() == 2
    assert np.array_equal(st.bits(r)[~ex], st.bits(frame)[~ex])


def test_rule_b_at_the_windows_edge_and_corner():
    plane, frame = planted()
    # pixels that read the body's depth outside its render: at Chebyshev distance 2 (edge, corner) and 3
    for (y, x) in ((5, 10), (3, 5), (8, 10), (5, 11), (2, 7), (3, 4)):
        frame[y, x] = 1.0
    r2 = st.bits(res([plane], [0], frame, 2)) == NAN_BITS
    assert r2[5, 10] and r2[3, 5] and r2[8, 10]          # |dx| = 2; (-2, -2) of (5, 7); (+2, +2) of (6, 8)
    assert not r2[5, 11] and not r2[2, 7] and not r2[3, 4]
    assert r2.sum() == 4 + 3
    r3 = st.bits(res([plane], [0], frame, 3)) == NAN_BITS
    assert r3[5, 11] and r3[2, 7] and r3[3, 4] and r3.sum() == 4 + 6
    r0 = st.bits(res([plane], [0], frame, 0)) == NAN_BITS
    assert r0.sum() == 4
    # the neighbour's own test: a reading within tau of d(j) is explained, one outside is not
    frame[5, 10] = 1.0 + 0.99 * tau(1.0)
    frame[3, 5] = 1.0 + 1.01 * tau(1.0)
    frame[8, 10] = 1.0 - 1.01 * tau(1.0)
    r2 = st.bits(res([plane], [0], frame, 2)) == NAN_BITS
    assert r2[5, 10] and not r2[3, 5] and not r2[8, 10]
    # a wall pixel beside the body is not explained: it reads 1 m behind
    assert not r2[5, 6]


def test_the_window_is_clipped_at_the_image_border():
    rows, cols = 6, 7
    plane = np.full((rows, cols), np.inf, dtype=np.float32)
    plane[0, 0] = plane[rows - 1, cols - 1] = 1.0
    frame = np.full((rows, cols), 1.0, dtype=np.float32)     # everything reads the bodies' depth
    ex = st.bits(res([plane], [0], frame, 2)) == NAN_BITS
    want = np.zeros((rows, cols), dtype=bool)
    want[:3, :3] = True
    want[-3:, -3:] = True
    assert np.array_equal(ex, want)
    ex8 = st.bits(res([plane], [0], frame, 8)) == NAN_BITS   # a window larger than the image
    assert ex8.all()


def test_a_pixel_owned_but_in_front_is_explained_by_a_neighbour():
    plane, frame = planted()
    plane[5, 8] = 1.2                                        # the render lies 20 cm behind what the sensor reads there
    assert 1.0 - 1.2 < -tau(1.2)
    r0 = st.bits(res([plane], [0], frame, 0)) == NAN_BITS
    assert not r0[5, 8] and r0.sum() == 3                    # owned, in_front: rule (a) leaves it
    r1 = st.bits(res([plane], [0], frame, 1)) == NAN_BITS
    assert r1[5, 8] and r1.sum() == 4                        # its neighbour (5, 7) is support at depth 1


def test_ties_of_owner_and_the_placed_bodies_only():
    plane, frame = planted()
    near = plane.copy()
    near[5, 7] = 0.5                                         # body 1 is nearer at (5, 7): it owns the pixel and reads in_front... of nothing
    same = plane.copy()
    # a tie: both bodies at depth 1 everywhere -> the owner is the lowest, and the class is the same
    a = res([plane, same], [0, 1], frame, 0)
    b = res([plane], [0], frame, 0)
    assert np.array_equal(st.bits(a), st.bits(b))
    # body 1 nearer at (5, 7): the frame's 1.0 lies behind 0.5 -> not support, and radius 0 leaves the pixel
    c = st.bits(res([plane, near], [0, 1], frame, 0)) == NAN_BITS
    assert not c[5, 7] and c.sum() == 3
    # ... but body 1 not placed: it does not own anything
    d = st.bits(res([plane, near], [0], frame, 0)) == NAN_BITS
    assert d[5, 7] and d.sum() == 4
    owner, depth = st.at.owners(np.stack([plane.ravel(), same.ravel()]))
    assert set(owner[owner >= 0].tolist()) == {0}


def test_frame_nan_and_infinities_keep_their_bits():
    plane, frame = planted()
    fb = st.bits(frame).copy()
    fb[0, 0] = 0x7FC00001        # a NaN with a payload, outside the body
    fb[5, 7] = 0xFFC12345        # a negative NaN with a payload, on the body
    fb[5, 8] = 0x7F800000        # +inf on the body
    fb[6, 7] = 0xFF800000        # -inf on the body
    fb[5, 9] = 0x7F800000        # +inf beside the body: not finite, rule (b) does not apply
    frame = fb.view(np.float32)
    r = st.bits(res([plane], [0], frame, 2))
    for (y, x) in ((0, 0), (5, 7), (5, 8), (6, 7), (5, 9)):
        assert r[y, x] == fb[y, x], (y, x)
    assert r[6, 8] == NAN_BITS and (r == NAN_BITS).sum() == 1


def test_no_placed_body_gives_the_frames_bits():
    plane, frame = planted()
    fb = st.bits(frame).copy()
    fb[1, 1] = 0x7FC00001
    frame = fb.view(np.float32)
    assert np.array_equal(st.bits(res([plane], [], frame, 2)), fb)
    empty = np.full_like(plane, np.inf)
    assert np.array_equal(st.bits(res([empty], [0], frame, 2)), fb)       # placed, but it covers nothing


def test_order_and_a_tie():
    assert st.order([0.04, 0.05, 0.03], 0b111) == [1, 0, 2]
    assert st.order([0.04, 0.05, 0.03], 0b101) == [0, 2]
    assert st.order([0.04, 0.04, 0.05, 0.04], 0b1011) == [0, 1, 3]        # ties to the lower b
    rng = np.random.default_rng(0)
    V = rng.normal(size=(500, 3)) * 0.05 + 0.3
    assert abs(st.mean_vertex_distance(V) - tw.depth_offset(V)) <= 1e-15
    s = ss.Scene(("m1", "m2", "m1"), 80, 60, 0)
    assert s.e[0] == s.e[2] != s.e[1]
    assert st.order(s.e, 0b111) == ([0, 2, 1] if s.e[0] > s.e[1] else [1, 0, 2])


def test_polish_counters_are_disjoint_from_step_6_and_step_1b():
    B = 16
    polish = set()
    for r in range(64 * B + 1):
        for c in (0, B - 1):
            hi, lo = st.polish_counter(r, c, 1, 0)
            assert (hi >> 32) == 0x10000 + r and (hi & 0xFFFFFFFF) == c
            polish.add(hi >> 32)
    step6 = set(range(65))                      # step 6: the counter's last word is a round <= 64
    assert not (polish & step6) and 0xFFFFFFFF not in polish and max(polish) < 0xFFFFFFFF
    # the normals are step 6's function of that counter, and differ from step 6's own
    nz = tw.child_normals(7, 0x10000 + 3, 1, 2)
    X = np.tile(np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0.1, 0, 1.0]), (3, 1))
    ch = st.polish_children(X, 1, 4, 3, 7, 0.005, 0.1)
    assert ch.shape == (4, 3, 12)
    np.testing.assert_array_equal(ch[0], X)
    np.testing.assert_array_equal(ch[:, [0, 2]], np.repeat(X[None, [0, 2]], 4, 0))
    np.testing.assert_allclose(ch[2, 1, 9:], X[1, 9:] + 0.005 * nz[3:], rtol=0, atol=1e-16)
    assert not np.allclose(nz, tw.child_normals(7, 3, 1, 2))
    assert st.polish_scales(st.DEFAULTS, 2, 0) == st.polish_scales(st.DEFAULTS, 2, 1) == (0.005, math.radians(5.0))
    assert st.polish_scales(st.DEFAULTS, 2, 2) == (0.005 * 0.6, math.radians(5.0) * 0.6)


def test_polish_keeps_the_best_child_and_never_goes_down():
    X = np.tile(np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0.0, 0, 1.0]), (2, 1))
    target = np.array([[0.01, 0.0, 1.0], [-0.01, 0.0, 1.0]])

    def score(poses):
        return -np.sum((poses[:, :, 9:] - target) ** 2, axis=(1, 2))

    Xn, s, rounds = st.polish(X, [1, 0], score, 5, polish_sweeps=3, polish_children=16)
    best = [float(cs[b]) for _, cs, b in rounds]
    assert len(rounds) == 6 and all(b >= a for a, b in zip(best, best[1:])) and s == best[-1] > float(score(X[None])[0])
    assert all(np.array_equal(ch[0], prev) for (ch, _, _), prev in zip(rounds[1:], [r[0][r[2]] for r in rounds]))
    _, s0, r0 = st.polish(X, [1, 0], score, 5, polish_sweeps=0)
    assert r0 == [] and s0 == float(score(X[None])[0])
    nan_first = lambda poses: np.where(np.arange(len(poses)) == 0, np.nan, 1.0)       # NaN never beats a number; ties to the lowest j
    assert st.polish(X, [0], nan_first, 5, polish_sweeps=1, polish_children=4)[2][0][2] == 1


# ---------------------------------------------------------------- the supervisor's find_bodies
class FakeTracker:
    def __init__(self, parts):
        self.parts = parts
        self.initialized = []
        self._in_flight = 0

    def track(self, frame):
        return np.full(self.parts * 12, float(frame))

    def initialize(self, states):
        self.initialized.append(np.array(states[0]))


class FakeAssessor:
    def __init__(self, script, found=None):
        self.script, self.found = script, found or {}

    def assess_state(self, tracker, state, frame):
        is_found = float(np.asarray(state).reshape(-1)[0]) >= 1000.0
        v = np.atleast_1d(np.array(self.found[frame] if is_found else self.script[frame], dtype=np.int32))
        return Assessment(np.zeros((1, v.size, 5), dtype=np.int32), v[None])


S, L, O = SUPPORTED, LOST, OCCLUDED


def test_find_bodies_searches_only_the_lost_bodies_and_confirms_only_them():
    calls = []

    def find_bodies(frame, lost, estimate):
        calls.append((frame, lost.tolist(), estimate.copy()))
        return None if frame == 2 else np.full(36, 1000.0 + frame)

    script = [[S, S, S], [S, L, S], [S, L, S], [O, L, S], [S, L, S], [S, L, L]] + [[S, S, S]] * 2
    # frame 4: body 1 found and SUPPORTED while body 0 (not searched) reads OCCLUDED in the found state: confirmed all the same
    asr = FakeAssessor(script, found={3: [S, L, S], 4: [O, S, L]})
    trk = FakeTracker(3)
    sup = TrackSupervisor(trk, asr, find_bodies=find_bodies, lost_frames=1)
    out = [sup.step(k) for k in range(6)]
    assert [o[2] for o in out] == [None, "lost", "find_failed", "find_failed", "reacquired", "lost"]   # (frame 5: a new run begins)
    assert [c[0] for c in calls] == [2, 3, 4]
    assert all(c[1] == [False, True, False] for c in calls)              # only the body that reads LOST
    assert all((c[2] == float(c[0])).all() and c[2].shape == (36,) for c in calls)   # the others' estimates go with it
    assert len(trk.initialized) == 1 and (trk.initialized[0] == 1004.0).all() and (out[4][0] == 1004.0).all()
    assert sup.lost_run == 1
    # occluded for too long counts as lost for that body too
    calls.clear()
    sup = TrackSupervisor(FakeTracker(2), FakeAssessor([[S, O]] * 4 + [[L, O]], found={3: [S, S], 4: [S, S]}), find_bodies=find_bodies,
                          lost_frames=1, occluded_frames=1)
    assert [sup.step(k)[2] for k in range(4)] == [None, "lost", "find_failed", "reacquired"]
    assert [c[1] for c in calls] == [[False, True], [False, True]]


def test_find_keeps_its_one_object_refusal_beside_find_bodies():
    with pytest.raises(ValueError, match="one object"):
        TrackSupervisor(FakeTracker(2), FakeAssessor([]), find=lambda f: None)
    with pytest.raises(ValueError, match="alternatives"):
        TrackSupervisor(FakeTracker(1), FakeAssessor([]), find=lambda f: None, find_bodies=lambda f, m, e: None)
    TrackSupervisor(FakeTracker(2), FakeAssessor([]), find_bodies=lambda f, m, e: None)
    sup = TrackSupervisor(FakeTracker(1), FakeAssessor([[L]] * 3, found={1: [S]}), find_bodies=lambda f, m, e: np.full(12, 1000.0 + f), lost_frames=1)
    assert [sup.step(k)[2] for k in range(2)] == ["lost", "reacquired"]      # any number of parts, one included


# ---------------------------------------------------------------- parameters, exports, kernels
def test_scene_mapping_and_unknown_keys():
    p = ObjectFinder.Parameters.from_rosparam({"object_finder": {"n_rotations": 64, "scene": {"explain_radius": 4, "polish_sigma_angle_deg": 2,
                                                                                            "polish_sweeps": 0, "explain_sigmas": 2.5}}})
    assert p.n_rotations == 64 and isinstance(p.scene, SceneFinder.Parameters)
    assert p.scene.explain_radius == 4 and p.scene.polish_sweeps == 0 and p.scene.explain_sigmas == 2.5
    assert p.scene.polish_sigma_angle == pytest.approx(math.radians(2)) and p.scene.polish_children == 64
    assert ObjectFinder.Parameters.from_rosparam({}).scene is None
    assert SceneFinder.Parameters.from_mapping(None) == SceneFinder.Parameters()
    with pytest.raises(ValueError, match="object_finder/scene/explain_radiu"):
        ObjectFinder.Parameters.from_rosparam({"object_finder": {"scene": {"explain_radiu": 1}}})
    from dbot_ros_amd import node
    assert callable(node.build_scene_finder)


def test_exports_defaults_and_parameter_checks_without_a_device():
    lib = _capi.load()
    for s in ("rbs_find_scene_create", "rbs_find_scene_run", "rbs_find_scene_get_residual", "rbs_find_scene_body_finder", "rbs_find_scene_destroy"):
        assert s in _capi.EXPORTS and hasattr(lib, s)
    assert C.sizeof(_capi.RbsFindSceneParams) == 48 and _capi.RbsFindSceneParams.polish_sigma_translation.offset == 24
    sp = _capi.RbsFindSceneParams()
    lib.rbs_find_scene_default_params(C.byref(sp))
    d = SceneFinder.Parameters()
    for f in sp._fields_:
        if f[0] != "reserved":
            assert getattr(sp, f[0]) == pytest.approx(getattr(d, f[0])), f[0]
    assert all(st.DEFAULTS[k] == pytest.approx(getattr(sp, k)) for k in st.DEFAULTS) and len(st.DEFAULTS) == len(sp._fields_) - 1
    fp = _capi.RbsFindParams()
    lib.rbs_find_default_params(C.byref(fp))
    out = C.c_void_p()
    for field, bad, message in (("explain_sigmas", 0.0, "find_scene: explain_sigmas must be finite and > 0"),
                                ("explain_radius", 9, "find_scene: explain_radius outside 0..8"),
                                ("explain_radius", -1, "find_scene: explain_radius outside 0..8"),
                                ("polish_sweeps", -1, "find_scene: polish_sweeps outside 0..8"),
                                ("polish_children", 0, "find_scene: polish_children outside 1..1024"),
                                ("polish_sigma_angle", float("nan"), "find_scene: polish_sigma_translation and polish_sigma_angle must be finite and >= 0"),
                                ("polish_decay", 1.5, "find_scene: polish_decay outside (0, 1]")):
        q = _capi.RbsFindSceneParams()
        lib.rbs_find_scene_default_params(C.byref(q))
        setattr(q, field, bad)
        assert lib.rbs_find_scene_create(None, C.byref(fp), C.byref(q), C.byref(out)) == _capi.RBS_ERR_INVALID_ARGUMENT
        assert lib.rbs_last_error(None).decode() == message, field
    fp.n_candidates = 2000          # the finder's own checks come first
    assert lib.rbs_find_scene_create(None, C.byref(fp), None, C.byref(out)) == _capi.RBS_ERR_INVALID_ARGUMENT
    assert lib.rbs_last_error(None).decode() == "find: n_candidates outside 1..1024"
    assert not out.value
    assert lib.rbs_find_scene_run(None, None, 1, None, None, None, None, None) == _capi.RBS_ERR_INVALID_ARGUMENT
    assert not lib.rbs_find_scene_body_finder(None, 0)
    assert lib.rbs_find_scene_last_error(None) == b"null scene finder"
    lib.rbs_find_scene_destroy(None)


def test_scene_finder_kernels_do_not_spill():
    txt = open(os.path.join(ROOT, "dbot_ros_amd", "lib", "resource_usage.txt")).read()
    seen = {}
    for b in re.split(r"remark: Function Name: ", txt)[1:]:
        m = re.search(r"rbs_finds_(\w+?)_kernel", b.split()[0])
        if not m:
            continue
        assert re.search(r"ScratchSize \[bytes/lane\]: 0\b", b), m.group(1)
        assert re.search(r"SGPRs Spill: 0\b", b) and re.search(r"VGPRs Spill: 0\b", b), m.group(1)
        seen[m.group(1)] = (int(re.search(r"VGPRs: (\d+)", b).group(1)), int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1)))
    assert set(seen) == {"residual", "children", "select"}, seen
    # the residual kernel: (support, depth) of a 48 x 48 staged tile and the bodies' rectangles, nothing else
    assert seen["residual"][1] == 48 * 48 * 5 + 16 * 16 and seen["residual"][0] <= 64, seen


def test_program_over_the_cpp_mirror_runs_or_fails_loudly(tmp_path):
    inc, lib = os.path.join(ROOT, "include"), os.path.join(ROOT, "dbot_ros_amd", "lib")
    exe = str(tmp_path / "scene_find_check")
    r = subprocess.run(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + inc, "-o", exe,
                        os.path.join(HERE, "cpp", "scene_find_check.cpp"),
                        "-L" + lib, "-lrbsensor_mi355x", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout, run.stderr[-2000:])
    if _capi.load().rbs_device_count() > 0:
        head, tail = run.stdout.split("|")
        assert head.split() == ["OK", "1", "0"], run.stdout            # the larger tetrahedron first
        mask, dt0, dt1, joint, same = tail.split()
        assert int(same) == 1 and math.isfinite(float(joint)) and 0 <= int(mask) <= 3, run.stdout
    else:
        assert run.stdout.startswith("NO_DEVICE") and "no CPU path" in run.stdout


# ---------------------------------------------------------------- the whole scene find, in the twin, with the oracle's scores
def test_twin_scene_find_places_two_copies_of_one_mesh_on_their_own_blobs():
    """The expectation of tests/test_gpu_scene_find.py's explain-away test, computed here: ss.explain_away_scene()."""
    s, kw = ss.explain_away_scene()
    r = ss.twin_scene_find(s, **kw)
    assert r["order"] == [0, 1] and r["found_mask"] == 3
    d = ss.distances_to_copies(r["poses"], s.truth)
    assert np.linalg.norm(r["poses"][0, 9:] - r["poses"][1, 9:]) > 0.02          # more than nms_translation apart
    assert sorted(int(np.argmin(row)) for row in d) == [0, 1]                    # one on each copy
    assert d.min(axis=1).max() < 0.01, d                                          # ... and within a centimetre of it
    np.testing.assert_allclose(d.min(axis=1), ss.EXPLAIN_AWAY_TWIN_DISTANCES, rtol=0, atol=1e-6)
    # the residual of the second body has the first body's blob taken out, and only that
    taken = st.bits(r["residuals"][1]) != st.bits(s.frame)
    assert taken.any() and np.isfinite(s.frame[taken]).all()
    assert np.array_equal(st.bits(r["residuals"][0]), st.bits(s.frame))
    # the contrast: nothing explained (explain_sigmas tiny) -> both copies land on the same blob
    r0 = ss.twin_scene_find(s, **dict(kw, explain_sigmas=1e-9))
    assert np.linalg.norm(r0["poses"][0, 9:] - r0["poses"][1, 9:]) < 0.02
    assert r["joint_score"] > r0["joint_score"]
