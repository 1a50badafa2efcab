"""CPU-side checks of the contour rule (rbs_contour_*, include/rbsensor_mi355x.h): the numpy twin (tests/contour_twin.py)
on planted planes and frames, and what the library answers without a device -- the verdict (a pure host function), the
defaults, the refusals, the exported symbols, the records' layout, the one kernel and its register report."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import contour_twin as ct
from dbot_ros_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# a noise model whose tau is exact in binary: sigmas (ms + sf a a) = 3 (2^-8 + 2^-10) = 15 / 1024 at a = 1
MS, SF = 2.0 ** -8, 2.0 ** -10
INF = np.float32(np.inf)
N = 9                                       # planted planes are 9 x 9


def plane(*covered):
    """[81] float32, +inf but for (row, col, depth) in covered."""
    p = np.full((N, N), INF, dtype=np.float32)
    for r, c, d in covered:
        p[r, c] = d
    return p.ravel()


def counts(planes, frame, radius):
    return ct.counts(np.stack(planes), frame, N, N, MS, SF, 3.0, radius)


FAR = np.full(N * N, 5.0, dtype=np.float32)  # a frame far beyond everything planted


# ---------------------------------------------------------------------------------------------- the twin
@pytest.mark.parametrize("r", [1, 2, 3])
def test_one_covered_pixel_has_its_window_as_rim(r):
    c = counts([plane((4, 4, 1.0))], FAR, r)
    assert c.tolist() == [[(2 * r + 1) ** 2 - 1] * 2 + [0, 0, (2 * r + 1) ** 2 - 1]]


@pytest.mark.parametrize("r", [1, 2, 3])
def test_the_window_is_clipped_to_the_image(r):
    for corner in ((0, 0), (0, N - 1), (N - 1, 0), (N - 1, N - 1)):
        c = counts([plane(corner + (1.0,))], FAR, r)
        assert c[0, 0] == (r + 1) ** 2 - 1 and c[0, 4] == c[0, 0], (corner, c.tolist())
    c = counts([plane((0, 4, 1.0))], FAR, r)                           # an edge: r + 1 rows of 2r + 1
    assert c[0, 0] == (r + 1) * (2 * r + 1) - 1


def test_what_one_body_covers_is_not_the_others_rim():
    c = counts([plane((4, 3, 1.0)), plane((4, 4, 1.0))], FAR, 1)
    assert c[:, 0].tolist() == [7, 7]                                   # 3 x 3 less the two covered pixels, each
    covered, a = ct.anchors(np.stack([plane((4, 3, 1.0)), plane((4, 4, 1.0))]), N, N, 1)
    assert covered.sum() == 2
    both = (a[0] > -np.inf) & (a[1] > -np.inf) & ~covered              # a pixel between them counts for both
    assert both.sum() == 4 and both[3, 3] and both[3, 4] and both[5, 3] and both[5, 4]


def test_a_tie_goes_to_the_lowest_body_and_the_other_has_no_rim():
    c = counts([plane((4, 4, 1.0)), plane((4, 4, 1.0))], FAR, 2)
    assert c.tolist() == [[24, 24, 0, 0, 24], [0] * 5]
    c = counts([plane((4, 4, 1.0)), plane((4, 4, 0.5))], FAR, 2)        # the nearer body owns it whatever its index
    assert c.tolist() == [[0] * 5, [24, 24, 0, 0, 24]]


def test_the_anchor_is_the_farthest_owned_depth_in_the_window():
    _, a = ct.anchors(plane((4, 3, 1.0), (4, 5, 2.0))[None], N, N, 1)
    assert a[0, 4, 4] == 2.0 and a[0, 4, 2] == 1.0 and a[0, 4, 6] == 2.0 and a[0, 0, 0] == -np.inf and a.dtype == np.float32
    frame = np.full(N * N, 1.0, dtype=np.float32)                       # flush with the near pixel, in front of the far one
    c = counts([plane((4, 3, 1.0), (4, 5, 2.0))], frame, 1)
    # rim: columns 2 .. 6 of rows 3 .. 5 less the two covered; anchored at 1.0: column 2 and 3 (3 + 2 pixels), the rest at 2.0
    assert c.tolist() == [[13, 13, 5, 8, 0]]


def test_the_class_boundaries_are_inclusive_and_one_ulp_decides():
    tau = 15.0 / 1024.0
    assert 3.0 * (MS + SF * 1.0) == tau
    hi, lo = np.float32(1.0 + tau), np.float32(1.0 - tau)
    assert float(hi) - 1.0 == tau and float(lo) - 1.0 == -tau          # the frame's float holds a +- tau exactly
    ys = (hi, np.nextafter(hi, INF), np.nextafter(hi, -INF), lo, np.nextafter(lo, -INF), np.nextafter(lo, INF))
    for y, want in zip(ys, ("flush", "beyond", "flush", "flush", "in_front", "flush")):
        c = counts([plane((4, 4, 1.0))], np.full(N * N, y, dtype=np.float32), 1)[0]
        col = {"flush": 2, "in_front": 3, "beyond": 4}[want]
        assert c.tolist() == [8, 8] + [8 if k == col else 0 for k in (2, 3, 4)], (float(y), want)


def test_readings_that_are_not_finite_zero_or_negative():
    frame = np.full((N, N), 1.0, dtype=np.float32)
    frame[3, 3:6] = (np.inf, -np.inf, np.nan)
    frame[4, 3], frame[4, 5] = 0.0, -2.0
    frame[4, 4] = np.nan                                               # the covered pixel's reading is nobody's business
    c = counts([plane((4, 4, 1.0))], frame.ravel(), 1)[0]
    # +-inf and NaN: a rim pixel without a reading; 0 and negative depths are finite readings far in front
    assert c.tolist() == [8, 5, 3, 2, 0]


def test_an_empty_pose_has_no_rim():
    planes = np.full((3, N * N), np.inf, dtype=np.float32)
    c, v = ct.contour(planes, FAR, N, N, MS, SF)
    assert not c.any() and v.tolist() == [ct.NO_RIM] * 3
    planes[1] = plane((4, 4, 1.0))                                      # one body alone in view
    c, v = ct.contour(planes, FAR, N, N, MS, SF)
    assert c.tolist() == [[0] * 5, [24, 24, 0, 0, 24], [0] * 5] and v.tolist() == [ct.NO_RIM, ct.PRESENT, ct.NO_RIM]


def test_the_verdict_rule_in_order():
    assert ct.verdict([15, 15, 0, 0, 15]) == ct.NO_RIM                 # 1. too few rim pixels, whatever they say
    assert ct.verdict([100, 49, 0, 0, 49]) == ct.UNDECIDED             # 2. valid < 0.5 rim
    assert ct.verdict([100, 0, 0, 0, 0], min_valid_fraction=0.0) == ct.UNDECIDED   # valid == 0 decides nothing
    assert ct.verdict([100, 50, 35, 0, 15]) == ct.PRESENT              # 3. beyond 15 >= 0.3 x 50, before flush is asked
    assert ct.verdict([100, 50, 25, 11, 14]) == ct.ABSENT              # 4. flush 25 >= 0.5 x 50
    assert ct.verdict([100, 50, 24, 12, 14]) == ct.UNDECIDED           # 5.


# ---------------------------------------------------------------------------------------------- the library, no device
def c_params(params):
    return _capi.RbsContourParams(params["radius"], params["min_rim_pixels"], params["min_valid_fraction"],
                                  params["min_contour_fraction"], params["min_flush_fraction"])


def lib_verdict(lib, c, params=None):
    body = _capi.RbsContourBody(*(int(v) for v in c[:5]))
    v = C.c_int32(-7)
    p = c_params(params) if params is not None else None
    rc = lib.rbs_contour_verdict(C.byref(p) if p is not None else None, C.byref(body), C.byref(v))
    return rc, v.value


def test_library_verdict_equals_the_twin_on_random_records():
    lib = _capi.load()
    rng = np.random.default_rng(5)
    seen = set()
    for _ in range(4000):
        rim = int(rng.choice([0, 1, 15, 16, 17, 100, 1000, 307200]))
        valid = int(rng.choice([0, rim // 2, rim, int(rng.integers(0, rim + 1))]))
        parts = rng.multinomial(valid, rng.dirichlet(np.ones(3) * 0.5))
        c = [rim, valid, int(parts[0]), int(parts[1]), int(parts[2])]
        params = dict(radius=int(rng.choice([1, 2, 8])), min_rim_pixels=int(rng.choice([1, 16, 64])),
                      min_valid_fraction=float(rng.choice([0.0, 0.25, 0.5, 1.0])),
                      min_contour_fraction=float(rng.choice([0.0, 0.3, 0.5, 1.0])),
                      min_flush_fraction=float(rng.choice([0.0, 0.5, 0.9, 1.0])))
        rc, v = lib_verdict(lib, c, params)
        assert rc == _capi.RBS_OK
        assert v == ct.verdict(c, **params), (c, params)
        seen.add(v)
    assert seen == {0, 1, 2, 3}


def test_library_verdict_on_each_boundary_and_the_defaults():
    lib = _capi.load()
    d = _capi.RbsContourParams()
    lib.rbs_contour_default_params(C.byref(d))
    assert (d.radius, d.min_rim_pixels, d.min_valid_fraction, d.min_contour_fraction, d.min_flush_fraction) == (2, 16, 0.5, 0.3, 0.5)
    assert ct.DEFAULTS == dict(radius=2, min_rim_pixels=16, min_valid_fraction=0.5, min_contour_fraction=0.3, min_flush_fraction=0.5)
    cases = [([15, 15, 0, 0, 15], ct.NO_RIM), ([16, 16, 0, 0, 16], ct.PRESENT),                   # 1. rim < min_rim_pixels
             ([0, 0, 0, 0, 0], ct.NO_RIM),
             ([100, 49, 0, 0, 49], ct.UNDECIDED), ([100, 50, 0, 0, 50], ct.PRESENT),              # 2. valid < 0.5 rim
             ([100, 0, 0, 0, 0], ct.UNDECIDED),                                                   #    valid == 0
             ([100, 100, 71, 0, 29], ct.ABSENT), ([100, 100, 70, 0, 30], ct.PRESENT),             # 3. beyond >= 0.3 valid
             ([100, 100, 49, 51, 0], ct.UNDECIDED), ([100, 100, 50, 50, 0], ct.ABSENT),           # 4. flush >= 0.5 valid
             ([100, 100, 0, 100, 0], ct.UNDECIDED)]                                               # 5. all in front
    for c, want in cases:
        assert ct.verdict(c) == want, c
        assert lib_verdict(lib, c) == (_capi.RBS_OK, want), c                                     # NULL params: the defaults
        assert lib_verdict(lib, c, ct.DEFAULTS) == (_capi.RBS_OK, want), c
    zero = dict(ct.DEFAULTS, min_valid_fraction=0.0)                                              # valid == 0 stays undecided
    assert ct.verdict([100, 0, 0, 0, 0], **zero) == ct.UNDECIDED
    assert lib_verdict(lib, [100, 0, 0, 0, 0], zero) == (_capi.RBS_OK, ct.UNDECIDED)


def test_symbols_are_declared_and_exported():
    text = open(os.path.join(ROOT, "include", "rbsensor_mi355x.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = C.CDLL(_capi.LIB_PATH)
    names = ("rbs_contour_default_params", "rbs_contour_poses", "rbs_contour_verdict", "rbs_contour_kernel_ms")
    for s in names:
        assert re.search(r"\b" + s + r"\s*\(", text), s
        assert s in _capi.EXPORTS and hasattr(lib, s), s
    assert sorted(set(re.findall(r"\b(rbs_contour_[a-z0-9_]+)\s*\(", text))) == sorted(names)
    for k, name in enumerate(("RBS_CONTOUR_NO_RIM", "RBS_CONTOUR_UNDECIDED", "RBS_CONTOUR_PRESENT", "RBS_CONTOUR_ABSENT")):
        assert re.search(name + r"\s*=\s*%d\b" % k, text) and getattr(_capi, name) == k
    from dbot_ros_amd import assess
    assert (assess.CONTOUR_NO_RIM, assess.CONTOUR_UNDECIDED, assess.CONTOUR_PRESENT, assess.CONTOUR_ABSENT) == (0, 1, 2, 3)
    assert (ct.NO_RIM, ct.UNDECIDED, ct.PRESENT, ct.ABSENT) == (0, 1, 2, 3)


def test_record_and_params_layout():
    assert C.sizeof(_capi.RbsContourBody) == 32 and _capi.RbsContourBody.verdict.offset == 20
    assert [getattr(_capi.RbsContourBody, f).offset for f in ("rim", "valid", "flush", "in_front", "beyond")] == [0, 4, 8, 12, 16]
    assert C.sizeof(_capi.RbsContourParams) == 32
    assert [getattr(_capi.RbsContourParams, f).offset for f in
            ("radius", "min_rim_pixels", "min_valid_fraction", "min_contour_fraction", "min_flush_fraction")] == [0, 4, 8, 16, 24]
    src = open(os.path.join(ROOT, "dbot_ros_amd", "csrc", "rbsensor_contour.hip")).read()
    assert "static_assert(sizeof(rbs_contour_body) == 32" in src and "static_assert(sizeof(rbs_contour_params) == 32" in src


def test_the_source_holds_one_kernel_that_neither_spills_nor_uses_scratch():
    src = open(os.path.join(ROOT, "dbot_ros_amd", "csrc", "rbsensor_contour.hip")).read()
    assert re.findall(r"__global__[^\n]*?void\s+(\w+)\s*\(", src) == ["rbs_contour_count_kernel"]
    capi = open(os.path.join(ROOT, "dbot_ros_amd", "csrc", "rbsensor_capi.hip")).read()
    assert capi.index('#include "rbsensor_assess.hip"') < capi.index('#include "rbsensor_contour.hip"')
    assert "rbsensor_contour.hip" in open(os.path.join(ROOT, "dbot_ros_amd", "csrc", "Makefile")).read()
    txt = open(os.path.join(ROOT, "dbot_ros_amd", "lib", "resource_usage.txt")).read()
    blocks = [b for b in re.split(r"remark: Function Name: ", txt)[1:] if "rbs_contour_count_kernel" in b.split()[0]]
    assert len(blocks) == 1
    b = blocks[0]
    assert re.search(r"ScratchSize \[bytes/lane\]: 0\b", b) and re.search(r"SGPRs Spill: 0\b", b) and re.search(r"VGPRs Spill: 0\b", b), b
    lds = int(re.search(r"LDS Size \[bytes/block\]: (\d+)", b).group(1))
    assert lds <= 48 * 48 * 8 + 16 * 48 * 32 * 4                       # the staging tile and B row-max planes bound it; it uses one


def test_bad_arguments_are_refused_before_any_device_call():
    lib = _capi.load()
    inv = _capi.RBS_ERR_INVALID_ARGUMENT
    poses = np.zeros(12)
    out = (_capi.RbsContourBody * 1)()
    assert lib.rbs_contour_poses(None, None, None, None, poses.ctypes.data_as(C.POINTER(C.c_double)), 1, None, out) == inv
    assert lib.rbs_contour_kernel_ms(None, (C.c_float * 3)()) == inv
    lib.rbs_contour_default_params(None)   # no-op
    body, v = _capi.RbsContourBody(100, 100, 50, 0, 50), C.c_int32()
    assert lib.rbs_contour_verdict(None, None, C.byref(v)) == inv
    assert lib.rbs_contour_verdict(None, C.byref(body), None) == inv
    good = dict(ct.DEFAULTS)
    nan = float("nan")
    for key, bad in (("radius", 0), ("radius", 9), ("radius", -1), ("min_rim_pixels", 0), ("min_rim_pixels", -3),
                     ("min_valid_fraction", -0.1), ("min_valid_fraction", 1.5), ("min_valid_fraction", nan),
                     ("min_contour_fraction", -0.1), ("min_contour_fraction", 1.0001), ("min_contour_fraction", nan),
                     ("min_flush_fraction", -0.1), ("min_flush_fraction", 1.5), ("min_flush_fraction", nan)):
        rc, _ = lib_verdict(lib, [100, 100, 50, 0, 50], dict(good, **{key: bad}))
        assert rc == inv, (key, bad)
    for radius in (1, 8):
        assert lib_verdict(lib, [100, 100, 50, 0, 50], dict(good, radius=radius)) == (_capi.RBS_OK, ct.PRESENT)


def test_python_parameters_mirror_the_c_defaults():
    from dbot_ros_amd.assess import Assessment, PoseAssessor
    p = PoseAssessor.ContourParameters()
    assert (p.radius, p.min_rim_pixels, p.min_valid_fraction, p.min_contour_fraction, p.min_flush_fraction) == (2, 16, 0.5, 0.3, 0.5)
    q = PoseAssessor.ContourParameters.from_mapping({"radius": 3, "min_flush_fraction": 1})
    assert (q.radius, q.min_flush_fraction, q.min_rim_pixels) == (3, 1.0, 16)
    assert PoseAssessor.ContourParameters.from_mapping(None) == p and PoseAssessor.ContourParameters.from_mapping({}) == p
    with pytest.raises(ValueError):
        PoseAssessor.ContourParameters.from_mapping({"radii": 2})
    c = q.c_params()
    assert (c.radius, c.min_rim_pixels, c.min_valid_fraction, c.min_contour_fraction, c.min_flush_fraction) == (3, 16, 0.5, 0.3, 1.0)
    # confirmed_mask: every body SUPPORTED, and with the contour rule on every body PRESENT
    verdicts = np.array([[2, 2], [2, 3], [2, 2], [2, 2]])
    off = Assessment(np.zeros((4, 2, 5), dtype=np.int32), verdicts)
    assert off.contour_counts is None and off.contour_verdicts is None and off.confirmed_mask().tolist() == [True, False, True, True]
    on = Assessment(off.counts, verdicts, off.counts, np.array([[2, 2], [2, 2], [2, 3], [1, 2]]))
    assert on.confirmed_mask().tolist() == [True, False, False, False]


def test_supervisor_and_node_take_the_contour_switches():
    from dbot_ros_amd.supervisor import TrackSupervisor

    class Tracker:
        parts = 1

    class Plain:
        contour = None

    with pytest.raises(ValueError):
        TrackSupervisor(Tracker(), Plain(), contour_lost=True)           # contour_lost needs the contour rule
    assert TrackSupervisor(Tracker(), Plain()).contour_lost is False


def test_supervisor_logic_with_the_contour_rule_on():
    """Host logic only, over a scripted tracker and assessor: contour_lost counts ABSENT frames as lost, and a found state
    must be SUPPORTED and PRESENT."""
    from dbot_ros_amd.assess import CONTOUR_ABSENT, CONTOUR_PRESENT, CONTOUR_UNDECIDED, SUPPORTED, Assessment
    from dbot_ros_amd.supervisor import TrackSupervisor

    class Tracker:
        parts = 1

        def __init__(self):
            self.started = []

        def track(self, frame):
            return np.zeros(12)

        def initialize(self, states):
            self.started.append(np.asarray(states[0]).copy())

    class Scripted:
        contour = object()

        def __init__(self, track_contour, found_contour):
            self.track_contour, self.found_contour = track_contour, found_contour

        def assess_state(self, tracker, state, frame):
            found = bool(np.asarray(state).any())                        # the finder's state is all ones, the estimate all zeros
            zero = np.zeros((1, 1, 5), dtype=np.int32)
            return Assessment(zero, np.array([[SUPPORTED]]), zero, np.array([[self.found_contour if found else self.track_contour]]))

    def events(sup, n=8):
        return [sup.step(None)[2] for _ in range(n)]

    find = lambda frame: np.ones(12)                                     # noqa: E731
    # a SUPPORTED track whose contour reads ABSENT is lost only when asked
    assert events(TrackSupervisor(Tracker(), Scripted(CONTOUR_ABSENT, CONTOUR_PRESENT), find=find, lost_frames=3)) == [None] * 8
    assert events(TrackSupervisor(Tracker(), Scripted(CONTOUR_ABSENT, CONTOUR_PRESENT), lost_frames=3, contour_lost=True)) == \
        [None, None, "lost", None, None, "lost", None, None]
    assert events(TrackSupervisor(Tracker(), Scripted(CONTOUR_UNDECIDED, CONTOUR_PRESENT), lost_frames=3, contour_lost=True)) == [None] * 8
    # ... and the re-found state must be PRESENT as well as SUPPORTED
    tr = Tracker()
    sup = TrackSupervisor(tr, Scripted(CONTOUR_ABSENT, CONTOUR_ABSENT), find=find, lost_frames=3, contour_lost=True)
    assert events(sup, 7) == [None, None, "lost", "find_failed", None, None, "find_failed"] and not tr.started
    tr = Tracker()
    assessor = Scripted(CONTOUR_ABSENT, CONTOUR_PRESENT)
    sup = TrackSupervisor(tr, assessor, find=find, lost_frames=3, contour_lost=True)
    assert events(sup, 4) == [None, None, "lost", "reacquired"] and len(tr.started) == 1 and tr.started[0].all()
