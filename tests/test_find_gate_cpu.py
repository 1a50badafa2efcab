"""CPU-side checks of the finder's silhouette gate (rbs_find_set_gate, include/rbsensor_mi355x.h steps 4b, 5 and 7): the
numpy twin (tests/find_gate_twin.py) on planted planes and frames, the gated orders, and what the library answers without a
device -- defaults, refusals, the yaml mapping, the exported symbols, the struct's layout, the one evidence kernel and its
register report."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import assess_twin as at
import contour_twin as ct
import find_gate_twin as gt
import find_twin as ft
from dbot_ros_amd import _capi
from dbot_ros_amd.finder import ObjectFinder, SceneFinder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# a noise model whose tau is exact in binary: sigmas (ms + sf d d) = 3 (2^-8 + 2^-10) = 15 / 1024 at d = 1
MS, SF = 2.0 ** -8, 2.0 ** -10
TAU = 15.0 / 1024.0
INF = np.float32(np.inf)
N = 12                                       # planted planes are 12 x 12


def block(r0, r1, c0, c1, depth=1.0):
    """[N * N] float32, +inf but for depth on rows r0 .. r1 - 1, columns c0 .. c1 - 1."""
    p = np.full((N, N), INF, dtype=np.float32)
    p[r0:r1, c0:c1] = depth
    return p.ravel()


def evidence(plane, frame, **params):
    return gt.evidence(plane, frame, N, N, MS, SF, **params)


# ---------------------------------------------------------------------------------------------- the twin's evidence
def test_the_record_is_the_two_twins_side_by_side():
    rng = np.random.default_rng(1)
    plane = block(3, 8, 4, 9)
    frame = (1.0 + rng.normal(0.0, 2 * TAU, N * N)).astype(np.float32)
    for radius in (1, 2, 3):
        rec, cls = evidence(plane, frame, radius=radius)
        a = at.counts(plane[None], frame, MS, SF, 3.0)[0]
        c = ct.counts(plane[None], frame, N, N, MS, SF, 3.0, radius)[0]
        assert rec.dtype == np.int32 and rec.tolist() == a.tolist() + c.tolist()
        assert cls == (0 if at.verdict(a) == at.SUPPORTED and ct.verdict(c, radius=radius) == ct.PRESENT else 1)
    assert rec[0] == 25 and rec[5] == 11 * 11 - 25                          # radius 3: the block's window, less the block


def test_a_body_on_its_background_is_confirmed_and_one_in_the_wall_is_not():
    plane = block(3, 8, 4, 9)
    stands = np.where(np.isfinite(plane), 1.0, 2.0).astype(np.float32)      # the body's face, the wall far behind its rim
    rec, cls = evidence(plane, stands, min_rim_pixels=8)
    assert rec.tolist() == [25, 25, 25, 0, 0, 56, 56, 0, 0, 56] and cls == 0
    in_wall = np.full(N * N, 1.0, dtype=np.float32)                         # the rim reads flush with the face
    rec, cls = evidence(plane, in_wall, min_rim_pixels=8)
    assert rec.tolist() == [25, 25, 25, 0, 0, 56, 56, 56, 0, 0] and cls == 1
    rec, cls = evidence(plane, np.full(N * N, 0.5, dtype=np.float32), min_rim_pixels=8)   # everything in front: occluded
    assert rec.tolist() == [25, 25, 0, 25, 0, 56, 56, 0, 56, 0] and cls == 1


def record(rendered, support, behind, rim, valid, beyond, in_front=0):
    """Ten counts with the given entries; the dependent ones filled consistently."""
    return np.array([rendered, support + behind + in_front, support, in_front, behind, rim, valid, valid - beyond, 0, beyond], dtype=np.int32)


@pytest.mark.parametrize("key, at_bar, below", [
    ("min_pixels", record(16, 16, 0, 64, 64, 64), record(15, 15, 0, 64, 64, 64)),
    ("min_visible_fraction", record(64, 16, 0, 64, 64, 64, in_front=48), record(64, 15, 0, 64, 64, 64, in_front=49)),   # u = 0.25 rendered
    ("min_support_fraction", record(64, 16, 16, 64, 64, 64), record(64, 15, 17, 64, 64, 64)),                          # support = 0.5 u
    ("min_rim_pixels", record(64, 64, 0, 16, 16, 16), record(64, 64, 0, 15, 15, 15)),
    ("min_valid_fraction", record(64, 64, 0, 64, 32, 32), record(64, 64, 0, 64, 31, 31)),                              # valid = 0.5 rim
    ("min_contour_fraction", record(64, 64, 0, 80, 80, 24), record(64, 64, 0, 80, 80, 23)),                            # beyond = 0.3 valid
])
def test_each_threshold_of_the_class_at_equality_and_one_count_either_side(key, at_bar, below):
    assert gt.class_of(at_bar) == 0, key                                   # equality confirms: every comparison is inclusive
    assert gt.class_of(below) == 1, key
    above = at_bar.copy()
    if key == "min_contour_fraction":
        above[9] += 1; above[7] -= 1
        assert gt.class_of(above) == 0
        # 0.3 x 80 is not exact in binary64: the product the rule compares with is the twin's, whatever it rounds to
        assert (float(at_bar[9]) >= 0.3 * float(at_bar[6])) and not (float(below[9]) >= 0.3 * float(below[6]))
    # the same decisions through the library's host verdicts
    lib = _capi.load()
    for rec in (at_bar, below):
        a, c, v, w = _capi.RbsAssessBody(*map(int, rec[:5])), _capi.RbsContourBody(*map(int, rec[5:])), C.c_int32(), C.c_int32()
        assert lib.rbs_assess_verdict(None, C.byref(a), C.byref(v)) == 0 and lib.rbs_contour_verdict(None, C.byref(c), C.byref(w)) == 0
        assert (0 if v.value == at.SUPPORTED and w.value == ct.PRESENT else 1) == gt.class_of(rec)


def test_min_flush_fraction_does_not_enter_the_class():
    rec = record(64, 64, 0, 80, 80, 24)
    assert gt.class_of(rec, min_flush_fraction=0.0) == gt.class_of(rec, min_flush_fraction=1.0) == 0
    rec = record(64, 64, 0, 80, 80, 23)                                     # ABSENT or UNDECIDED: both class 1
    assert gt.class_of(rec, min_flush_fraction=0.0) == gt.class_of(rec, min_flush_fraction=1.0) == 1


def test_the_class_boundary_of_a_reading_is_inclusive_and_one_ulp_decides():
    plane = block(5, 6, 5, 6)                                               # one covered pixel, a rim of 8 at radius 1
    hi = np.float32(1.0 + TAU)
    assert float(hi) - 1.0 == TAU
    for y, col in ((hi, 7), (np.nextafter(hi, INF), 9), (np.float32(1.0 - TAU), 7), (np.nextafter(np.float32(1.0 - TAU), -INF), 8)):
        rec, _ = evidence(plane, np.full(N * N, y, dtype=np.float32), radius=1)
        assert rec[5:].tolist() == [8, 8] + [8 if k == col else 0 for k in (7, 8, 9)], float(y)
        assert rec[:5].tolist() == [1, 1] + [1 if k + 5 == col else 0 for k in (2, 3, 4)]


def test_nan_and_infinite_readings_on_the_rim():
    plane = block(5, 6, 5, 6)
    frame = np.full((N, N), 2.0, dtype=np.float32)
    frame[4, 4:7] = (np.nan, np.inf, -np.inf)
    rec, _ = evidence(plane, frame.ravel(), radius=1)
    assert rec.tolist() == [1, 1, 0, 0, 1, 8, 5, 0, 0, 5]                   # three rim pixels without a reading
    frame[5, 5] = np.nan                                                    # ... and the covered pixel without one
    rec, _ = evidence(plane, frame.ravel(), radius=1)
    assert rec.tolist() == [1, 0, 0, 0, 0, 8, 5, 0, 0, 5]


def test_a_rim_clipped_at_the_image_border():
    far = np.full(N * N, 2.0, dtype=np.float32)
    for r in (1, 2, 3):
        rec, _ = evidence(block(0, 1, 0, 1), far, radius=r)                 # a corner pixel
        assert rec[5] == (r + 1) ** 2 - 1 and rec[9] == rec[5]
        rec, _ = evidence(block(0, 2, 4, 7), far, radius=r)                 # a block on the top border
        assert rec[0] == 6 and rec[5] == (2 + r) * (3 + 2 * r) - 6
        rec, _ = evidence(block(N - 2, N, N - 3, N), far, radius=r)         # ... and in the bottom right corner
        assert rec[5] == (2 + r) * (3 + r) - 6


def test_an_empty_plane_is_class_1_with_a_record_of_zeros():
    rec, cls = evidence(np.full(N * N, INF, dtype=np.float32), np.full(N * N, 1.0, dtype=np.float32))
    assert not rec.any() and cls == 1


# ---------------------------------------------------------------------------------------------- the gated orders
def reference_order(scores, classes, k):
    """(class, -score, index) sorted in plain Python, NaN dropped."""
    items = sorted((int(c), -float(s), i) for i, (s, c) in enumerate(zip(scores, classes)) if s == s)
    return [i for _, _, i in items][:k]


def test_gated_topk_on_ties_nan_and_short_classes():
    nan = np.nan
    scores = np.array([5.0, 7.0, 7.0, nan, 9.0, 7.0, nan, 1.0, 9.0, -np.inf])
    classes = np.array([1, 0, 1, 0, 1, 0, 1, 0, 1, 0])
    s, i = gt.gated_topk(scores, classes, 6)
    assert i.tolist() == [1, 5, 7, 9, 4, 8] and s.tolist() == [7.0, 7.0, 1.0, -np.inf, 9.0, 9.0]   # ties: the lower index; NaN never
    assert gt.gated_topk(scores, classes, 3)[1].tolist() == [1, 5, 7]      # more class 0 than asked for
    assert gt.gated_topk(scores, classes, 64)[1].tolist() == [1, 5, 7, 9, 4, 8, 2, 0]   # fewer numbers than asked for
    assert gt.gated_topk(scores, np.ones(10, dtype=int), 4)[1].tolist() == [4, 8, 1, 2]   # no class 0: plain selection
    assert gt.gated_topk(scores, np.zeros(10, dtype=int), 4)[1].tolist() == [4, 8, 1, 2]  # all class 0: plain selection
    assert gt.gated_topk(np.full(5, nan), np.zeros(5, dtype=int), 4)[1].tolist() == []
    assert gt.gated_topk(np.array([0.0, -0.0, 0.0]), np.array([1, 1, 0]), 3)[1].tolist() == [2, 0, 1]   # -0 == +0: the index decides


def test_gated_topk_equals_a_plain_sort_on_random_input():
    rng = np.random.default_rng(5)
    for n, k in ((1, 1), (7, 16), (500, 64), (5000, 512)):
        scores = np.round(rng.normal(0, 3, n))                              # many ties
        scores[rng.random(n) < 0.1] = np.nan
        classes = (rng.random(n) < 0.7).astype(int)
        s, i = gt.gated_topk(scores, classes, k)
        assert i.tolist() == reference_order(scores, classes, k) and np.array_equal(s, scores[i])
        # with every class alike it is the finder's plain selection
        plain = ft.select_order(scores)[:k]
        assert gt.gated_topk(scores, np.ones(n, dtype=int), k)[1].tolist() == plain.tolist()
        # the index given: hypothesis numbers that are not positions
        idx = rng.permutation(n).astype(np.int64) * 3
        s2, i2 = gt.gated_topk(scores, classes, k, idx)
        want = sorted((int(c), -float(v), int(h)) for v, c, h in zip(scores, classes, idx) if v == v)[:k]
        assert i2.tolist() == [h for _, _, h in want]


def test_result_order_and_found():
    nan = np.nan
    scores = np.array([10.0, nan, 30.0, 20.0, nan, 20.0])
    classes = np.array([0, 0, 1, 0, 1, 0])
    o = gt.result_order(scores, classes)
    assert o.tolist() == [3, 5, 0, 2, 1, 4]                                 # class 0 by score, ties by index; class 1; NaN last in survivor order
    assert gt.found(scores, classes, o, -np.inf, True) and gt.found(scores, classes, o, 20.0, True)
    assert not gt.found(scores, classes, o, 20.5, True) and not gt.found(scores, classes, o, 20.5, False)
    ones = np.ones(6, dtype=int)
    o = gt.result_order(scores, ones)
    assert o.tolist() == ft.result_order(scores).tolist() == [2, 3, 5, 0, 1, 4]   # no pose confirmed: today's order
    assert gt.found(scores, ones, o, -np.inf, False) and not gt.found(scores, ones, o, -np.inf, True)
    o = gt.result_order(np.full(3, nan), np.zeros(3, dtype=int))
    assert o.tolist() == [0, 1, 2] and not gt.found(np.full(3, nan), np.zeros(3, dtype=int), o, -np.inf, False)
    assert not gt.found(np.zeros(0), np.zeros(0), np.zeros(0, dtype=int), -np.inf, False)


# ---------------------------------------------------------------------------------------------- the twin chain on the scene
def test_the_twin_chain_finds_the_visible_body_that_plain_selection_puts_into_the_slab():
    """Body m1 of Scene(("m1", "m2"), 640, 480, 101) in the numpy twins with the eager oracle's scores (steps 1b and 6b on,
    tests/test_gpu_scene_find.py's accuracy settings): with the gate the final order begins with a confirmed pose within 1 mm
    of the truth -- the only confirmed final; plain selection's pose 0 lies more than 0.3 m off, at a higher score.  About
    100 s on 8 threads; the figures are kept in tests/find_gate_scenes.py."""
    import find_gate_scenes as gs
    s = gs.scene()
    truth = s.truth[gs.BODY, 9:]
    r = gs.twin_find(s, {})
    d = float(np.linalg.norm(r["poses"][0, 9:] - truth))
    print("gated", r["hypotheses"], r["confirmed_hypotheses"], r["candidates_near"], d, r["scores"][0], r["classes"].tolist())
    assert r["found"] and r["classes"][0] == 0 and d < 1e-3
    assert (r["hypotheses"], r["confirmed_hypotheses"], r["candidates_near"]) == (gs.TWIN_GATED["hypotheses"], gs.TWIN_GATED["confirmed_hypotheses"],
                                                                                 gs.TWIN_GATED["candidates_near"])
    assert int((r["classes"] == 0).sum()) == gs.TWIN_GATED["confirmed_finals"]
    assert d == pytest.approx(gs.TWIN_GATED["distance"], abs=2e-5) and r["scores"][0] == pytest.approx(gs.TWIN_GATED["score"], rel=1e-6)
    q = gs.twin_find(s, None)
    dq = float(np.linalg.norm(q["poses"][0, 9:] - truth))
    print("plain", dq, q["scores"][0])
    assert dq > 0.3 and q["scores"][0] > r["scores"][0]
    assert dq == pytest.approx(gs.TWIN_PLAIN["distance"], abs=1e-3) and q["scores"][0] == pytest.approx(gs.TWIN_PLAIN["score"], rel=1e-4)


# ---------------------------------------------------------------------------------------------- the library, no device
NAMES = ("rbs_find_default_gate", "rbs_find_set_gate", "rbs_find_get_evidence", "rbs_find_gate_ms", "rbs_find_scene_set_gate")


def test_symbols_are_declared_and_exported_and_the_struct_is_mirrored():
    text = open(os.path.join(ROOT, "include", "rbsensor_mi355x.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = C.CDLL(_capi.LIB_PATH)
    for s in NAMES:
        assert re.search(r"\b" + s + r"\s*\(", code) and s in _capi.EXPORTS and hasattr(lib, s), s
    assert "4b evidence" in text
    fields = re.search(r"typedef struct rbs_find_gate \{(.*?)\} rbs_find_gate;", code, re.S).group(1)
    declared = [n.strip() for line in fields.split(";") for n in re.sub(r"^\s*(int32_t|double)", "", line).split(",") if n.strip()]
    assert declared == [f[0] for f in _capi.RbsFindGate._fields_]
    assert C.sizeof(_capi.RbsFindGate) == 72 and _capi.RbsFindGate.sigmas.offset == 24 and _capi.RbsFindGate.min_flush_fraction.offset == 64
    src = open(os.path.join(ROOT, "dbot_ros_amd", "csrc", "rbsensor_find_gate.hip")).read()
    assert "static_assert(sizeof(rbs_find_gate) == 72" in src


def test_defaults_are_the_two_rules_defaults():
    lib = _capi.load()
    g = _capi.RbsFindGate()
    lib.rbs_find_default_gate(C.byref(g))
    lib.rbs_find_default_gate(None)   # no-op
    a, c = _capi.RbsAssessParams(), _capi.RbsContourParams()
    lib.rbs_assess_default_params(C.byref(a))
    lib.rbs_contour_default_params(C.byref(c))
    assert (g.enabled, g.require_confirmed) == (1, 0)
    assert (g.sigmas, g.min_support_fraction, g.min_visible_fraction, g.min_pixels) == (a.sigmas, a.min_support_fraction, a.min_visible_fraction, a.min_pixels)
    assert (g.radius, g.min_rim_pixels, g.min_valid_fraction, g.min_contour_fraction, g.min_flush_fraction) == \
        (c.radius, c.min_rim_pixels, c.min_valid_fraction, c.min_contour_fraction, c.min_flush_fraction)
    d = ObjectFinder.Gate()
    for f in g._fields_:
        assert getattr(g, f[0]) == getattr(d, f[0]), f[0]
    assert all(gt.DEFAULTS[k] == getattr(g, k) for k in gt.DEFAULTS) and len(gt.DEFAULTS) == len(g._fields_) - 2
    cp = ObjectFinder.Gate(require_confirmed=True, radius=3, sigmas=2).c_params()
    assert (cp.enabled, cp.require_confirmed, cp.radius, cp.sigmas, cp.min_pixels) == (1, 1, 3, 2.0, 16)


def test_null_handles_are_refused_before_any_device_call():
    lib = _capi.load()
    inv = _capi.RBS_ERR_INVALID_ARGUMENT
    g = _capi.RbsFindGate()
    lib.rbs_find_default_gate(C.byref(g))
    n = C.c_int64()
    assert lib.rbs_find_set_gate(None, C.byref(g)) == inv and lib.rbs_find_set_gate(None, None) == inv
    assert lib.rbs_find_get_evidence(None, _capi.RBS_FIND_COARSE, None, None, C.byref(n)) == inv
    assert lib.rbs_find_gate_ms(None, (C.c_float * 2)()) == inv
    assert lib.rbs_find_scene_set_gate(None, C.byref(g)) == inv


def test_the_yaml_mapping_and_the_builders_pass_the_gate_on():
    p = ObjectFinder.Parameters.from_rosparam({"object_finder": {"n_rotations": 64, "gate": {"require_confirmed": True, "radius": 3,
                                                                                            "min_contour_fraction": 0.25}}})
    assert p.n_rotations == 64 and isinstance(p.gate, ObjectFinder.Gate)
    assert (p.gate.enabled, p.gate.require_confirmed, p.gate.radius, p.gate.min_contour_fraction, p.gate.sigmas) == (True, True, 3, 0.25, 3.0)
    assert isinstance(p.gate.require_confirmed, bool) and isinstance(p.gate.radius, int)
    assert ObjectFinder.Parameters.from_rosparam({}).gate is None and ObjectFinder.Parameters().gate is None
    assert ObjectFinder.Gate.from_mapping(None) == ObjectFinder.Gate() and ObjectFinder.Gate.from_mapping({}) == ObjectFinder.Gate()
    assert ObjectFinder.Gate.from_mapping({"enabled": 0}).enabled is False
    with pytest.raises(ValueError, match="object_finder/gate/radiu"):
        ObjectFinder.Parameters.from_rosparam({"object_finder": {"gate": {"radiu": 1}}})
    cp = p.c_params()                                                       # the gate is no field of rbs_find_params
    assert cp.n_rotations == 64 and not hasattr(cp, "gate")
    import inspect
    from dbot_ros_amd import node
    for fn in (node.build_object_finder, node.build_scene_finder):
        assert "gate=finder_params.gate" in inspect.getsource(fn)
    for cls in (ObjectFinder, SceneFinder):
        assert "gate" in inspect.signature(cls.__init__).parameters and callable(cls.set_gate)
    assert callable(ObjectFinder.evidence) and callable(ObjectFinder.gate_ms)


def test_the_source_holds_one_evidence_kernel_that_neither_spills_nor_uses_scratch():
    """The compiler's report for gfx950: no scratch and nothing spilled, scalar registers included (184 VGPRs: the kernel keeps
    what the rasterizer reads in vector registers)."""
    src = open(os.path.join(ROOT, "dbot_ros_amd", "csrc", "rbsensor_find_gate.hip")).read()
    kernels = re.findall(r"__global__[^\n]*?void\s+(\w+)\s*\(", src)
    assert kernels == ["rbs_findc_evidence_kernel", "rbs_findc_mask_kernel", "rbs_findc_merge_kernel", "rbs_findc_order_kernel"]
    assert not any(re.fullmatch(r"rbs_find_\w*_kernel", k) for k in kernels)   # (that list is closed: tests/test_finder_cpu.py)
    find = open(os.path.join(ROOT, "dbot_ros_amd", "csrc", "rbsensor_find.hip")).read()
    assert find.index('#include "rbsensor_find_gate.hip"') < find.index('#include "rbsensor_find_scene.hip"')
    assert "rbsensor_find_gate.hip" in open(os.path.join(ROOT, "dbot_ros_amd", "csrc", "Makefile")).read()
    for unchanged in ("rbs_find_topk_kernel", "rbs_find_nms_kernel", "rbs_find_keep_kernel"):
        assert unchanged not in re.sub(r"//[^\n]*", "", src)                # the gate launches them through rbsensor_find.hip's helpers
    release = open(_capi.LIB_PATH, "rb").read() if _capi.LIB_PATH.endswith("librbsensor_mi355x.so") else b""
    assert b"rbs_test_findc" not in release
    txt = open(os.path.join(ROOT, "dbot_ros_amd", "lib", "resource_usage.txt")).read()
    seen = {}
    for b in re.split(r"remark: Function Name: ", txt)[1:]:
        m = re.search(r"rbs_findc_(\w+?)_kernel", b.split()[0])
        if m:
            seen[m.group(1)] = b
    assert set(seen) == {"evidence", "mask", "merge", "order"}
    for name, b in seen.items():
        assert re.search(r"ScratchSize \[bytes/lane\]: 0\b", b) and re.search(r"VGPRs Spill: 0\b", b), (name, b)
    for name, b in seen.items():
        assert re.search(r"SGPRs Spill: 0\b", b), (name, re.search(r"SGPRs Spill: \d+", b).group(0))
