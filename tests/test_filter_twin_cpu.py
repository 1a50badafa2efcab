"""tests/filter_twin.py, the plain reference tests/test_gpu_filter_kernels.py holds the particle filter's kernels to,
against what it can be held to without a device: the published Philox known answers, the moments of its normals, and
the project's own checker (oracle/tracker_oracle.c) over whole frames."""
import numpy as np
import pytest

import filter_twin as ft
import oracle_binding as ob
import scenarios as sc
from dbot_ros_amd import pose, synth
from dbot_ros_amd.tracker import ObjectTransitionBuilder


def _model_init(om, nb):
    """The synthetic truth's first poses as a model-coordinate state."""
    init = np.zeros(12 * nb)
    for b in range(nb):
        Rt = synth.truth_pose(nb, frame=0)[b]
        init[12 * b + 3:12 * b + 6] = pose.matrix_to_rotvec(Rt[:9].reshape(3, 3))
        init[12 * b:12 * b + 3] = Rt[9:]
    return init


def _words(text):
    return tuple(int(w, 16) for w in text.split())


# Random123's known answers for philox4x32_10 (kat_vectors): counter words, key words, output words
KNOWN_ANSWERS = [
    ("00000000 00000000 00000000 00000000", "00000000 00000000", "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff", "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0", "d16cfe09 94fdcceb 5001e420 24126ea1"),
]


@pytest.mark.parametrize("ctr,key,out", KNOWN_ANSWERS, ids=["zeros", "ones", "pi"])
def test_philox_reproduces_the_random123_known_answers(ctr, key, out):
    c, k = _words(ctr), _words(key)
    seed, lo, hi = k[1] << 32 | k[0], c[1] << 32 | c[0], c[3] << 32 | c[2]
    assert ft.philox4x32_10(seed, hi, lo) == _words(out)
    assert tuple(int(w[0]) for w in ft.philox_words(seed, hi, np.array([lo], dtype=np.uint64))) == _words(out)


def test_the_array_form_is_the_integer_form():
    rng = np.random.default_rng(0)
    for _ in range(20):
        seed, hi = (int(v) for v in rng.integers(0, 2 ** 64, 2, dtype=np.uint64))
        lo = rng.integers(0, 2 ** 64, 50, dtype=np.uint64)
        got = np.stack(ft.philox_words(seed, hi, lo), axis=1)
        ref = np.array([ft.philox4x32_10(seed, hi, int(v)) for v in lo], dtype=np.uint64)
        assert np.array_equal(got, ref)


def test_counter_layout_and_uniform_range():
    """The frame number sits above eight bits of sampling block (and wraps at 64 bits); u01 keeps the top 53 bits."""
    assert ft.stream_counter(1, 2) == 0x102 and ft.stream_counter(2 ** 24 + 3, 0) == (2 ** 24 + 3) << 8
    assert ft.stream_counter(2 ** 24 + 3, 0) >> 32 == 1 and ft.stream_counter(2 ** 60, 5) == 5
    assert ft.u01(0, 0) == 0.0 and ft.u01(0xFFFFFFFF, 0xFFFFFFFF) == 1.0 - 2.0 ** -53 and ft.u01(0x80000000, 0) == 0.5
    assert ft.u01(0, 0x7FF) == 0.0 and ft.u01(0, 0x800) == 2.0 ** -53
    seed = 0x0123456789ABCDEF
    w = ft.philox4x32_10(seed ^ ft.UNIFORM_KEY_XOR, ft.stream_counter(7, 1), 5)
    assert ft.device_uniforms(seed, 7, 1, 6)[5] == ft.u01(w[0], w[1])
    w = ft.philox4x32_10(seed, ft.stream_counter(7, 1), 5 << 2 | 2)
    rad = np.sqrt(-2.0 * np.log(1.0 - ft.u01(w[0], w[1])))
    assert ft.device_normals(seed, 7, 1, 6)[5, 4] == rad * np.cos(ft.TWO_PI * ft.u01(w[2], w[3]))
    assert ft.device_normals(seed, 7, 1, 6)[5, 5] == rad * np.sin(ft.TWO_PI * ft.u01(w[2], w[3]))


def test_a_million_normals_have_the_moments_of_a_standard_normal():
    """Mean, variance and fourth moment within five standard errors of 0, 1 and 3: Var x = 1, Var x^2 = 2, Var x^4 = 96."""
    x = ft.device_normals(0x9E3779B97F4A7C15, 3, 1, 166_667).ravel()[:1_000_000]
    n = x.size
    assert n == 1_000_000 and np.all(np.isfinite(x))
    figures = (x.mean(), (x ** 2).mean() - 1.0, (x ** 4).mean() - 3.0)
    print("normals: mean, variance - 1, fourth moment - 3:", figures)
    for got, var in zip(figures, (1.0, 2.0, 96.0)):
        assert abs(got) <= 5.0 * np.sqrt(var / n)
    u = ft.device_uniforms(0x9E3779B97F4A7C15, 3, 1, 1_000_000)
    assert u.min() >= 0.0 and u.max() < 1.0 and abs(u.mean() - 0.5) <= 5.0 * np.sqrt(1.0 / 12.0 / n)


def test_parents_at_the_edges_of_the_cdf():
    cdf = np.array([0.25, 0.25, 0.5, 1.0 - 2.0 ** -52])
    u = np.array([0.0, 0.25, np.nextafter(0.25, 0), 0.5, cdf[3], np.nextafter(1.0, 0.0)])
    assert ft.parents_of(cdf, u).tolist() == [0, 2, 0, 3, 3, 3]


@pytest.mark.parametrize("meshes,n", [(("m1_l2",), 48), (("m1_l2", "box12"), 64)])
def test_twin_frames_match_the_c_oracle_tracker(meshes, n):
    """The twin's whole step against oracle/tracker_oracle.c, both driving oracle sensors with the same normals and
    uniforms: four frames at 48 and 2 x 32 particles, the bars of test_host_tracker_mirror_matches_the_c_oracle_tracker."""
    nb = len(meshes)
    per = n // nb
    om, cam, P = sc.make_scene(meshes, 80, 60, max_particles=n)
    o1 = ob.Oracle(om, cam, P, max_particles=per, mode=ob.EAGER)
    o2 = ob.Oracle(om, cam, P, max_particles=per, mode=ob.EAGER)
    trans = ObjectTransitionBuilder(ObjectTransitionBuilder.Parameters(part_count=nb)).build()
    twin = ft.TwinTracker(o1, per, nb, trans.sigma, trans.vf, 2.0)
    ref = ob.OracleTracker(o2, per, trans.sigma, trans.vf, 2.0)
    init = _model_init(om, nb)
    twin.initialize(init)
    ref.initialize(init)
    draw, rng = np.random.default_rng(1), np.random.default_rng(9)
    for k in range(1, 5):
        frame = synth.make_frame(o1.render_depth(synth.truth_pose(nb, frame=k)), 60, 80, rng, occluder=False)
        normals, uniforms = draw.standard_normal((nb, per, 6)), draw.random((nb, per))
        et = twin.track(frame, normals, uniforms)
        er, nres = ref.track(frame, normals, uniforms)
        assert np.abs(et - er).max() <= 1e-12
        p, w, idx = ref.get_state()
        assert np.abs(p - twin.particles).max() <= 1e-12 and np.array_equal(idx, twin.indices)
        assert np.abs(w - twin.log_weights).max() <= 1e-9 and nres == twin.n_resamplings
    assert twin.n_resamplings >= 1
