"""The per-pixel Kinect likelihood ON THE DEVICE, value by value.

tests/test_math_cpu.py pins dbot_ros_amd/csrc/rbs_math.h on its HOST build.  Under __HIP_DEVICE_COMPILE__ the kernels
take branches no host build compiles (the Horner literals of exp_nonpos, the hex-coded constants and the classf test of
log_f32, the reciprocal expansions div_f32 / rcp_f64, ocml exp / sqrt in frame_terms, the LDS copy of the tables), and
the F32 pixel model (rbsensor_kernels.hip) exists on the device only.  The other GPU tests see all of it through sums of
thousands of terms.  Here the test build of the library (librbsensor_mi355x_hooks.so) runs those same inline functions
over chosen arguments (rbsensor_probes.hip) and every value is compared:

  a. exp_nonpos, erfc_pos, log_f32 (constant and LDS tables): the bits of the host build of the same source
  b. div_f32: the bits of the correctly rounded float quotient; rcp_f64: 2^-52 relative of the exact reciprocal
  c. frame_terms as stored: entries 0-2 the host's bits, entry 3 (ocml exp against glibc exp) within 3 ulp
  d. the F64 pixel term: the oracle's, pixel by pixel, with the bars of the host build's test
  e. the F32 pixel term: within twice the committed numpy twin's own error against the oracle

The probes exist in the hooks build only, and two builds of the library do not share a process: outside a process that
has loaded the hooks build, the first test here re-runs this file once in a child with RBS_LIB_PATH set to it, and every
test reports its own outcome of that run."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import oracle_binding as ob
import pixel_f32_twin as twin
import pixel_math_cases as cases
import scenarios as sc
from dbot_ros_amd import _capi
from pixel_probes import LAMBDA, PROBE_SYMBOLS, RBS_ERR_INVALID_ARGUMENT, RBS_OK, Probes

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
HOOKS = os.path.join(os.path.dirname(os.path.abspath(_capi.LIB_PATH)), "librbsensor_mi355x_hooks.so")
IN_HOOKS_PROCESS = os.path.abspath(_capi.LIB_PATH) == os.path.abspath(HOOKS)
PLANE_TOL = 2e-6     # the F32 likelihood's bar on occlusion values (tests/test_gpu_f32.py)
_child = {}


def _delegated(request):
    """True: this process has not loaded the hooks build -- the test's outcome is the one of the child run."""
    if IN_HOOKS_PROCESS:
        return False
    if not _child:
        assert os.path.exists(HOOKS), "build() makes librbsensor_mi355x_hooks.so"
        r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-rA", "-m", "gpu", "-p", "no:cacheprovider", __file__],
                           capture_output=True, text=True, timeout=600, env=dict(os.environ, RBS_LIB_PATH=HOOKS))
        _child["out"] = r.stdout[-6000:] + r.stderr[-2000:]
        _child["outcome"] = dict((m.group(2), m.group(1)) for m in re.finditer(r"^(PASSED|FAILED|ERROR) \S+?::(\S+)", r.stdout, re.M))
    assert _child["outcome"].get(request.node.name) == "PASSED", _child["out"]
    return True


@pytest.fixture(scope="module")
def probes(gpu_lib):
    return Probes(HOOKS) if IN_HOOKS_PROCESS else None


@pytest.fixture(scope="module")
def mlib():
    subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "cpp"), "librbs_math_host.so"])
    return C.CDLL(os.path.join(HERE, "cpp", "librbs_math_host.so"))


def _host(lib, fn, x, dtype=np.float64):
    x = np.ascontiguousarray(x, dtype=dtype)
    out = np.empty(x.size)
    getattr(lib, fn)(x.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), C.c_long(x.size))
    return out


def _same_bits(got, ref):
    """Elementwise: the same bits, or NaN on both sides."""
    assert got.dtype == ref.dtype and got.shape == ref.shape
    u = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    return (got.view(u) == ref.view(u)) | (np.isnan(got) & np.isnan(ref))


def _report(what, ok, *show):
    """Every figure is printed before it is asserted."""
    bad = np.flatnonzero(~ok)
    print(f"{what}: {bad.size} of {ok.size} differ" + "".join(f"\n    {[v[i] for v in show]}" for i in bad[:8]))
    return bad.size == 0


def _model(params):
    om, cam, P = sc.make_scene(("m1_l2",), 80, 60, max_particles=1)
    for k, v in params.items():
        setattr(P.kinect, k, v)
    return om, cam, P, (P.kinect.tail_weight, P.kinect.model_sigma, P.kinect.sigma_factor)


# ---------------------------------------------------------------- the entry points themselves
def test_probes_refuse_bad_arguments(request, probes):
    if _delegated(request):
        return
    lib = probes.lib
    assert all(hasattr(lib, s) for s in PROBE_SYMBOLS)
    d, f = np.ones(4), np.ones(4, dtype=np.float32)
    od, of, o4 = np.full(4, 7.0), np.full(4, 7.0, dtype=np.float32), np.full(16, 7.0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    m = [C.c_double(v) for v in (0.01, 0.003, 0.0014247, LAMBDA)]
    calls = {
        "rbs_test_exp_nonpos": lambda a, b, n: lib.rbs_test_exp_nonpos(a and p(d), b and p(od), C.c_int64(n)),
        "rbs_test_erfc_pos": lambda a, b, n: lib.rbs_test_erfc_pos(a and p(d), b and p(od), C.c_int64(n), C.c_int32(1)),
        "rbs_test_log_f32": lambda a, b, n: lib.rbs_test_log_f32(a and p(f), b and p(od), C.c_int64(n), C.c_int32(1)),
        "rbs_test_rcp_f64": lambda a, b, n: lib.rbs_test_rcp_f64(a and p(d), b and p(od), C.c_int64(n)),
        "rbs_test_div_f32": lambda a, b, n: lib.rbs_test_div_f32(a and p(f), a and p(f), b and p(of), C.c_int64(n)),
        "rbs_test_frame_terms": lambda a, b, n: lib.rbs_test_frame_terms(a and p(f), C.c_int64(n), *m, b and p(o4)),
        "rbs_test_pixel_f64": lambda a, b, n: lib.rbs_test_pixel_f64(a and p(f), p(f), p(f), C.c_int64(n), *m, b and p(od), p(of)),
        "rbs_test_pixel_f32": lambda a, b, n: lib.rbs_test_pixel_f32(a and p(f), p(f), p(f), C.c_int64(n), *m, p(od), b and p(of)),
    }
    assert sorted(calls) == sorted(PROBE_SYMBOLS)
    for name, call in calls.items():
        assert call(None, True, 4) == RBS_ERR_INVALID_ARGUMENT, name
        assert call(True, None, 4) == RBS_ERR_INVALID_ARGUMENT, name
        assert call(True, True, -1) == RBS_ERR_INVALID_ARGUMENT, name
        assert call(True, True, 0) == RBS_OK, name
    assert np.all(od == 7.0) and np.all(of == 7.0) and np.all(o4 == 7.0)      # nothing was written


# ---------------------------------------------------------------- a. device against the host build, bit for bit
def test_exp_nonpos_has_the_bits_of_the_host_build(request, probes, mlib):
    """The Horner literals against kExpPoly, the device rint / ldexp against libm's: the whole argument set of
    test_math_cpu, the special arguments, and the gradual underflow between -708 and -745."""
    if _delegated(request):
        return
    under = -np.random.default_rng(10).uniform(708.0, 745.2, 4000)
    x = np.concatenate([cases.exp_args(), cases.EXP_TAIL, [0.0, -708.0, -745.0, -745.2], under])
    dev, host = probes.exp_nonpos(x), _host(mlib, "rbsm_exp_nonpos", x)
    same = _report("exp_nonpos device / host", _same_bits(dev, host), x, dev, host)
    # the far tail: gradual underflow and the clamp, never NaN / negative (test_exp_nonpos)
    tail = dev[x <= -745.0]
    assert tail.size >= 5 and np.all(tail >= 0) and np.all(tail <= 1e-320)
    assert dev[x == 0.0][0] == 1.0
    # the subnormal results: one rounding to the subnormal grid (spacing 2^-1074) of a value good to 1e-15
    sub = (x < -708.0) & (x >= -745.2)
    ref = np.exp(x[sub])
    err = np.abs(dev[sub] - ref) - 1e-15 * ref
    print("exp_nonpos device underflow: worst error beyond 1e-15 relative, in subnormal spacings:", err.max() / 5e-324)
    assert np.all(err <= 5e-324)
    assert same


@pytest.mark.parametrize("lds", [0, 1], ids=["constant_tables", "lds_tables"])
def test_erfc_pos_has_the_bits_of_the_host_build(request, probes, mlib, lds):
    if _delegated(request):
        return
    z = np.concatenate([cases.erfc_args(), [np.nan, np.inf, 1e300, 6.0, np.nextafter(6.0, 0.0), float.fromhex("0x1.7ffffffffffp+2"), 5.875, 0.0]])
    dev, host = probes.erfc_pos(z, lds), _host(mlib, "rbsm_erfc_pos", z)
    assert _report("erfc_pos device / host", _same_bits(dev, host), z, dev, host)


@pytest.mark.parametrize("lds", [0, 1], ids=["constant_tables", "lds_tables"])
def test_log_f32_has_the_bits_of_the_host_build(request, probes, mlib, lds):
    """The four hex-coded constants against 0.2, 1/3, kLn2Hi, kLn2Lo; the classf test against the comparison."""
    if _delegated(request):
        return
    tiny = np.finfo(np.float32).tiny
    odd = np.array(cases.LOG_ODD + [1e-45, 1e-39, -0.0, -np.inf, -1e-40], dtype=np.float32)
    edge = np.array([np.nextafter(np.float32(tiny), np.float32(0)), tiny, np.nextafter(np.float32(tiny), np.float32(1))], dtype=np.float32)
    x = np.concatenate([cases.log_args(), odd, edge])
    dev, host = probes.log_f32(x, lds), _host(mlib, "rbsm_log_f32", x, np.float32)
    assert _report("log_f32 device / host", _same_bits(dev, host), x, dev, host)
    o = dev[cases.log_args().size:]
    assert o[0] == -np.inf and o[1] == np.inf and np.isnan(o[2]) and np.isnan(o[3])


# ---------------------------------------------------------------- b. the device-only expansions against exact arithmetic
def _pixel_quotients(o, r, prior, tw, ms, sf, lam=LAMBDA):
    """The operands of the two float divisions of rbsm::pixel_loglik_f64, (b, a + b) and (a + b, p_bg), restated in
    numpy binary64 with the header's roundings to float (libm for exp / erf: the float operands are the kernel's
    except on the few pixels where a rounding flips)."""
    from scipy.special import erf
    o, r, pd = (v.astype(np.float64) for v in (o, r, prior))
    sigma = ms + sf * o * o
    inv = 1.0 / (np.sqrt(2.0) * sigma)
    kk = lam * sigma / np.sqrt(2.0)
    eo = 0.5 * (1.0 - tw) * lam * np.exp(0.5 * lam * (-2.0 * o + lam * sigma * sigma))
    twD, cv0 = tw / 6.0, (1.0 - tw) / np.sqrt(np.pi)
    w = (r - o) * inv
    pv = cv0 * inv * np.exp(-(w * w)) + twD
    po = eo / (1.0 - np.exp(-lam * r)) * (1.0 + erf(w + kk)) + twD
    a, b = (pv * (1.0 - pd)).astype(np.float32), (po * pd).astype(np.float32)
    return b, a + b, (2.0 * eo + twD).astype(np.float32)


def test_div_f32_is_the_correctly_rounded_quotient(request, probes):
    """div_f32's stated contract: the bits of the IEEE float division (numpy's float32 division) for normal operands
    and a normal or zero quotient."""
    if _delegated(request):
        return
    rng = np.random.default_rng(11)

    def normals(n, lo=-60, hi=60):
        return (rng.choice([-1.0, 1.0], n) * rng.uniform(1.0, 2.0, n) * np.exp2(rng.integers(lo, hi + 1, n))).astype(np.float32)

    A, B = [normals(1_000_000)], [normals(1_000_000)]
    same = normals(5000)
    A += [same, np.zeros(5000, dtype=np.float32)]                    # a == b; a = 0
    B += [same, normals(5000)]
    i, j = rng.integers(-60, 61, 5000), rng.integers(-60, 61, 5000)
    A += [np.exp2(i).astype(np.float32), normals(5000), np.exp2(i).astype(np.float32)]   # powers of two
    B += [np.exp2(j).astype(np.float32), np.exp2(j).astype(np.float32), normals(5000)]
    # quotients next to a float (b q rounded) and next to a rounding tie (b (q + ulp(q) / 2) rounded)
    q, b = normals(100_000, -20, 20), normals(100_000, -20, 20)
    mid = q.astype(np.float64) + 0.5 * np.spacing(q).astype(np.float64)
    A += [(b.astype(np.float64) * q.astype(np.float64)).astype(np.float32), (b.astype(np.float64) * mid).astype(np.float32)]
    B += [b, b]
    # the quotients the pixel term forms
    for params in cases.PARAM_SETS:
        pb, psum, pbg = _pixel_quotients(*cases.pixels(200_000, 5), *_model(params)[3])
        A += [pb, psum]
        B += [psum, pbg]
    a, b = np.concatenate(A), np.concatenate(B)
    tiny = np.finfo(np.float32).tiny
    with np.errstate(all="raise"):
        ref = a / b
    assert np.all(np.abs(b) >= tiny) and np.all((np.abs(a) >= tiny) | (a == 0)) and np.all((np.abs(ref) >= tiny) | (ref == 0))
    assert np.all(np.isfinite(ref))
    dev = probes.div_f32(a, b)
    assert _report("div_f32 device / IEEE", _same_bits(dev, ref), a, b, dev, ref)


def test_rcp_f64_is_within_one_ulp(request, probes):
    """v_rcp_f64 + two Newton steps: relative error <= 2^-52 against the exact reciprocal, over the arguments
    depth_term hands it (1 - exp(-lam r), r in [0.05, 6]) and over random normals."""
    if _delegated(request):
        return
    assert np.finfo(np.longdouble).nmant >= 63
    rng = np.random.default_rng(12)
    r = np.concatenate([rng.uniform(0.05, 6.0, 500_000), np.float32([0.05, 6.0]).astype(np.float64)])
    x = np.concatenate([1.0 - np.exp(-LAMBDA * r),
                        rng.choice([-1.0, 1.0], 500_000) * rng.uniform(1.0, 2.0, 500_000) * np.exp2(rng.integers(-1000, 1001, 500_000)),
                        [1.0, 2.0, 0.5, -1.0, 3.0, np.nextafter(1.0, 2.0), np.nextafter(2.0, 1.0)]])
    dev = probes.rcp_f64(x)
    xl = x.astype(np.longdouble)
    rel = np.abs((dev.astype(np.longdouble) - 1 / xl) * xl).astype(np.float64)
    print("rcp_f64 device: worst relative error in units of 2^-52:", rel.max() * 2.0 ** 52, "wrongly rounded:", (dev != 1.0 / x).mean())
    assert np.all(np.isfinite(dev)) and rel.max() <= 2.0 ** -52


# ---------------------------------------------------------------- c. frame_terms as stored
@pytest.mark.parametrize("params", cases.PARAM_SETS, ids=["default_model", "narrow_model"])
def test_frame_terms_as_stored(request, probes, mlib, params):
    """The aux entry of a frame pixel as frame_aux_kernel stores it.  Entries 0, 1, 2 are IEEE-exact + * / sqrt with
    contraction off: the host's bits.  Entry 3: the argument of exp has the host's bits, ocml's exp and glibc's are
    each within 1 ulp of exp, and two rounded products follow: within 3 ulp of the host's value."""
    if _delegated(request):
        return
    tw, ms, sf = _model(params)[3]
    rng = np.random.default_rng(13)
    obs = np.concatenate([rng.uniform(0.3, 6.0, 200_000), [0.3, 6.0, np.nextafter(np.float32(0), np.float32(1))]]).astype(np.float32)
    dev = probes.frame_terms(obs, tw, ms, sf)
    host = np.empty((obs.size, 4))
    mlib.rbsm_frame_terms(obs.ctypes.data_as(C.c_void_p), C.c_long(obs.size), C.c_double(tw), C.c_double(ms), C.c_double(sf), C.c_double(LAMBDA),
                          host.ctypes.data_as(C.c_void_p))
    assert np.array_equal(host[:, 2], obs.astype(np.float64))
    exact = all([_report(f"frame_terms[{k}] device / host", _same_bits(dev[:, k], host[:, k]), obs, dev[:, k], host[:, k]) for k in range(3)])
    ulps = np.abs(dev[:, 3] - host[:, 3]) / np.spacing(host[:, 3])
    print("frame_terms[3] device / host: worst", ulps.max(), "ulp, differing", (ulps != 0).mean())
    assert np.all(np.isfinite(dev)) and ulps.max() <= 3.0
    assert exact


# ---------------------------------------------------------------- d. the F64 pixel term
def _edge_pixels(tw, ms, sf, lam=LAMBDA):
    """20 000 (observation, rendered depth, prior) triples at the edges of the F64 pixel term: the priors 0, 1, float
    eps and 1 - 2^-24; w + k within 1e-9 of 0 (where 1 + erf switches between erfc and 2 - erfc) and one float of r to
    either side; |w + k| from 5.9 to 7 (across the erfc table's clamp at 6); |w| so large that -w^2 < -745 (exp_nonpos
    past its underflow); r = 0.05 m, where g(r) is largest.  Filled up with ordinary pixels."""
    rng = np.random.default_rng(14)
    f32 = np.float32
    s2 = np.sqrt(2.0)

    def sigma_of(o):
        return ms + sf * o.astype(np.float64) ** 2

    def r_for_x(o, x):   # the rendered depth at which w + k = x (before r is rounded to float)
        sg = sigma_of(o)
        return (o.astype(np.float64) + (x - lam * sg / s2) * s2 * sg).astype(f32)

    def x_of(o, r):
        sg = sigma_of(o)
        return (r.astype(np.float64) - o.astype(np.float64)) / (s2 * sg) + lam * sg / s2

    O, R, Pr = [], [], []
    o, r, _ = cases.pixels(5000, 15)
    O.append(o); R.append(r); Pr.append(np.tile(f32([0.0, 1.0, np.finfo(f32).eps, 1.0 - 2.0 ** -24]), 1250))
    # the sign switch: r is a float, so x moves in steps of ~1e-5 -- the candidates that land within 1e-9, and their neighbours
    o = rng.uniform(0.3, 3.0, 2_000_000).astype(f32)
    r = r_for_x(o, 0.0)
    hit = np.flatnonzero(np.abs(x_of(o, r)) <= 1e-9)[:1000]
    assert hit.size >= 100, hit.size
    o, r = o[hit], r[hit]
    O += [o, o, o]; R += [r, np.nextafter(r, f32(0)), np.nextafter(r, f32(10))]; Pr += [rng.uniform(0, 1, o.size).astype(f32)] * 3
    # across the erfc clamp, both signs
    o = rng.uniform(0.5, 3.0, 4000).astype(f32)
    x = rng.choice([-1.0, 1.0], 4000) * np.concatenate([rng.uniform(5.9, 7.0, 3000), rng.uniform(5.99, 6.01, 1000)])
    O.append(o); R.append(r_for_x(o, x)); Pr.append(rng.uniform(0, 1, 4000).astype(f32))
    # exp_nonpos past -745: |w| from 27.3 up (in front of the object while that leaves r above 0.05 m, else behind it)
    o = rng.uniform(0.5, 3.0, 3000).astype(f32)
    w = rng.uniform(27.3, 80.0, 3000)
    d = w * s2 * sigma_of(o)
    r = np.where((rng.random(3000) < 0.5) & (o - d > 0.05), o - d, o + d).astype(f32)
    assert np.all(((r.astype(np.float64) - o) / (s2 * sigma_of(o))) ** 2 > 745.0)
    O.append(o); R.append(r); Pr.append(rng.uniform(0, 1, 3000).astype(f32))
    # r = 0.05 m: the object right there, the background behind it
    r = np.full(2000, 0.05, dtype=f32)
    o = np.concatenate([0.05 + sigma_of(r[:1000]) * rng.normal(0, 1.5, 1000), 0.05 + rng.uniform(0.01, 3.0, 1000)]).astype(f32)
    O.append(o); R.append(r); Pr.append(rng.uniform(0, 1, 2000).astype(f32))
    n = sum(v.size for v in O)
    o, r, p = cases.pixels(20_000 - n, 16)
    O.append(o); R.append(r); Pr.append(p)
    o, r, p = np.concatenate(O), np.concatenate(R), np.concatenate(Pr)
    assert o.size == 20_000 and o.dtype == r.dtype == p.dtype == f32 and np.all(r > 0) and np.all(o > 0)
    return o, r, p


@pytest.mark.parametrize("params", cases.PARAM_SETS, ids=["default_model", "narrow_model"])
@pytest.mark.parametrize("batch", ["pixels", "edges"])
def test_f64_pixel_term_matches_the_oracle_pixel_by_pixel(request, probes, params, batch):
    """pixel_loglik<false> on the device (frame_aux_kernel's stored entry, depth_term, pixel_loglik_f64, the tables in
    LDS) against the oracle's (libm) pixel term, with the bars test_math_cpu holds the host build to."""
    if _delegated(request):
        return
    om, cam, P, (tw, ms, sf) = _model(params)
    orc = ob.Oracle(om, cam, P, max_particles=1, mode=ob.EAGER)
    o, r, prior = cases.pixels(1_000_000, 5) if batch == "pixels" else _edge_pixels(tw, ms, sf)
    ref_ll, ref_post = orc.pixel_terms(o, r, prior)
    ll, post = probes.pixel_f64(o, r, prior, tw, ms, sf)
    d = np.abs(ll - ref_ll)
    print(f"F64 pixel term, {batch}: worst {d.max():.3e}, outside 2.5e-16 + 2 ulp {(d > 2.5e-16 + 2 * np.spacing(np.abs(ref_ll))).mean():.2e}, "
          f"posterior differing {(post != ref_post).mean():.2e}")
    cases.check_pixel_terms(ll, post, ref_ll, ref_post)


# ---------------------------------------------------------------- e. the F32 pixel term
@pytest.mark.parametrize("params", cases.PARAM_SETS, ids=["default_model", "narrow_model"])
def test_f32_pixel_term_stays_within_twice_the_twin_error(request, probes, params):
    """pixel_loglik_f32 on the device against the oracle's pixel term.  The bar is the committed numpy twin's own
    worst (and mean) error against the oracle on the same pixels, times 2: the twin performs the kernel's float32
    operations in the kernel's order with correctly rounded exp2 / log2 / rcp, the hardware's are 1-ulp units, which
    roughly doubles those steps' share.  Posterior: PLANE_TOL, absolute."""
    if _delegated(request):
        return
    om, cam, P, (tw, ms, sf) = _model(params)
    orc = ob.Oracle(om, cam, P, max_particles=1, mode=ob.EAGER)
    o, r, prior = cases.pixels(400_000, 5)
    ref_ll, ref_post = orc.pixel_terms(o, r, prior)
    t_worst, t_mean, t_bias, t_post = twin.error_figures(*twin.pixel_loglik_f32(o, r, prior, tw, ms, sf, LAMBDA), ref_ll, ref_post)
    ll, post = probes.pixel_f32(o, r, prior, tw, ms, sf)
    assert np.all(np.isfinite(ll)) and np.all(np.isfinite(post))
    worst, mean, bias, pworst = twin.error_figures(ll, post, ref_ll, ref_post)
    print(f"F32 pixel term: twin worst {t_worst:.3e} mean {t_mean:.3e} bias {t_bias:+.3e} posterior {t_post:.3e}; "
          f"device worst {worst:.3e} mean {mean:.3e} bias {bias:+.3e} posterior {pworst:.3e}")
    assert worst <= 2 * t_worst and mean <= 2 * t_mean
    assert pworst <= PLANE_TOL
