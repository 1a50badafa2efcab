"""The numpy float32 twin of the F32 pixel likelihood (tests/pixel_f32_twin.py) against the oracle's pixel term,
WITHOUT a GPU: what the F32 model's arithmetic costs when every hardware unit is correctly rounded.
tests/test_gpu_pixel_math.py holds the device to twice the figures measured here.

Bars, from the arithmetic (eps = 2^-24):
  term      the term is log(sum) - log(p_bg).  Each log is 0.6931f * log2: two roundings of a value of magnitude <= 7
            (sum and p_bg lie in [1e-3, 1.4e2]), 7 * 1.5 eps = 6e-7 each.  The relative error of sum is led by the
            Gaussian's exponent: w carries about 2.5 eps relative, w^2 about 5.5 eps, so exp(-w^2) is off by
            5.5 eps w^2 relative, weighted by the Gaussian's share of the sum -- with c_v / (tw / D) ~ 6e4 that product
            peaks near w^2 = 8: 2.5e-6.  erfcc's own 1.2e-7 and the remaining dozen roundings: under 1e-6.
            Together: <= 5e-6 on every pixel.  Mean: independent roundings do not line up, a tenth of that, 5e-7;
            bias: <= 1e-7 in magnitude (the sum over 5 000 pixels is held to 1e-5 relative elsewhere).
  posterior PLANE_TOL of tests/test_gpu_f32.py, 2e-6 absolute: b / sum with both good to a few eps relative.
Measured: worst 3.0e-6 / 3.1e-6, mean 1.8e-7 / 1.6e-7, bias +3.0e-8 / +3.6e-8, posterior 6.6e-7 / 6.3e-7 (default /
narrow model)."""
import numpy as np
import pytest

import oracle_binding as ob
import pixel_f32_twin as twin
import pixel_math_cases as cases
import scenarios as sc

PLANE_TOL = 2e-6


@pytest.mark.parametrize("params", cases.PARAM_SETS, ids=["default_model", "narrow_model"])
def test_f32_twin_against_the_oracle_pixel_by_pixel(params):
    om, cam, P = sc.make_scene(("m1_l2",), 80, 60, max_particles=1)
    for k, v in params.items():
        setattr(P.kinect, k, v)
    orc = ob.Oracle(om, cam, P, max_particles=1, mode=ob.EAGER)
    o, r, prior = cases.pixels(400_000, 5)
    ref_ll, ref_post = orc.pixel_terms(o, r, prior)
    ll, post = twin.pixel_loglik_f32(o, r, prior, P.kinect.tail_weight, P.kinect.model_sigma, P.kinect.sigma_factor, np.log(2.0))
    assert ll.dtype == np.float64 and post.dtype == np.float32
    assert np.all(np.isfinite(ll)) and np.all(np.isfinite(post))
    worst, mean, bias, pworst = twin.error_figures(ll, post, ref_ll, ref_post)
    print(f"F32 twin: term worst {worst:.3e} mean {mean:.3e} bias {bias:+.3e}; posterior worst {pworst:.3e}")
    assert worst <= 5e-6 and mean <= 5e-7 and abs(bias) <= 1e-7
    assert pworst <= PLANE_TOL
    assert np.all((post >= 0) & (post <= 1))

