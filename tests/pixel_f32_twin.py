"""numpy float32 twin of the F32 pixel likelihood (dbot_ros_amd/csrc/rbsensor_kernels.hip: fast_exp, fast_log,
fast_rcp, fast_erfc, pixel_loglik_f32), operation by operation in the order of the source, every intermediate
rounded to float32 where the kernel holds a float.  Test infrastructure.

What differs from the device, and only this:
  * the hardware's exp2 / log2 / rcp units are 1-ulp units; here they are the correctly rounded float32 values
    (computed in binary64, rounded once);
  * fmaf(a, b, c) is float32(a b + c) with the product and the sum in binary64: the product of two float32 is exact
    there, the sum is rounded to binary64 and then to float32 -- a double rounding that can differ from the fused
    result by one float32 ulp only when the binary64 sum lands on a float32 tie, about one operation in 2^29;
  * denormal results of exp2 are kept (the hardware unit flushes them): they are added to tw / D, 30 orders larger.
"""
import numpy as np

F = np.float32
MAX_DEPTH = 6.0


def _fma(a, b, c):
    return (np.asarray(a, F).astype(np.float64) * np.asarray(b, F).astype(np.float64) + np.asarray(c, F).astype(np.float64)).astype(F)


def _exp2(x):
    with np.errstate(under="ignore"):
        return np.exp2(x.astype(np.float64)).astype(F)


def _log2(x):
    return np.log2(x.astype(np.float64)).astype(F)


def _rcp(x):
    return (1.0 / x.astype(np.float64)).astype(F)


def fast_exp(x):
    return _exp2(x * F(1.4426950408889634))


def fast_log(x):
    return F(0.6931471805599453) * _log2(x)


def fast_rcp(x):
    r = _rcp(x)
    return _fma(r, _fma(-x, r, F(1.0)), r)


def fast_erfc(x):
    z = np.abs(x)
    t = _rcp(_fma(F(0.5), z, F(1.0)))
    p = np.full_like(t, F(0.17087277))
    for c in (-0.82215223, 1.48851587, -1.13520398, 0.27886807, -0.18628806, 0.09678418, 0.37409196, 1.00002368, -1.26551223):
        p = _fma(p, t, F(c))
    a = t * fast_exp(p - z * z)
    return np.where(x >= 0, a, F(2.0) - a).astype(F)


def pixel_loglik_f32(obs, depth, prior, tw, ms, sf, lam):
    """-> (term [n] binary64, posterior [n] float32) of pixel_loglik_f32(P, r, prior, o)."""
    o, r, prior = (np.ascontiguousarray(v, dtype=F) for v in (obs, depth, prior))
    lam, twD, omt = F(lam), F(tw / MAX_DEPTH), F(1.0 - tw)
    sigma = _fma(F(sf) * o, o, F(ms))
    is_ = fast_rcp(sigma)
    inv_s2s = F(0.7071067811865476) * is_
    kk = (F(0.7071067811865476) * lam) * sigma
    cv = (F(0.3989422804014327) * omt) * is_
    eo = (F(0.5) * omt * lam) * fast_exp((F(0.5) * lam) * _fma(lam * sigma, sigma, F(-2.0) * o))
    lpbg = fast_log(_fma(F(2.0), eo, twD))
    w = (r - o) * inv_s2s
    pv = _fma(cv, fast_exp(-(w * w)), twD)
    ratio = fast_rcp(F(1.0) - fast_exp(-(r * lam)))
    po = _fma(eo * ratio, fast_erfc(-(w + kk)), twD)
    av = pv * (F(1.0) - prior)
    bv = po * prior
    s = av + bv
    rs = fast_rcp(s)
    qd = bv * rs
    posterior = _fma(rs, _fma(-qd, s, bv), qd)
    term = (fast_log(s) - lpbg).astype(np.float64)
    assert all(v.dtype == F for v in (sigma, is_, inv_s2s, kk, cv, eo, lpbg, w, pv, ratio, po, av, bv, s, rs, qd, posterior))
    return term, posterior


def error_figures(term, post, ref_term, ref_post):
    """(worst, mean, bias) of the term's error and the worst posterior error against the oracle's pixel terms."""
    d = term - ref_term
    return float(np.abs(d).max()), float(np.abs(d).mean()), float(d.mean()), float(np.abs(post.astype(np.float64) - ref_post).max())
