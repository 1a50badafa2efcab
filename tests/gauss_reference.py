"""An extended-precision reference for the Gaussian tracker's reduced moments, with an
error bar derived from the device's operation order.

rbs_gauss_moments_kernel / rbs_gauss_reduce_kernel turn the sigma points' depths and the staged frame into
NE = 6B(6B+1)/2 + 6B sums: the upper triangle of Lambda - I (row-major, a <= b), then eta.  moments() recomputes
every pixel's y_hat, P, h, R, b and pi from the float32 planes in np.longdouble (x86 80-bit, 64-bit mantissa),
forms the terms t_ie = (pi_i h_ia) h_ib and (pi_i h_ia) r_i, and sums them pairwise in extended precision.

The bar (why |device_e - reference_e| <= bar_e must hold).  u = 2^-53.  The kernel builds with -ffp-contract=off,
so every operation of Appendix G's per-pixel formulas is one binary64 rounding, in the order the kernel writes
them.  _Val below evaluates that same order on exact values and carries, beside each value x, a first-order
bound u*E_x on the error of the device's binary64 x (running error analysis):

    x + y, x - y   E = E_x + E_y + |z|               x * y   E = |y| E_x + |x| E_y + |z|
    x / y          E = (E_x + |z| E_y) / |y| + |z|   max(x, c)  E = max(E_x, E_c)  (max is 1-Lipschitz)
    log x          E = E_x / |x| + 2 |z|             exp x   E = |z| E_x + 2 |z|   (1 ulp: the HIP math library)
    so 1 / (1 + exp x) = b has E = b (1 - b) (E_x + 2) + 2b.

The host's constants (w_m0, w_c0, W, 1/(2 sqrt c), fg^2, bg^2, log_tail, and the literal 2 pi) enter with the
bound of their own binary64 evaluation from the parameters.  A pixel's term error is then u*kappa_ie*|t_ie| with
kappa_ie = E_t / |t_ie|, its per-pixel condition count.  It is large exactly where the arithmetic is
ill-conditioned: the cancellation in R = P - |h|^2 (E_R ~ E_P, |R| small: kappa ~ P / R), the logistic's
sensitivity (E_b = b (1 - b) (E_x + 2) + 2b with x = log_tail - lg, E_x ~ |log_tail| + |lg| + |r| E_r / P), the residual
r = y - y_hat for the eta entries (E_r ~ |y_hat| (2 NP + 4)), and a small constant for everything else.

The sums.  Thread e of a moments block adds its block's staged terms in pixel order: 256 per pass over the union
rectangle, ceil(n_u / 65536) passes (256 blocks of 256 pixels), so L = 256 ceil(n_u / 65536) additions; the
reduction adds the 256 block partials in block order.  Every term goes through at most L + 256 roundings, so

    bar_e = u sum_i kappa_ie |t_ie| + (L + 256) u sum_i |t_ie|        (first order; n_u <= rows * cols)

plus the reference's own error, the same expression with 2^-64 and ceil(log2 n) + 8 additions (pairwise
summation), and 16 * 2^-1074 per pixel for terms that underflow.  The neglected second-order terms are below
(u kappa)^2 relative; moments() refuses a pixel with u kappa > 1e-4.  An overflowing exponent gives b = 0
exactly, as the kernel's exp overflows to inf (Appendix G); where the exponent lies within its own error bound
of the overflow threshold either answer is allowed.

float64_moments() is a plain binary64 evaluation in the twin's order (tests/gauss_twin.py) summed sequentially in
pixel order, with switches that break it on purpose: tests/test_gaussian_moments_cpu.py shows that the bar holds
it and that each broken version leaves it."""
import numpy as np

U = 2.0 ** -53
U_LD = 2.0 ** -64
LD = np.longdouble
LN_DBL_MAX = float(np.log(np.finfo(np.float64).max))   # exp(x) overflows to inf beyond this
TWO_PI = 2 * np.arccos(LD(-1))
GRID_PX = 256 * 256                                   # pixels one pass of the moments grid covers


def require_extended():
    """The reference needs the x86 80-bit extended type; anything else fails loudly."""
    fi = np.finfo(np.longdouble)
    if fi.nmant != 63 or fi.nexp != 15:
        raise AssertionError(f"np.longdouble is not x86 80-bit extended precision (nmant {fi.nmant}, nexp {fi.nexp})")


class _Val:
    """An exact value (np.longdouble) and E, the first-order bound on the device's error in units of u."""
    __slots__ = ("v", "e")

    def __init__(self, v, e):
        self.v, self.e = v, e

    @staticmethod
    def exact(v):
        v = np.asarray(v, dtype=LD)
        return _Val(v, np.zeros(v.shape))

    def _mag(self):
        return np.abs(self.v).astype(np.float64)

    def __add__(self, o):
        z = self.v + o.v
        return _Val(z, self.e + o.e + np.abs(z).astype(np.float64))

    def __sub__(self, o):
        z = self.v - o.v
        return _Val(z, self.e + o.e + np.abs(z).astype(np.float64))

    def __mul__(self, o):
        z = self.v * o.v
        return _Val(z, o._mag() * self.e + self._mag() * o.e + np.abs(z).astype(np.float64))

    def __truediv__(self, o):
        z = self.v / o.v
        az = np.abs(z).astype(np.float64)
        return _Val(z, (self.e + az * o.e) / o._mag() + az)


def _vmax(x, c):
    return _Val(np.maximum(x.v, c.v), np.maximum(x.e, c.e))


def _vlog(x):
    z = np.log(x.v)
    return _Val(z, x.e / x._mag() + 2.0 * np.abs(z).astype(np.float64))


def _vlogistic(x):
    """1 / (1 + exp x) as the kernel evaluates it: exp (E = |e^x| E_x + 2 |e^x|), + 1, 1 / (.) -- which composes to
    E = b (1 - b) (E_x + 2) + 2 b, written out so that no intermediate overflows."""
    with np.errstate(over="ignore"):
        z = LD(1) / (LD(1) + np.exp(x.v))
    bz = z.astype(np.float64)
    return _Val(z, bz * (1.0 - bz) * (x.e + 2.0) + 2.0 * bz)


def _host_constants(params, B):
    """The host's binary64 constants (rbs_gauss_create / track_impl), exact and with their bounds."""
    D, NP = 12 * B, 6 * B
    one, two = _Val.exact(1.0), _Val.exact(2.0)
    a = _Val.exact(params.ut_alpha)
    a2 = a * a
    wm0 = one - one / a2
    wc0 = ((wm0 + one) - a2) + two
    c = a2 * _Val.exact(float(D))
    w = one / (two * c)
    sc = np.sqrt(c.v)
    sqrtc = _Val(sc, c.e / (2.0 * c._mag()) * np.abs(sc).astype(np.float64) + np.abs(sc).astype(np.float64))   # sqrt: correctly rounded
    inv2sqrtc = one / (two * sqrtc)
    fg, bg = _Val.exact(params.fg_noise_std), _Val.exact(params.bg_noise_std)
    k = dict(wm0=wm0, wc0=wc0, w=w, inv2sqrtc=inv2sqrtc, fg2=fg * fg, bg2=bg * bg, extra=_Val.exact(2.0 * NP),
             two_pi=_Val(TWO_PI, np.float64(TWO_PI)), half=_Val.exact(0.5), one=one)
    if params.tail_weight > 0.0:
        tw = _Val.exact(params.tail_weight)
        k["log_tail"] = _vlog(tw / (_Val.exact(params.uniform_tail_max) - _Val.exact(params.uniform_tail_min))) - _vlog(one - tw)
    return k


class Moments:
    """value [NE] (upper triangle of Lambda - I row-major, then eta), bar [NE], and per-pixel facts the tests assert."""

    def __init__(self, value, bar, abs_sum, counts, NP):
        self.value, self.bar, self.abs_sum, self.counts, self.NP = value, bar, abs_sum, counts, NP

    def excess(self, got):
        """max over entries of |got - value| / bar (0 / 0 := 0); <= 1 means inside the bar."""
        d = np.abs(np.asarray(got, dtype=LD) - self.value).astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(self.bar > 0, d / self.bar, np.where(d > 0, np.inf, 0.0))
        return float(r.max())

    def outside(self, got):
        """Entries where got misses the bar."""
        d = np.abs(np.asarray(got, dtype=LD) - self.value).astype(np.float64)
        return np.nonzero(d > self.bar)[0]


def entry_pairs(NP):
    """(a, b) of entry e: the upper triangle row-major, then eta_a as (a, -1)."""
    return [(a, b) for a in range(NP) for b in range(a, NP)] + [(a, -1) for a in range(NP)]


def moments(depths, y, params, B, n_union=None):
    """depths [1 + 12B, rows*cols] float32 (+inf uncovered) as rendered, y [rows*cols] float32 (NaN = no reading)
    as staged on the device, params a gauss_twin.Params.  n_union: an upper bound on the kernel's union rectangle
    (default: the whole image).  -> Moments."""
    require_extended()
    depths = np.asarray(depths)
    y = np.asarray(y)
    assert depths.dtype == np.float32 and y.dtype == np.float32, "the device works on float32 planes and frames"
    NP, ND = 6 * B, 1 + 12 * B
    assert depths.shape[0] == ND and depths.shape[1] == y.size
    npx = y.size
    n_u = npx if n_union is None else int(n_union)
    L = 256 * -(-n_u // GRID_PX)
    cov_all = np.isfinite(depths)
    # pixels with a finite observation that some sigma point covers; elsewhere h = 0 exactly on the device too
    sel = np.nonzero(np.isfinite(y) & cov_all.any(0))[0]
    n = sel.size
    k = _host_constants(params, B)
    cov = cov_all[:, sel]
    m = [_Val.exact(np.where(cov[j], depths[j, sel].astype(LD), LD(params.bg_depth))) for j in range(ND)]
    s = [_Val(np.where(cov[j], k["fg2"].v, k["bg2"].v), np.where(cov[j], k["fg2"].e, k["bg2"].e)) for j in range(ND)]
    # the kernel's order, line for line (rbsensor_gauss.hip, rbs_gauss_moments_kernel)
    sm, ss = _Val.exact(np.zeros(n)), _Val.exact(np.zeros(n))
    for j in range(1, ND):
        sm = sm + m[j]
        ss = ss + s[j]
    yhat = k["wm0"] * m[0] + k["w"] * (sm + k["extra"] * m[0])
    sq = _Val.exact(np.zeros(n))
    for j in range(1, ND):
        dj = m[j] - yhat
        sq = sq + dj * dj
    d0 = m[0] - yhat
    d00 = d0 * d0
    Pv = k["wc0"] * d00 + k["w"] * (sq + k["extra"] * d00) + (k["wm0"] * s[0] + k["w"] * (ss + k["extra"] * s[0]))
    p_clamped = Pv.v < k["fg2"].v
    Pv = _vmax(Pv, k["fg2"])
    h, hh = [], _Val.exact(np.zeros(n))
    for j in range(NP):
        h.append((m[1 + 2 * j] - m[2 + 2 * j]) * k["inv2sqrtc"])
        hh = hh + h[j] * h[j]
    R = _vmax(Pv - hh, k["fg2"])
    yv = y[sel].astype(LD)
    res = _Val.exact(yv) - yhat
    b = _Val.exact(np.ones(n))
    inside = (yv >= LD(params.uniform_tail_min)) & (yv <= LD(params.uniform_tail_max))
    robust = params.tail_weight > 0.0
    counts = dict(pixels=int(n), p_clamp=int(p_clamped.sum()), r_clamp=int((Pv.v - hh.v < k["fg2"].v).sum()),
                  b_range=int((robust & ~inside).sum()), b_zero=0, b_mid=0, b_ambiguous=0)
    if robust and inside.any():
        lg = k["half"] * _vlog(k["two_pi"] * Pv)
        lg = _Val(-lg.v, lg.e) - k["half"] * (res * res) / Pv
        x = k["log_tail"] - lg
        bl = _vlogistic(x)
        over = x.v > LD(LN_DBL_MAX)
        near = np.abs(x.v - LD(LN_DBL_MAX)) <= LD(U) * x.e.astype(LD) + LD(1e-12)
        # b = 0 beyond the threshold; near it (b < 1e-307) the device may give 0 or about b: allow 2 |b|
        bv = np.where(over, LD(0.0), bl.v)
        be = np.where(near, 2.0 * np.abs(bl.v).astype(np.float64) / U, np.where(over, 0.0, bl.e))
        b = _Val(np.where(inside, bv, LD(1.0)), np.where(inside, be, 0.0))
        counts["b_zero"] = int((inside & over).sum())
        counts["b_mid"] = int((inside & ~over & (bl.v > 0) & (bl.v < 1)).sum())
        counts["b_ambiguous"] = int((inside & near).sum())
    pi = b / R
    terms = entry_pairs(NP)
    value = np.zeros(len(terms), dtype=LD)
    bar, abs_sum = np.zeros(len(terms)), np.zeros(len(terms))
    ph = [pi * h[a] for a in range(NP)]
    worst = 0.0
    for e, (a, bb) in enumerate(terms):
        t = ph[a] * (h[bb] if bb >= 0 else res)
        at = np.abs(t.v).astype(np.float64)
        value[e] = np.sum(t.v) if n else LD(0.0)
        abs_sum[e] = float(at.sum())
        with np.errstate(divide="ignore", invalid="ignore"):
            kap = np.where(at > 0, t.e / at, 0.0)
        worst = max(worst, float(kap.max()) if n else 0.0)
        lg_n = int(np.ceil(np.log2(max(n, 2))))
        bar[e] = (U + U_LD) * float(t.e.sum()) + ((L + 256) * U + (lg_n + 8) * U_LD) * abs_sum[e] + 16 * 2.0 ** -1074 * n
    if U * worst > 1e-4:
        raise AssertionError(f"a pixel term's condition count {worst:.3g} is beyond the first-order bar")
    counts["kappa_max"] = worst
    counts["L"] = L
    return Moments(value, bar, abs_sum, counts, NP)


def float64_terms(depths, y, params, B, extra=True, pi_over="R", tail_inverted=False):
    """Per pixel (pi, h [NP, npx], residual) in binary64, in the twin's order (GaussTwin.pixel_terms).  The switches
    break it on purpose: extra=False drops the velocity columns' 2 x 6B copies of the centre (kExtra), pi_over="P"
    takes pi = b / P, tail_inverted=True applies the logistic outside the tail range instead of inside."""
    NP = 6 * B
    p = params
    fg2, bg2 = p.fg_noise_std ** 2, p.bg_noise_std ** 2
    a2 = p.ut_alpha ** 2
    c = a2 * 12 * B
    wm0 = 1.0 - 1.0 / a2
    wc0 = wm0 + 1.0 - a2 + 2.0
    w = 1.0 / (2.0 * c)
    y = np.asarray(y, dtype=np.float64)
    cov = np.isfinite(depths)
    m = np.where(cov, depths.astype(np.float64), p.bg_depth)
    s = np.where(cov, fg2, bg2)
    ex = 2.0 * NP if extra else 0.0
    yhat = wm0 * m[0] + w * (m[1:].sum(0) + ex * m[0])
    d0 = m[0] - yhat
    P = wc0 * d0 * d0 + w * (((m[1:] - yhat) ** 2).sum(0) + ex * d0 * d0) + (wm0 * s[0] + w * (s[1:].sum(0) + ex * s[0]))
    P = np.maximum(P, fg2)
    h = (m[1::2] - m[2::2]) / (2.0 * np.sqrt(c))
    R = np.maximum(P - (h * h).sum(0), fg2)
    valid = np.isfinite(y)
    res = np.where(valid, y - yhat, 0.0)
    b = np.ones_like(P)
    if p.tail_weight > 0.0:
        log_tail = np.log(p.tail_weight / (p.uniform_tail_max - p.uniform_tail_min)) - np.log(1.0 - p.tail_weight)
        inside = (y >= p.uniform_tail_min) & (y <= p.uniform_tail_max)
        if tail_inverted:
            inside = ~inside
        with np.errstate(over="ignore", invalid="ignore"):
            lg = -0.5 * np.log(2.0 * np.pi * P) - 0.5 * res * res / P
            b = np.where(valid & inside, 1.0 / (1.0 + np.exp(log_tail - lg)), 1.0)
    pi = np.where(valid, b / (R if pi_over == "R" else P), 0.0)
    return pi, h, res


def float64_moments(depths, y, params, B, **switches):
    """The NE entries from float64_terms, each summed sequentially in pixel order (binary64)."""
    pi, h, res = float64_terms(depths, y, params, B, **switches)
    out = []
    for a, b in entry_pairs(6 * B):
        t = (pi * h[a]) * (h[b] if b >= 0 else res)
        out.append(np.cumsum(t)[-1])
    return np.array(out)
