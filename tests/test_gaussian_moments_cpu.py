"""The moments reference and its bar on the CPU (tests/gauss_reference.py): a plain binary64 evaluation stays inside
the bar on every case of tests/gauss_cases.py, and each of five small mistakes leaves it.  The device is held to the
same bar by tests/test_gpu_gaussian_moments.py."""
import numpy as np
import pytest

import gauss_cases as gc
import gauss_reference as gr
import gauss_twin as gt


def test_longdouble_is_x87_extended():
    gr.require_extended()
    assert np.finfo(np.longdouble).eps == 2.0 ** -63


def _twin_case(name):
    """The case's first frame with the twin's own sigma poses (its first predict from the truth) rendered by the oracle."""
    _, cam, _, orc, p, frames = gc.scene(name, 1)
    B = len(gc.CASES[name]["meshes"])
    truth, y = frames[0]
    tw = gt.GaussTwin(p, B, orc.render_depth)
    tw.initialize(gt.truth_state(truth))
    mu, S = tw.predict(tw.mu, tw.cov)
    mpf, Spf = tw.to_pf(mu, S)
    poses = tw.absolute_poses(tw.z, tw.sigma_deltas(mpf, np.linalg.cholesky(Spf)))
    depths = np.stack([orc.render_depth(q) for q in poses])
    return tw, depths, y, p, B, cam


_CACHE = {}


def _case(name):
    if name not in _CACHE:
        tw, depths, y, p, B, cam = _twin_case(name)
        _CACHE[name] = (tw, depths, y, p, B, cam, gr.moments(depths, y, p, B))
    return _CACHE[name]


@pytest.mark.parametrize("name", list(gc.CASES))
def test_binary64_in_the_twins_order_stays_inside_the_bar(name):
    tw, depths, y, p, B, cam, ref = _case(name)
    gc.check_reach(name, ref, depths, cam.cols, cam.rows)
    pi, h, res, _ = tw.pixel_terms(depths, y)
    pi2, h2, res2 = gr.float64_terms(depths, y, p, B)
    assert np.array_equal(pi, pi2) and np.array_equal(h, h2) and np.array_equal(res, res2)   # the twin's order, bit for bit
    got = gr.float64_moments(depths, y, p, B)
    assert ref.excess(got) <= 1.0, (ref.excess(got), ref.outside(got))
    # and the twin's own sums, in numpy's order: Lambda and eta of whitened_update
    NP = 6 * B
    lam, eta = (h * pi) @ h.T, (h * pi) @ res
    iu = np.triu_indices(NP)
    assert ref.excess(np.concatenate([lam[iu], eta])) <= 1.0


@pytest.mark.parametrize("name", [n for n, c in gc.CASES.items() if "empty" not in c["expect"]])
def test_each_small_mistake_leaves_the_bar(name):
    """Mistakes of the size that a missing bound check or a wrong constant would make."""
    _, depths, y, p, B, cam, ref = _case(name)
    rows, cols = cam.rows, cam.cols
    # one pixel dropped at the edge of a rectangle: of the pixels on the border of some sigma render's covered box,
    # the one with the heaviest terms
    border = np.zeros((rows, cols), bool)
    for plane in np.isfinite(depths).reshape(-1, rows, cols):
        if plane.any():
            rr, cc = np.nonzero(plane)
            r0, r1, c0, c1 = rr.min(), rr.max(), cc.min(), cc.max()
            border[r0, c0:c1 + 1] = border[r1, c0:c1 + 1] = border[r0:r1 + 1, c0] = border[r0:r1 + 1, c1] = True
    pi, h, res = gr.float64_terms(depths, y, p, B)
    weight = (np.abs(pi) * (h * h).sum(0)).reshape(rows, cols)
    weight[~border] = -1.0
    i = int(np.argmax(weight))
    assert weight.flat[i] > 0
    dropped = y.copy()
    dropped[i] = np.nan
    assert ref.outside(gr.float64_moments(depths, dropped, p, B)).size > 0, "one edge pixel dropped"
    # the velocity columns' 2 x 6B copies of the centre left out (kExtra)
    assert ref.outside(gr.float64_moments(depths, y, p, B, extra=False)).size > 0, "kExtra"
    # pi = b / P instead of b / R
    assert ref.outside(gr.float64_moments(depths, y, p, B, pi_over="P")).size > 0, "pi = b / P"
    # one sigma rectangle one column narrower: of the first and last columns every render covers, the one whose
    # pixels weigh most is lost
    w2 = (np.abs(pi) * (h * h).sum(0)).reshape(rows, cols)
    best = (-1.0, 0, 0)
    for k, plane in enumerate(np.isfinite(depths).reshape(-1, rows, cols)):
        if plane.any():
            cs = np.nonzero(plane.any(0))[0]
            for c in (cs.min(), cs.max()):
                best = max(best, (float(w2[plane[:, c], c].sum()), k, c))
    assert best[0] > 0
    shrunk = depths.copy()
    shrunk[best[1]].reshape(rows, cols)[:, best[2]] = np.inf
    assert ref.outside(gr.float64_moments(shrunk, y, p, B)).size > 0, "rectangle one column short"
    # the tail-range test inverted (the robust path only)
    if p.tail_weight > 0.0:
        assert ref.outside(gr.float64_moments(depths, y, p, B, tail_inverted=True)).size > 0, "tail range inverted"


def test_the_bar_follows_the_union_size():
    """L grows by 256 for every further pass of the 256 x 256-pixel grid."""
    _, depths, y, p, B, _, ref = _case("b1_80x60")
    assert ref.counts["L"] == 256
    big = gr.moments(depths, y, p, B, n_union=3 * 65536 + 1)
    assert big.counts["L"] == 4 * 256
    assert np.all(big.bar >= ref.bar) and np.array_equal(big.value, ref.value)
