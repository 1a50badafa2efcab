"""numpy restatement of the scene finder's rule (rbs_find_scene_*, include/rbsensor_mi355x.h), built on
the finder's twins: S1's order, S2's residual frame (owner and support by assess_twin's rule), S3 as a one-body find out of
find_twin / find_fg_twin / find_refine_twin with a scoring function handed in, S4's polish.  binary64 with + - x / and
comparisons in the order of the header: the order, every residual pixel's bits and every selection are the device's."""
import math

import numpy as np

import assess_twin as at
import find_fg_twin as fg
import find_refine_twin as rf
import find_twin as tw

RESIDUAL_NAN = np.uint32(0x7FC00000)
DEFAULTS = dict(explain_sigmas=3.0, explain_radius=2, polish_sweeps=2, polish_children=64, polish_sigma_translation=0.005,
                polish_sigma_angle=math.radians(5.0), polish_decay=0.6)
POLISH_ROUND_BASE = 0x10000


# ---------------------------------------------------------------- S1
def mean_vertex_distance(vertices):
    """e_b in rbs_find_create's order: the sums run over the vertices from the first, one by one (np.cumsum adds in order)."""
    V = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    nv = len(V)
    c = np.cumsum(V, axis=0)[-1] / float(nv)
    dx, dy, dz = V[:, 0] - c[0], V[:, 1] - c[1], V[:, 2] - c[2]
    return float(np.cumsum(np.sqrt(dx * dx + dy * dy + dz * dz))[-1] / float(nv))


def order(e, search_mask):
    """The searched bodies by e_b descending, ties to the lower b."""
    bodies = [b for b in range(len(e)) if search_mask >> b & 1]
    return sorted(bodies, key=lambda b: (-e[b], b))


# ---------------------------------------------------------------- S2
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _agrees(y, d, model_sigma, sigma_factor, sigmas):
    """neither r < -tau nor r > tau with r = (double)y - (double)d, tau = sigmas (model_sigma + sigma_factor (d d))."""
    with np.errstate(invalid="ignore", over="ignore"):
        d = d.astype(np.float64)
        r = y.astype(np.float64) - d
        tau = np.float64(sigmas) * (np.float64(model_sigma) + np.float64(sigma_factor) * (d * d))
        return ~(r < -tau) & ~(r > tau)


def support(planes, placed, frame, model_sigma, sigma_factor, sigmas):
    """planes [B, npx] float32 (+inf: uncovered), placed: the placed bodies -> (support [npx] bool, depth [npx] float32 of the
    owner among the placed bodies, +inf where none)."""
    planes = np.asarray(planes, dtype=np.float32)
    y = np.asarray(frame, dtype=np.float32).reshape(-1)
    placed = sorted(placed)
    if not placed:
        return np.zeros(y.size, dtype=bool), np.full(y.size, np.inf, dtype=np.float32)
    owner, depth = at.owners(planes[placed])
    return (owner >= 0) & np.isfinite(y) & _agrees(y, depth, model_sigma, sigma_factor, sigmas), depth


def explained(planes, placed, frame, rows, cols, model_sigma, sigma_factor, sigmas=3.0, radius=2):
    """[rows, cols] bool: rule (a) or rule (b)."""
    y = np.asarray(frame, dtype=np.float32).reshape(rows, cols)
    sup, depth = support(planes, placed, frame, model_sigma, sigma_factor, sigmas)
    sup, depth = sup.reshape(rows, cols), depth.reshape(rows, cols)
    out = sup.copy()
    if radius > 0 and sup.any():
        r = int(radius)
        ps = np.zeros((rows + 2 * r, cols + 2 * r), dtype=bool)           # outside the image: no support pixel
        pd = np.full((rows + 2 * r, cols + 2 * r), np.inf, dtype=np.float32)
        ps[r:r + rows, r:r + cols] = sup
        pd[r:r + rows, r:r + cols] = depth
        finite = np.isfinite(y)
        for dy in range(2 * r + 1):
            for dx in range(2 * r + 1):
                sj = ps[dy:dy + rows, dx:dx + cols]
                if not sj.any():
                    continue
                out |= finite & sj & _agrees(y, pd[dy:dy + rows, dx:dx + cols], model_sigma, sigma_factor, sigmas)
    return out


def residual(planes, placed, frame, rows, cols, model_sigma, sigma_factor, sigmas=3.0, radius=2):
    """The residual frame [rows * cols] float32: the quiet NaN 0x7FC00000 where explained, the frame's bits elsewhere."""
    fb = bits(np.asarray(frame, dtype=np.float32).reshape(-1))
    if not list(placed):
        return fb.copy().view(np.float32)
    ex = explained(planes, placed, frame, rows, cols, model_sigma, sigma_factor, sigmas, radius).reshape(-1)
    return np.where(ex, RESIDUAL_NAN, fb).astype(np.uint32).view(np.float32)


# ---------------------------------------------------------------- S3: a one-body find with the scores handed in
def find_body(frame, rows, cols, K, vertices, p, model_sigma, sigma_factor, coarse_score, full_score, foreground=None, refinement=None):
    """rbs_find_run's steps 1-7 on `frame` for the mesh `vertices`.  p: the finder's parameters (attributes of
    rbs_find_params' names); coarse_score(coarse frame, rows, cols, K, poses) and full_score(poses) -> scores.
    foreground / refinement: dicts of rbs_find_foreground's / rbs_find_refinement's fields, or None.
    -> (poses [S, 12] best first, scores [S], found)."""
    f = tw.coarse_factor(cols, p.coarse_downsampling)
    coarse, cr, cc = tw.subsample(frame, rows, cols, f)
    Kc = tw.coarse_K(K, f)
    seed_frame = coarse
    if foreground is not None:
        _, seed_frame = fg.foreground(coarse.ravel(), cr, cc, p.min_depth, p.max_depth, model_sigma, sigma_factor, p.seed, **foreground)
    seeds, _ = tw.seeds(np.asarray(seed_frame).reshape(cr, cc), p.seed_stride, p.min_depth, p.max_depth, p.max_seeds)
    if len(seeds) == 0:
        return np.zeros((0, 12)), np.zeros(0), False
    off = mean_vertex_distance(vertices) if p.depth_offset < 0 else p.depth_offset
    hyp = tw.hypotheses(seeds, p.n_rotations, Kc, off)
    hs = np.asarray(coarse_score(coarse, cr, cc, Kc, hyp))
    cand = tw.select_order(hs)[: p.n_candidates]
    kept = tw.nms(hyp[cand], p.nms_translation, p.nms_angle, p.n_survivors)
    cur = hyp[cand][kept]
    S = len(cur)
    if S == 0:
        return np.zeros((0, 12)), np.zeros(0), False
    if refinement is not None and p.rounds > 0:
        cur, best, _ = rf.refine(cur, full_score, p.rounds, p.children, p.seed, p.sigma_angle, p.sigma_translation, **refinement)
    else:
        best = np.asarray(full_score(cur)) if p.rounds == 0 else None
        st, sa = p.sigma_translation, p.sigma_angle
        for r in range(p.rounds):
            kp = tw.children_array(cur, p.children, r, p.seed, st, sa)
            ks = np.asarray(full_score(kp.reshape(-1, 12))).reshape(S, p.children)
            b = tw.best_child(ks)
            best, cur = ks[np.arange(S), b], kp[np.arange(S), b]
            st, sa = st * p.decay, sa * p.decay
    o = tw.result_order(best)
    found = bool(best[o[0]] >= p.min_score)      # (NaN: False)
    return cur[o], best[o], found


# ---------------------------------------------------------------- S4
def polish_counter(r, c, j, pair):
    """The Philox counter of pair `pair` of child j of polish round r moving body c: (ctr_hi, ctr_lo) as find_twin.philox takes them."""
    return ((POLISH_ROUND_BASE + r) << 32) | c, (j << 2) | pair


def polish_children(X, c, n_children, r, seed, st, sa):
    """[children][B][12]: child 0 is X; child j > 0 has body c perturbed by step 6's rule with the counter of polish_counter."""
    X = np.asarray(X, dtype=np.float64).reshape(-1, 12)
    out = np.repeat(X[None], n_children, 0).copy()
    P = X[c]
    for j in range(1, n_children):
        nz = tw.child_normals(seed, POLISH_ROUND_BASE + r, c, j)
        A = tw.rotvec_matrix(sa * nz[:3])
        out[j, c, :9] = (A @ P[:9].reshape(3, 3)).ravel()
        out[j, c, 9:] = P[9:] + st * nz[3:]
    return out


def polish_scales(sp, ns, r):
    """(st, sa) of round r: the sigmas times decay^(r div ns), by repeated multiplication."""
    st, sa = sp["polish_sigma_translation"], sp["polish_sigma_angle"]
    for _ in range(r // ns):
        st, sa = st * sp["polish_decay"], sa * sp["polish_decay"]
    return st, sa


def polish(X, searched_order, joint_score, seed, **params):
    """S4 over X [B][12]; joint_score(poses [n][B][12]) -> [n].  -> (X, its joint score, per round (children, scores, best))."""
    sp = dict(DEFAULTS, **params)
    X = np.asarray(X, dtype=np.float64).reshape(-1, 12).copy()
    ns = len(searched_order)
    rounds = []
    score = np.nan
    for r in range(sp["polish_sweeps"] * ns):
        c = searched_order[r % ns]
        st, sa = polish_scales(sp, ns, r)
        ch = polish_children(X, c, sp["polish_children"], r, seed, st, sa)
        cs = np.asarray(joint_score(ch), dtype=np.float64)
        b = int(tw.best_child(cs[None])[0])
        X, score = ch[b].copy(), float(cs[b])
        rounds.append((ch, cs, b))
    if not rounds:
        score = float(np.asarray(joint_score(X[None]))[0])
    return X, score, rounds


# ---------------------------------------------------------------- the whole scene find
def scene_find(frame, rows, cols, e, search_mask, given, plane_of, find_of, joint_score, model_sigma, sigma_factor, seed, **params):
    """plane_of(b, pose [12]) -> body b's plane [npx] float32 (+inf: uncovered); find_of(b, residual frame) -> (pose [12] or
    None, score, found); joint_score(poses [n][B][12]) -> [n].  -> dict(poses [B][12], scores [B], found_mask, joint_score,
    order, residuals {b: frame}, rounds)."""
    sp = dict(DEFAULTS, **params)
    B = len(e)
    X = np.full((B, 12), np.nan)
    scores = np.full(B, np.nan)
    placed = [b for b in range(B) if not search_mask >> b & 1]
    for b in placed:
        X[b] = np.asarray(given, dtype=np.float64).reshape(B, 12)[b]
    posed = set(placed)
    planes = np.full((B, rows * cols), np.inf, dtype=np.float32)
    for b in placed:
        planes[b] = plane_of(b, X[b])
    srch = order(e, search_mask)
    found_mask, residuals = 0, {}
    for b in srch:
        res = residual(planes, placed, frame, rows, cols, model_sigma, sigma_factor, sp["explain_sigmas"], sp["explain_radius"])
        residuals[b] = res
        pose, score, found = find_of(b, res)
        if pose is None:
            continue
        X[b], scores[b] = pose, score
        posed.add(b)
        if found:
            placed = sorted(placed + [b])
            planes[b] = plane_of(b, X[b])
            found_mask |= 1 << b
    joint, rounds = np.nan, None
    if len(posed) == B:
        X, joint, rounds = polish(X, srch, joint_score, seed, **sp)
    return dict(poses=X, scores=scores, found_mask=found_mask, joint_score=joint, order=srch, residuals=residuals, rounds=rounds)
