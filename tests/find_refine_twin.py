"""numpy twin of the object finder's step 6b, the adaptive refinement (include/rbsensor_mi355x.h; rbs_findr_*_kernel in
dbot_ros_amd/csrc/rbsensor_find.hip): every survivor's 6 x 6 search covariance, its Cholesky factor by rows with the diagonal
fallback, the perturbations d = L n, the elite of a round and the covariance update.  Binary64 scalars with + - * / and sqrt in
the header's order: given the device's perturbations and scores, every elite and covariance is the device's, bit for bit.  The
normals, the rotation and the total order are find_twin's."""
import math

import numpy as np

import find_twin as tw

DEFAULTS = dict(elite=8, mix=0.5, shrink=1.0, jitter=1e-10)
F64_MAX = float(np.finfo(np.float64).max)


def initial_covariance(sigma_angle, sigma_translation):
    sa, st = np.float64(sigma_angle), np.float64(sigma_translation)
    return np.diag([sa * sa] * 3 + [st * st] * 3)


def factor(C, jitter):
    """The lower Cholesky factor of C [6][6] by rows; a pivot that is not > 0 or not finite: diag(sqrt(max(C_ii, jitter)))."""
    C = np.asarray(C, dtype=np.float64).reshape(6, 6)
    L = np.zeros((6, 6))
    ok = True
    with np.errstate(all="ignore"):
        for i in range(6):
            for j in range(i + 1):
                s = C[i, j]
                for k in range(j):
                    s = s - L[i, k] * L[j, k]
                if j == i:
                    ok = ok and bool(s > 0.0) and bool(s <= F64_MAX)
                    L[i, i] = np.sqrt(s)
                else:
                    L[i, j] = s / L[j, j]
    if ok:
        return L
    return np.diag([math.sqrt(C[i, i] if C[i, i] > jitter else jitter) for i in range(6)])


def perturb(L, nz):
    """d = L n for normals nz [..., 6]: d_a = L_a0 n_0 + ... + L_aa n_a, summed in that order."""
    nz = np.asarray(nz, dtype=np.float64)
    d = np.empty_like(nz)
    for a in range(6):
        s = L[a, 0] * nz[..., 0]
        for b in range(1, a + 1):
            s = s + L[a, b] * nz[..., b]
        d[..., a] = s
    return d


def children(surv, factors, n_children, rnd, seed):
    """-> (poses [S][children][12], d [S][children][6]) of round rnd around survivors [S][12] with factors [S][6][6]."""
    surv = np.asarray(surv, dtype=np.float64)
    S = len(surv)
    nz = tw.child_normals_array(seed, rnd, S, n_children)
    d = np.stack([perturb(np.asarray(factors[k]).reshape(6, 6), nz[k]) for k in range(S)])
    d[:, 0] = 0.0
    return poses_from(surv, d), d


def poses_from(surv, d):
    """The children's poses from their perturbations d [S][children][6]: R = R(d_0..2) R_k, t = t_k + d_3..5; child 0: the survivor."""
    surv = np.asarray(surv, dtype=np.float64)
    v = d[..., :3]
    angle = np.sqrt(v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1] + v[..., 2] * v[..., 2])
    half = 0.5 * angle
    with np.errstate(invalid="ignore", divide="ignore"):
        kk = np.where(angle < 1e-9, 0.5 - angle * angle / 48.0, np.sin(half) / angle)
    A = tw.quat_xyzw_to_matrix(np.stack([v[..., 0] * kk, v[..., 1] * kk, v[..., 2] * kk, np.cos(half)], -1))
    P = surv[:, None, :]
    out = np.empty(d.shape[:2] + (12,))
    for r in range(3):
        for c in range(3):
            out[..., 3 * r + c] = A[..., 3 * r] * P[..., c] + A[..., 3 * r + 1] * P[..., 3 + c] + A[..., 3 * r + 2] * P[..., 6 + c]
    out[..., 9:] = P[..., 9:] + d[..., 3:]
    out[:, 0] = surv
    return out


def children_ext(surv, factors, n_children, rnd, seed, pick, use_mpmath=True):
    """children(...) in extended precision from the same binary64 factors, for the (k, j) pairs of `pick`:
    (poses [len(pick)][12], d [len(pick)][6]) np.longdouble."""
    E = tw._ext(use_mpmath)
    surv = np.asarray(surv, dtype=np.float64)
    out = np.empty((len(pick), 12), dtype=np.longdouble)
    dd = np.zeros((len(pick), 6), dtype=np.longdouble)
    for row, (k, j) in enumerate(pick):
        if j == 0:
            out[row] = surv[k]
            continue
        P = [E.num(float(v)) for v in surv[k]]
        L = np.asarray(factors[k], dtype=np.float64).reshape(6, 6)
        nz = tw._child_normals_ext(E, seed, rnd, k, j)
        d = []
        for a in range(6):
            s = E.num(float(L[a, 0])) * nz[0]
            for b in range(1, a + 1):
                s = s + E.num(float(L[a, b])) * nz[b]
            d.append(s)
        angle = E.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
        half = angle / 2
        kk = E.num(0.5) - angle * angle / 48 if angle < 1e-9 else E.sin(half) / angle
        A = tw._quat_matrix_ext(d[0] * kk, d[1] * kk, d[2] * kk, E.cos(half))
        for r in range(3):
            for c in range(3):
                out[row, 3 * r + c] = E.out(A[3 * r] * P[c] + A[3 * r + 1] * P[3 + c] + A[3 * r + 2] * P[6 + c])
        for e in range(3):
            out[row, 9 + e] = E.out(P[9 + e] + d[3 + e])
        dd[row] = [E.out(x) for x in d]
    return out, dd


def elite_order(scores, elite):
    """The `elite` best children of one survivor in step 5's order (score descending, j ascending, NaN never): their j."""
    return tw.select_order(np.asarray(scores, dtype=np.float64))[:elite]


def update(C, scores, d, elite, mix, shrink, jitter):
    """One survivor's covariance after a round: scores [children], d [children][6] -> C' [6][6]."""
    C = np.asarray(C, dtype=np.float64).reshape(6, 6)
    d = np.asarray(d, dtype=np.float64).reshape(-1, 6)
    el = elite_order(scores, elite)
    m = len(el)
    if m == 0:
        return C.copy()
    mix, shrink, jitter = np.float64(mix), np.float64(shrink), np.float64(jitter)
    with np.errstate(all="ignore"):
        acc = np.zeros((6, 6))
        for j in el:                                   # (element-wise: M_ab's own sum, in elite order)
            acc = acc + d[j][:, None] * d[j][None, :]
        out = shrink * ((np.float64(1.0) - mix) * C + mix * (acc / np.float64(m)))
        out[np.arange(6), np.arange(6)] = np.diag(out) + jitter
    return out


def update_all(C, scores, d, elite, mix, shrink, jitter):
    """update for survivors [S]: C [S][6][6] (or [S][36]), scores [S][children], d [S][children][6] -> (C' [S][6][6], L' [S][6][6])."""
    C = np.asarray(C, dtype=np.float64).reshape(-1, 6, 6)
    S = len(C)
    scores = np.asarray(scores, dtype=np.float64).reshape(S, -1)
    d = np.asarray(d, dtype=np.float64).reshape(S, -1, 6)
    new = np.stack([update(C[k], scores[k], d[k], elite, mix, shrink, jitter) for k in range(S)])
    return new, np.stack([factor(new[k], jitter) for k in range(S)])


def refine(surv, score_fn, rounds, n_children, seed, sigma_angle, sigma_translation, elite=8, mix=0.5, shrink=1.0, jitter=1e-10):
    """Step 6b's rounds over survivors [S][12]; score_fn(poses [n][12]) -> scores [n].  -> (survivors, their scores,
    the covariances entering every round and the final ones [rounds + 1][S][6][6])."""
    cur = np.asarray(surv, dtype=np.float64).copy()
    S = len(cur)
    C = np.stack([initial_covariance(sigma_angle, sigma_translation)] * S)
    L = np.stack([factor(C[k], jitter) for k in range(S)])
    hist, best = [C], np.full(S, np.nan)
    for r in range(rounds):
        kp, d = children(cur, L, n_children, r, seed)
        ks = np.asarray(score_fn(kp.reshape(-1, 12))).reshape(S, n_children)
        b = tw.best_child(ks)
        best, cur = ks[np.arange(S), b], kp[np.arange(S), b]
        C, L = update_all(C, ks, d, elite, mix, shrink, jitter)
        hist.append(C)
    return cur, best, np.stack(hist)
