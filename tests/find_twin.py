"""numpy twin of the object finder's deterministic stages (rbs_find_*, include/rbsensor_mi355x.h):
coarse sub-sample, seeds, Super-Fibonacci rotations, hypothesis poses, the suppression, Philox4x32-10
and the refinement's perturbation.  Same formulas, same operation order as rbsensor_find.hip."""
import math

import numpy as np

PSI = 1.533751168755204288118041
TWO_PI = 6.283185307179586


def coarse_factor(cols, f=0):
    if f:
        return f
    return 4 if cols // 4 >= 160 else 2 if cols // 2 >= 160 else 1


def subsample(frame, rows, cols, f):
    img = np.asarray(frame, dtype=np.float32).reshape(rows, cols)
    r, c = rows // f, cols // f
    return np.ascontiguousarray(img[: r * f: f, : c * f: f]), r, c


def coarse_K(K, f):
    K = np.array(K, dtype=np.float64).reshape(3, 3).copy()
    K[:2, :] /= f
    return K


def seeds(coarse, stride, dmin, dmax, max_seeds):
    """-> (seeds [n][4] = (u, v, d, pixel), number of valid grid pixels before thinning)."""
    rows, cols = coarse.shape
    vv, uu = np.meshgrid(np.arange(0, rows, stride), np.arange(0, cols, stride), indexing="ij")
    px = (vv * cols + uu).ravel()
    d = coarse.ravel()[px].astype(np.float64)
    with np.errstate(invalid="ignore"):
        ok = (d >= dmin) & (d <= dmax)
    px = px[ok]
    n = len(px)
    step = -(-n // max_seeds) if n > max_seeds else 1
    px = px[::step]
    out = np.stack([px % cols, px // cols, coarse.ravel()[px].astype(np.float64), px], -1).astype(np.float64)
    return out.reshape(-1, 4), n


def sf_quaternions(n, i=None):
    """(x, y, z, w) Super-Fibonacci spiral (Alexa, CVPR 2022): all n points, or those of i."""
    s = (np.arange(n, dtype=np.float64) if i is None else np.asarray(i, dtype=np.float64)) + 0.5
    t = s / n
    r, R = np.sqrt(t), np.sqrt(1.0 - t)
    a, b = TWO_PI * s / 1.4142135623730951, TWO_PI * s / PSI
    return np.stack([r * np.sin(a), r * np.cos(a), R * np.sin(b), R * np.cos(b)], -1)


def quat_xyzw_to_matrix(q):
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    R = np.empty(q.shape[:-1] + (9,))
    R[..., 0] = 1.0 - 2.0 * (y * y + z * z); R[..., 1] = 2.0 * (x * y - w * z); R[..., 2] = 2.0 * (x * z + w * y)
    R[..., 3] = 2.0 * (x * y + w * z); R[..., 4] = 1.0 - 2.0 * (x * x + z * z); R[..., 5] = 2.0 * (y * z - w * x)
    R[..., 6] = 2.0 * (x * z - w * y); R[..., 7] = 2.0 * (y * z + w * x); R[..., 8] = 1.0 - 2.0 * (x * x + y * y)
    return R


def sf_rotations(n):
    return quat_xyzw_to_matrix(sf_quaternions(n))


def depth_offset(vertices):
    V = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    return float(np.linalg.norm(V - V.mean(0), axis=1).mean())


def hypotheses(seed_arr, n_rot, Kc, offset, idx=None):
    """Poses [H][12] of hypotheses h = seed * n_rot + rotation (all of them, or those in idx)."""
    H = len(seed_arr) * n_rot
    idx = np.arange(H) if idx is None else np.asarray(idx, dtype=np.int64)
    s, r = idx // n_rot, idx % n_rot
    Rs = quat_xyzw_to_matrix(sf_quaternions(n_rot, r))
    u, v, d = seed_arr[s, 0], seed_arr[s, 1], seed_arr[s, 2]
    x = (u - Kc[0, 2]) / Kc[0, 0]
    y = (v - Kc[1, 2]) / Kc[1, 1]
    nrm = np.sqrt(x * x + y * y + 1.0)
    t = np.stack([d * x + offset * (x / nrm), d * y + offset * (y / nrm), d + offset * (1.0 / nrm)], -1)
    return np.concatenate([Rs, t], -1)


def select_order(scores, index=None):
    """Positions in the order (score descending, index ascending), NaN dropped."""
    scores = np.asarray(scores)
    index = np.arange(len(scores)) if index is None else np.asarray(index)
    keep = ~np.isnan(scores)
    pos = np.nonzero(keep)[0]
    return pos[np.lexsort((index[pos], -scores[pos]))]


def nms(poses, nms_t, nms_a, max_keep, scores=None):
    """Greedy suppression over poses [n][12] already in order: positions kept.  d2 and the trace in the kernel's operation
    order, in binary64 (element-wise over the kept poses); a NaN score (they sort last) ends the candidates."""
    poses = np.asarray(poses, dtype=np.float64)
    t2, trace_min = nms_t * nms_t, 1.0 + 2.0 * math.cos(nms_a)
    kept = []
    for c in range(len(poses)):
        if len(kept) >= max_keep:
            break
        if scores is not None and np.isnan(scores[c]):
            break
        P, Q = poses[c], poses[kept]
        dx, dy, dz = P[9] - Q[:, 9], P[10] - Q[:, 10], P[11] - Q[:, 11]
        d2 = dx * dx + dy * dy + dz * dz
        tr = P[0] * Q[:, 0]
        for e in range(1, 9):
            tr = tr + P[e] * Q[:, e]
        if not np.any((d2 <= t2) & (tr >= trace_min)):
            kept.append(c)
    return kept


M32 = 0xFFFFFFFF


def philox(seed, ctr_hi, ctr_lo):
    """Philox4x32-10 as rbt::philox: (key = seed, counter = (ctr_lo, ctr_hi)) -> 4 x uint32."""
    k0, k1 = seed & M32, (seed >> 32) & M32
    c0, c1, c2, c3 = ctr_lo & M32, (ctr_lo >> 32) & M32, ctr_hi & M32, (ctr_hi >> 32) & M32
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        n0 = ((p1 >> 32) ^ c1 ^ k0) & M32
        n2 = ((p0 >> 32) ^ c3 ^ k1) & M32
        c1, c3, c0, c2 = p1 & M32, p0 & M32, n0, n2
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def u01(hi, lo):
    return float((((hi << 32) | lo) >> 11)) * (1.0 / 9007199254740992.0)


def child_normals(seed, rnd, k, j):
    nz = np.zeros(6)
    for pr in range(3):
        x, y, z, w = philox(seed, (rnd << 32) | k, (j << 2) | pr)
        u1, u2 = 1.0 - u01(x, y), u01(z, w)
        rad = math.sqrt(-2.0 * math.log(u1))
        nz[2 * pr] = rad * math.cos(TWO_PI * u2)
        nz[2 * pr + 1] = rad * math.sin(TWO_PI * u2)
    return nz


def rotvec_matrix(v):
    angle = math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    half = 0.5 * angle
    k = 0.5 - angle * angle / 48.0 if angle < 1e-9 else math.sin(half) / angle
    q = np.array([v[0] * k, v[1] * k, v[2] * k, math.cos(half)])
    return quat_xyzw_to_matrix(q).reshape(3, 3)


def children(surv, n_children, rnd, seed, st, sa):
    """[S][children][12] of round rnd around survivors [S][12]."""
    S = len(surv)
    out = np.zeros((S, n_children, 12))
    for k in range(S):
        P = surv[k]
        out[k, 0] = P
        for j in range(1, n_children):
            nz = child_normals(seed, rnd, k, j)
            A = rotvec_matrix(sa * nz[:3])
            out[k, j, :9] = (A @ P[:9].reshape(3, 3)).ravel()
            out[k, j, 9:] = P[9:] + st * nz[3:]
    return out


def best_child(scores):
    """Index of the best child per row (ties: lowest j; NaN never beats a number; a row of NaN keeps child 0)."""
    scores = np.asarray(scores, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        filled = np.where(np.isnan(scores), -np.inf, scores)
        first_max = np.argmax(filled, axis=1)             # (argmax: the first of equal maxima)
    # a row whose only numbers are -inf: the first NUMBER wins over a NaN before it
    number = ~np.isnan(scores)
    first_number = np.argmax(number, axis=1)
    only_low = number.any(axis=1) & np.isneginf(filled.max(axis=1))
    return np.where(only_low, first_number, np.where(number.any(axis=1), first_max, 0))


def child_normals_array(seed, rnd, S, n_children):
    """[S][children][6]: child_normals for every (k, j), the Philox blocks through filter_twin's array form (held to the
    integer form by tests/test_filter_twin_cpu.py)."""
    import filter_twin as ft
    j = np.arange(n_children, dtype=np.uint64)
    out = np.empty((S, n_children, 6))
    for k in range(S):
        for pr in range(3):
            w = ft.philox_words(seed, (rnd << 32) | k, (j << np.uint64(2)) | np.uint64(pr))
            u1, u2 = 1.0 - ft.u01(w[0], w[1]), ft.u01(w[2], w[3])
            rad = np.sqrt(-2.0 * np.log(u1))
            out[k, :, 2 * pr] = rad * np.cos(TWO_PI * u2)
            out[k, :, 2 * pr + 1] = rad * np.sin(TWO_PI * u2)
    return out


def children_array(surv, n_children, rnd, seed, st, sa):
    """children(...) for many children at once: numpy over (k, j), the products summed in the kernel's order."""
    surv = np.asarray(surv, dtype=np.float64)
    S = len(surv)
    nz = child_normals_array(seed, rnd, S, n_children)
    v = sa * nz[..., :3]
    angle = np.sqrt(v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1] + v[..., 2] * v[..., 2])
    half = 0.5 * angle
    with np.errstate(invalid="ignore", divide="ignore"):
        kk = np.where(angle < 1e-9, 0.5 - angle * angle / 48.0, np.sin(half) / angle)
    A = quat_xyzw_to_matrix(np.stack([v[..., 0] * kk, v[..., 1] * kk, v[..., 2] * kk, np.cos(half)], -1))
    P = surv[:, None, :]
    out = np.empty((S, n_children, 12))
    for r in range(3):
        for c in range(3):
            out[..., 3 * r + c] = A[..., 3 * r] * P[..., c] + A[..., 3 * r + 1] * P[..., 3 + c] + A[..., 3 * r + 2] * P[..., 6 + c]
    out[..., 9:] = P[..., 9:] + st * nz[..., 3:]
    out[:, 0] = surv
    return out


# ---------------------------------------------------------------- the selection's total order
INT64_MAX = 2 ** 63 - 1


def topk(scores, index=None, k=None):
    """The best k of (score, index) in rbs_find_topk_kernel's total order -- larger score first, NaN last, then smaller
    index -- as (scores [k], indices [k]).  NaN items are KEPT, in index order at the end (select_order drops them);
    fewer than k items are padded with (NaN, INT64_MAX), the kernel's own padding."""
    scores = np.asarray(scores, dtype=np.float64)
    index = np.arange(len(scores), dtype=np.int64) if index is None else np.asarray(index, dtype=np.int64)
    k = len(scores) if k is None else k
    nan = np.isnan(scores)
    with np.errstate(invalid="ignore"):
        order = np.lexsort((index, -np.where(nan, 0.0, scores), nan))     # (-0.0 == +0.0: the index decides, as in the kernel)
    order = order[:k]
    pad = k - len(order)
    return (np.concatenate([scores[order], np.full(pad, np.nan)]), np.concatenate([index[order], np.full(pad, INT64_MAX, dtype=np.int64)]))


def result_order(scores):
    """The final sort of the survivors: positions in topk's order.  A survivor whose children all scored NaN stays, with
    its NaN score, after every survivor that has a number."""
    return topk(scores)[1]


# ---------------------------------------------------------------- the transcendental stages in extended precision
# The same formulas from the same binary64 inputs and constants, every operation in extended precision: mpmath at 40
# digits where it is installed, np.longdouble (64-bit mantissa) otherwise.  Results are np.longdouble arrays.
try:
    import mpmath as _mp
except ImportError:             # pragma: no cover
    _mp = None

assert np.finfo(np.longdouble).nmant >= 63, "the extended-precision twin needs an x87 long double"


class _Ext:
    """Scalar arithmetic of the extended-precision twin."""
    def __init__(self, use_mpmath):
        self.mp = _mp if use_mpmath and _mp is not None else None
        if self.mp is not None:
            self.ctx = _mp.mp.clone()
            self.ctx.dps = 40
            self.num, self.sqrt, self.sin, self.cos, self.log = self.ctx.mpf, self.ctx.sqrt, self.ctx.sin, self.ctx.cos, self.ctx.log
        else:
            self.num, self.sqrt, self.sin, self.cos, self.log = np.longdouble, np.sqrt, np.sin, np.cos, np.log

    def out(self, x):
        """-> np.longdouble (mpmath: the two leading binary64 pieces, 106 bits, rounded once)."""
        if self.mp is None:
            return np.longdouble(x)
        hi = float(x)
        return np.longdouble(hi) + np.longdouble(float(x - hi))


def _ext(use_mpmath=True):
    return _Ext(use_mpmath)


def _quat_matrix_ext(x, y, z, w):
    return [1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
            2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
            2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]


def sf_rotations_ext(n, idx=None, use_mpmath=True):
    """sf_rotations(n)[idx] in extended precision: [len(idx)][9] np.longdouble."""
    E = _ext(use_mpmath)
    idx = range(n) if idx is None else idx
    two_pi, root2, psi = E.num(TWO_PI), E.num(1.4142135623730951), E.num(PSI)
    out = np.empty((len(idx), 9), dtype=np.longdouble)
    for row, i in enumerate(idx):
        s = E.num(int(i)) + E.num(0.5)
        t = s / E.num(int(n))
        r, R = E.sqrt(t), E.sqrt(1 - t)
        a, b = two_pi * s / root2, two_pi * s / psi
        out[row] = [E.out(v) for v in _quat_matrix_ext(r * E.sin(a), r * E.cos(a), R * E.sin(b), R * E.cos(b))]
    return out


def hypotheses_ext(seed_arr, n_rot, Kc, offset, idx, use_mpmath=True):
    """hypotheses(...)[idx] in extended precision: [len(idx)][12] np.longdouble."""
    E = _ext(use_mpmath)
    idx = np.asarray(idx, dtype=np.int64)
    s, r = idx // n_rot, idx % n_rot
    out = np.empty((len(idx), 12), dtype=np.longdouble)
    out[:, :9] = sf_rotations_ext(n_rot, r, use_mpmath)
    fx, fy, cx, cy, off = (E.num(float(v)) for v in (Kc[0][0], Kc[1][1], Kc[0][2], Kc[1][2], offset))
    for row, k in enumerate(s):
        u, v, d = (E.num(float(q)) for q in seed_arr[k][:3])
        x, y = (u - cx) / fx, (v - cy) / fy
        nrm = E.sqrt(x * x + y * y + 1)
        out[row, 9:] = [E.out(d * x + off * (x / nrm)), E.out(d * y + off * (y / nrm)), E.out(d + off * (1 / nrm))]
    return out


def _child_normals_ext(E, seed, rnd, k, j):
    nz = []
    for pr in range(3):
        x, y, z, w = philox(seed, (rnd << 32) | k, (j << 2) | pr)
        # (u01 is exact in binary64: a 53-bit integer times 2^-53; so is 1 - u)
        u1, u2 = E.num(1.0 - u01(x, y)), E.num(u01(z, w))
        rad = E.sqrt(-2 * E.log(u1))
        nz += [rad * E.cos(E.num(TWO_PI) * u2), rad * E.sin(E.num(TWO_PI) * u2)]
    return nz


def child_normals_ext(seed, rnd, k, j, use_mpmath=True):
    E = _ext(use_mpmath)
    return np.array([E.out(v) for v in _child_normals_ext(E, seed, rnd, k, j)], dtype=np.longdouble)


def children_ext(surv, n_children, rnd, seed, st, sa, pick=None, use_mpmath=True):
    """children(...) in extended precision, for the (k, j) pairs of `pick` (default: all): [len(pick)][12] np.longdouble."""
    E = _ext(use_mpmath)
    surv = np.asarray(surv, dtype=np.float64)
    pick = [(k, j) for k in range(len(surv)) for j in range(n_children)] if pick is None else pick
    out = np.empty((len(pick), 12), dtype=np.longdouble)
    st_, sa_ = E.num(float(st)), E.num(float(sa))
    for row, (k, j) in enumerate(pick):
        P = [E.num(float(v)) for v in surv[k]]
        if j == 0:
            out[row] = surv[k]
            continue
        nz = _child_normals_ext(E, seed, rnd, k, j)
        v = [sa_ * nz[0], sa_ * nz[1], sa_ * nz[2]]
        angle = E.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
        half = angle / 2
        kk = E.num(0.5) - angle * angle / 48 if angle < 1e-9 else E.sin(half) / angle
        A = _quat_matrix_ext(v[0] * kk, v[1] * kk, v[2] * kk, E.cos(half))
        for r in range(3):
            for c in range(3):
                out[row, 3 * r + c] = E.out(A[3 * r] * P[c] + A[3 * r + 1] * P[3 + c] + A[3 * r + 2] * P[6 + c])
        for e in range(3):
            out[row, 9 + e] = E.out(P[9 + e] + st_ * nz[3 + e])
    return out
