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


def sf_quaternions(n):
    """(x, y, z, w) Super-Fibonacci spiral (Alexa, CVPR 2022)."""
    s = np.arange(n, dtype=np.float64) + 0.5
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
    Rs = sf_rotations(n_rot)
    s, r = idx // n_rot, idx % n_rot
    u, v, d = seed_arr[s, 0], seed_arr[s, 1], seed_arr[s, 2]
    x = (u - Kc[0, 2]) / Kc[0, 0]
    y = (v - Kc[1, 2]) / Kc[1, 1]
    nrm = np.sqrt(x * x + y * y + 1.0)
    t = np.stack([d * x + offset * (x / nrm), d * y + offset * (y / nrm), d + offset * (1.0 / nrm)], -1)
    return np.concatenate([Rs[r], t], -1)


def select_order(scores, index=None):
    """Positions in the order (score descending, index ascending), NaN dropped."""
    scores = np.asarray(scores)
    index = np.arange(len(scores)) if index is None else np.asarray(index)
    keep = ~np.isnan(scores)
    pos = np.nonzero(keep)[0]
    return pos[np.lexsort((index[pos], -scores[pos]))]


def nms(poses, nms_t, nms_a, max_keep):
    """Greedy suppression over poses [n][12] already in order: positions kept."""
    t2, trace_min = nms_t * nms_t, 1.0 + 2.0 * math.cos(nms_a)
    kept = []
    for c in range(len(poses)):
        if len(kept) >= max_keep:
            break
        P = poses[c]
        drop = False
        for q in kept:
            Q = poses[q]
            dx, dy, dz = P[9] - Q[9], P[10] - Q[10], P[11] - Q[11]
            d2 = dx * dx + dy * dy + dz * dz
            tr = P[0] * Q[0]
            for e in range(1, 9):
                tr = tr + P[e] * Q[e]
            if d2 <= t2 and tr >= trace_min:
                drop = True
                break
        if not drop:
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
    """Index of the best child per row (ties: lowest j; NaN never beats a number)."""
    out = []
    for row in np.asarray(scores):
        b, bs = 0, row[0]
        for j in range(1, len(row)):
            s = row[j]
            if s > bs or (np.isnan(bs) and not np.isnan(s)):
                b, bs = j, s
        out.append(b)
    return np.array(out)
