"""What the occlusion map's tests share (tests/test_occlusion_map_cpu.py, tests/test_gpu_occlusion_map.py): the bar, planted
populations and planes, and the numpy restatement of the per-body summary.  The rule itself is restated in
dbot_ros_amd.tracker.occlusion_map_of (np.longdouble).

The bar.  With T(p) the twin's longdouble value over the planes rbs_get_occlusion hands out,
    |M_dev(p) - T(p)| <= 1/2 spacing32(T(p)) + (n + 16) 2^-52.
The first term is the one rounding of the binary64 quotient to float.  The second bounds the binary64 work in front of it:
every v_s is in [0, 1] and every term is positive, so sum W_s v_s / S <= 1 and each of the at most n additions of W_s, of S
and of the per-pixel sum, each product, the quotient and the exp of a weight (a couple of ulps of a number <= 1) moves the
result by at most a few 2^-53 relative to a value <= 1: (n + 16) 2^-52 covers them with room and is still 5 000 times
smaller than a float's half spacing near 1/2 at n = 300."""
import numpy as np

import assess_twin as at

LD = np.longdouble
SIZES = [1, 2, 63, 64, 65, 300]


def spacing32_below(t):
    """The spacing of the float32 grid at |t| (the binade |t| lies in, not the one its rounding may reach)."""
    a = np.abs(np.asarray(t, dtype=LD))
    f = a.astype(np.float32)
    f = np.where(f.astype(LD) > a, np.nextafter(f, np.float32(0)), f).astype(np.float32)
    return np.spacing(f).astype(LD)


def bar(t, n):
    return LD(0.5) * spacing32_below(t) + LD(n + 16) * LD(2.0) ** -52


def check(m_dev, twin, n, note=None, what=""):
    """The bar at every pixel; note[what] keeps the worst share of the bar seen."""
    err = np.abs(np.asarray(m_dev, dtype=np.float32).ravel().astype(LD) - twin)
    share = float((err / bar(twin, n)).max())
    if note is not None:
        note[what] = max(note.get(what, 0.0), share)
    assert share <= 1.0, (what, n, share, int(np.argmax(err / bar(twin, n))))
    return share


def slot_patterns(n, slots, rng):
    i = np.arange(n)
    return {"one_slot": np.full(n, min(3, slots - 1)), "by_sevens": (i // 7) % slots, "round_robin": i % slots,
            "random": rng.integers(0, slots, n)}


def weight_patterns(n, rng):
    lw = rng.normal(0.0, 3.0, n)
    holes = lw.copy()
    holes[::3] = -np.inf
    if not np.isfinite(holes).any():
        holes[-1] = 0.0
    if n > 1:
        holes[-1] = -1.5          # (at least one finite weight, and not the first)
    dominant = rng.uniform(-40.0, -30.0, n)
    dominant[n // 2] = 0.0
    return {"uniform": None, "with_minus_inf": holes, "dominant": dominant}


def populations(slots, seed=0):
    """(name, n, indices int32 [n], log-weights [n] or None) over every size, slot pattern and weight pattern."""
    rng = np.random.default_rng(seed)
    out = []
    for n in SIZES:
        for sn, idx in slot_patterns(n, slots, rng).items():
            for wn, lw in weight_patterns(n, rng).items():
                out.append((f"n{n}-{sn}-{wn}", n, idx.astype(np.int32), lw))
    return out


def planted_planes(rows, cols, slots, bg, seed=0):
    """{slot: plane}: values in [0, 1] over rectangles of different places and sizes (one touching the frame's corner), the
    background elsewhere; slot 0 all background (its window is empty)."""
    rng = np.random.default_rng(seed)
    out = {0: np.full(rows * cols, bg, dtype=np.float32)}
    boxes = [(0, 0, 12, 9), (cols - 16, rows - 7, cols, rows), (20, 10, 52, 41), (4, 30, 24, 50), (40, 5, 44, 6)]
    for s, (x0, y0, x1, y1) in zip(range(1, slots), boxes):
        p = np.full((rows, cols), bg, dtype=np.float32)
        p[y0:y1, x0:x1] = rng.uniform(0.0, 1.0, (y1 - y0, x1 - x0)).astype(np.float32)
        out[s] = p.ravel()
    return out


def inside(win, rows, cols):
    """Boolean [rows*cols]: the pixels of window (x0, y0, x1, y1)."""
    m = np.zeros((rows, cols), dtype=bool)
    x0, y0, x1, y1 = win
    if x1 > x0 and y1 > y0:
        m[y0:y1, x0:x1] = True
    return m.ravel()


def bodies_of(planes, m, threshold):
    """The per-body summary restated: planes [B, npx] of one pose (inf where a body has no surface or outside its rectangle,
    as rbs_assess_get_plane hands them out), m [npx] float32 -> int64 [B, 3] of rendered, occluded, sum_q32.  The owner of
    a pixel is assess_twin.owners': the nearest plane, a tie with the lowest body, no owner where every plane is inf."""
    planes = np.asarray(planes, dtype=np.float32)
    owner, _ = at.owners(planes)
    md = np.asarray(m, dtype=np.float32).astype(np.float64)
    q = np.floor(md * 4294967296.0).astype(np.uint64)      # exact: a float times 2^32 is a binary64 number
    out = np.zeros((planes.shape[0], 3), dtype=np.int64)
    for b in range(planes.shape[0]):
        mine = owner == b
        out[b] = [int(mine.sum()), int((md[mine] > threshold).sum()), int(q[mine].sum(dtype=np.uint64))]
    return out
