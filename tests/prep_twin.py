"""Plain numpy reference of the rectangles kernel (dbot_ros_amd/csrc/rbsensor_kernels.hip prep_particles), written from
DESIGN.md sections 3 / 4 and the comments above `Groups` and `Strips`, and the checkers tests/test_gpu_prep_kernels.py applies
to what the device hands back (tests/test_prep_twin_cpu.py runs every checker on the twin's own outputs and on planted
mistakes).  Test infrastructure.

Rectangles are (x0, y0, x1, y1), half open; EMPTY is the empty window marker (cols, rows, 0, 0) -- unions are plain min / max --
and an empty screen rectangle is (0, 0, 0, 0).  Every checker returns a list of complaints, empty when it has none."""
import numpy as np

MAX_GROUPS = 4                                        # kMaxGroups
MAX_STRIPS = (2 * MAX_GROUPS + 1) * (MAX_GROUPS + 1)  # kMaxStrips
PREP_PER_BLOCK = 8                                    # kPrepPerBlock
Z_FULL = 1e-4                                         # a vertex this close to the camera plane (or behind it): the whole frame
Z_CLEAR = 1.01e-4                                     # from here on the rectangle must be the projection's
LD = np.longdouble


# ---------------------------------------------------------------- work-item tiles
def tile_grid(rw, rh, max_w, cap_px):
    """-> (tw, th, nx, ny): nx columns of equal 16-aligned width <= max_w, then as few equal rows as keep a tile within cap_px."""
    nx = max(1, -(-rw // max_w))
    tw = max(16, (-(-rw // nx) + 15) // 16 * 16)
    hmax = max(1, cap_px // tw)
    ny = max(1, -(-rh // hmax))
    th = max(1, -(-rh // ny))
    return tw, th, nx, ny


def tiles_upper_bound(cols, rows, max_w, cap_px):
    """Most work items a rectangle inside the frame splits into, as the host sizes its buffers: the widths that are multiples
    of 16 at full height."""
    worst = 1
    for rw in range(16, (cols + 15) // 16 * 16 + 1, 16):
        _, _, nx, ny = tile_grid(rw, rows, max_w, cap_px)
        worst = max(worst, nx * ny)
    return worst


def cap_px(tile_w, tile_h, tile_px):
    return min(tile_w * tile_h, tile_px)


def tile_count(rect, tile_w, tile_h, tile_px):
    """Work items of one rectangle; an empty one still owns one (empty) item."""
    x0, y0, x1, y1 = rect
    if x1 <= x0:
        return 1
    _, _, nx, ny = tile_grid(x1 - x0, y1 - y0, tile_w, cap_px(tile_w, tile_h, tile_px))
    return nx * ny


# ---------------------------------------------------------------- exact projection
def project(vtx, pose):
    """Vertices [nv][>= 3] float32 (widened exactly) under a pose [12] binary64 (rotation row-major, translation), pinhole
    transform in long double -> camera-frame points [nv][3]."""
    p = np.asarray(vtx, dtype=np.float32)[:, :3].astype(LD)
    q = np.asarray(pose, dtype=np.float64).astype(LD)
    R, t = q[:9].reshape(3, 3), q[9:12]
    with np.errstate(all="ignore"):
        X = p @ R.T + t
    return X


def extents(bodies, poses, K):
    """bodies: list of vertex arrays; poses [len(bodies)][12]; K = (fx, fy, cx, cy) -> the union's (umin, umax, vmin, vmax, zmin)
    in long double, `finite` (every pose entry is), and tabs = max over the bodies of |tx| + |ty| + |tz|."""
    fx, fy, cx, cy = (LD(k) for k in K)
    poses = np.asarray(poses, dtype=np.float64).reshape(len(bodies), 12)
    finite = bool(np.isfinite(poses).all())
    e = dict(umin=LD(np.inf), umax=LD(-np.inf), vmin=LD(np.inf), vmax=LD(-np.inf), zmin=LD(np.inf), finite=finite,
             tabs=float(np.abs(poses[:, 9:12]).sum(axis=1).max()))
    if not finite:
        return e
    for vtx, pose in zip(bodies, poses):
        if len(vtx) == 0:
            continue
        X = project(vtx, pose)
        Z = X[:, 2]
        e["zmin"] = min(e["zmin"], Z.min())
        front = Z > 0
        if front.any():
            u = fx * X[front, 0] / Z[front] + cx
            v = fy * X[front, 1] / Z[front] + cy
            e["umin"], e["umax"] = min(e["umin"], u.min()), max(e["umax"], u.max())
            e["vmin"], e["vmax"] = min(e["vmin"], v.min()), max(e["vmax"], v.max())
    return e


def margin(e, K):
    """The margin the kernel states for its float32 arithmetic (the formula above the rounding of the rectangle in bodies_rect),
    in binary64 from the exact extents -> (mx, my) pixels."""
    fx, fy, cx, cy = (float(k) for k in K)
    zmin = float(e["zmin"])
    mx = 4e-6 * fx * (e["tabs"] + 1.0) / zmin + 3e-7 * (abs(float(e["umin"]) - cx) + abs(float(e["umax"]) - cx)) + 1e-3
    my = 4e-6 * fy * (e["tabs"] + 1.0) / zmin + 3e-7 * (abs(float(e["vmin"]) - cy) + abs(float(e["vmax"]) - cy)) + 1e-3
    return mx, my


def _clamp(x, hi):
    """An extended-precision coordinate, already floored or ceiled, as a pixel index in [0, hi]."""
    return int(min(max(x, LD(0)), LD(hi)))


def rect_bars(e, K, cols, rows, align):
    """-> (inner, outer): the rectangle must contain `inner` (the exact projection's pixels, clamped to the frame; None when
    there are none) and lie inside `outer` (the projection grown by twice the stated margin, x aligned)."""
    mx, my = margin(e, K)
    ix0, ix1 = _clamp(np.floor(e["umin"]), cols), _clamp(np.floor(e["umax"]) + 1, cols)
    iy0, iy1 = _clamp(np.floor(e["vmin"]), rows), _clamp(np.floor(e["vmax"]) + 1, rows)
    inner = (ix0, iy0, ix1, iy1) if ix1 > ix0 and iy1 > iy0 else None
    ox0 = _clamp(np.floor(e["umin"] - 2 * LD(mx)), cols) // align * align
    ox1 = min(cols, -(-_clamp(np.ceil(e["umax"] + 2 * LD(mx)) + 1, cols) // align) * align)
    oy0, oy1 = _clamp(np.floor(e["vmin"] - 2 * LD(my)), rows), _clamp(np.ceil(e["vmax"] + 2 * LD(my)) + 1, rows)
    return inner, (ox0, oy0, ox1, oy1)


def check_rect(rect, e, K, cols, rows, align):
    """The bars of one screen rectangle against the exact extents `e` of what it is the rectangle of."""
    x0, y0, x1, y1 = (int(k) for k in rect)
    bad = []
    full = (x0, y0, x1, y1) == (0, 0, cols, rows)
    if x1 <= x0 or y1 <= y0:
        if (x0, y0, x1, y1) != (0, 0, 0, 0):
            bad.append(f"an empty rectangle is (0, 0, 0, 0), not {rect}")
    else:
        if not (0 <= x0 < x1 <= cols and 0 <= y0 < y1 <= rows):
            bad.append(f"{rect} leaves the frame")
        if x0 % align or (x1 % align and x1 != cols):
            bad.append(f"x edges of {rect} are not multiples of {align}")
    must_full = (not e["finite"]) or e["zmin"] <= LD(Z_FULL)
    if must_full:
        if not full:
            bad.append(f"zmin {float(e['zmin']):.6g} / finite {e['finite']}: the whole frame, not {rect}")
        return bad
    if e["zmin"] < LD(Z_CLEAR) and full:
        return bad          # (between the two thresholds either answer stands)
    inner, outer = rect_bars(e, K, cols, rows, align)
    if inner is not None:
        if x1 <= x0:
            bad.append(f"empty, but the projection covers {inner}")
        elif not (x0 <= inner[0] and y0 <= inner[1] and x1 >= inner[2] and y1 >= inner[3]):
            bad.append(f"containment: {rect} does not contain {inner}")
    if x1 > x0 and not (x0 >= outer[0] and y0 >= outer[1] and x1 <= outer[2] and y1 <= outer[3]):
        bad.append(f"tightness: {rect} is not inside {outer}")
    return bad


def rect_slack(rect, e, cols, rows):
    """The least distance, in pixels, between an edge of the rectangle that is not the frame's and the exact projection's
    extreme coordinate on that side (what is left of the margin on the containment side; inf: every edge is the frame's)."""
    x0, y0, x1, y1 = (int(k) for k in rect)
    slack = np.inf
    for lo, hi, a, b, size in ((x0, x1, e["umin"], e["umax"], cols), (y0, y1, e["vmin"], e["vmax"], rows)):
        if lo > 0:
            slack = min(slack, float(a - lo))
        if hi < size:
            slack = min(slack, float(hi - b))
    return slack


# ---------------------------------------------------------------- composed poses
def rotvec_matrix_ld(rv):
    rv = np.asarray(rv, dtype=np.float64).astype(LD)
    angle = np.sqrt((rv * rv).sum())
    if angle == 0:
        return np.eye(3, dtype=LD)
    k = rv / angle
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]], dtype=LD)
    return np.eye(3, dtype=LD) + np.sin(angle) * Kx + (1 - np.cos(angle)) * (Kx @ Kx)    # Rodrigues


def compose_ld(delta, default):
    """(position, rotation vector) delta and default pose [6] each -> absolute pose [12] in long double:
    R = R(delta) R(default), t = t(delta) + t(default)."""
    d, d0 = np.asarray(delta, dtype=np.float64), np.asarray(default, dtype=np.float64)
    R = rotvec_matrix_ld(d[3:6]) @ rotvec_matrix_ld(d0[3:6])
    return np.concatenate([R.ravel(), d[:3].astype(LD) + d0[:3].astype(LD)])


# ---------------------------------------------------------------- groups
def overlap(a, b):
    """Strict: rectangles that only abut do not overlap."""
    return a[0] < b[2] and b[0] < a[2] and a[1] < b[3] and b[1] < a[3]


def union(a, b):
    return (min(a[0], b[0]), min(a[1], b[1]), max(a[2], b[2]), max(a[3], b[3]))


def partition(body_rects):
    """The finest partition of the bodies with a non-empty rectangle whose blocks' bounding boxes are pairwise non-overlapping
    -> {(rect, mask)} (unique whatever the order of the merges)."""
    blocks = [(tuple(int(k) for k in r), 1 << b) for b, r in enumerate(body_rects) if r[2] > r[0]]
    merged = True
    while merged:
        merged = False
        for i in range(len(blocks)):
            hit = [j for j in range(len(blocks)) if j != i and overlap(blocks[i][0], blocks[j][0])]
            if hit:
                r, m = blocks[i]
                for j in hit:
                    r, m = union(r, blocks[j][0]), m | blocks[j][1]
                blocks = [blk for j, blk in enumerate(blocks) if j != i and j not in hit] + [(r, m)]
                merged = True
                break
    return set(blocks)


def groups(body_rects):
    """... as the particle's groups: more than MAX_GROUPS blocks are one union rectangle with every mask."""
    P = partition(body_rects)
    if len(P) > MAX_GROUPS:
        r, m = None, 0
        for br, bm in P:
            r, m = (br if r is None else union(r, br)), m | bm
        P = {(r, m)}
    return P


def union_rect(group_set):
    r = None
    for br, _ in group_set:
        r = br if r is None else union(r, br)
    return r if r is not None else (0, 0, 0, 0)


def check_groups(dev, body_rects, tile_w, tile_h, tile_px, cnt):
    """dev: [(rect, mask, first)] in stored order; cnt: the particle's item count."""
    bad = []
    want = groups(body_rects)
    got = [(tuple(int(k) for k in r), int(m)) for r, m, _ in dev]
    if len(got) > MAX_GROUPS:
        bad.append(f"{len(got)} groups")
    if set(got) != want or len(got) != len(want):
        bad.append(f"groups {sorted(got)} != {sorted(want)}")
    for i in range(len(got)):
        for j in range(i + 1, len(got)):
            if overlap(got[i][0], got[j][0]):
                bad.append(f"groups {got[i][0]} and {got[j][0]} overlap")
    at = 0
    for r, _, first in dev:
        if int(first) != at:
            bad.append(f"group {tuple(r)} starts at item {first}, not {at}")
        at = int(first) + tile_count(r, tile_w, tile_h, tile_px)
    if at != (cnt if dev else 0) or (not dev and cnt != 1):
        bad.append(f"the groups' spans end at {at}, the particle has {cnt} items")
    return bad


# ---------------------------------------------------------------- items
def check_items(item_range, item_particle, total, counts, bound):
    """item_range [n][2], item_particle [>= total], total = ctr_this[0], counts [n] the twin's tile counts, bound the most a
    particle may have: ranges pairwise disjoint, covering [0, total) exactly, each naming its owner."""
    bad = []
    n = len(item_range)
    owner = np.full(max(int(total), 0), -1, dtype=np.int64)
    for i in range(n):
        first, cnt = int(item_range[i][0]), int(item_range[i][1])
        if cnt != counts[i]:
            bad.append(f"particle {i}: {cnt} items, the twin has {counts[i]}")
        if cnt > bound:
            bad.append(f"particle {i}: {cnt} items exceed the bound {bound}")
        if first < 0 or cnt < 1 or first + cnt > total:
            bad.append(f"particle {i}: range [{first}, {first + cnt}) outside [0, {total})")
            continue
        if (owner[first:first + cnt] != -1).any():
            bad.append(f"particle {i}: range [{first}, {first + cnt}) overlaps particle {int(owner[first:first + cnt].max())}'s")
        owner[first:first + cnt] = i
        if not np.array_equal(item_particle[first:first + cnt], np.full(cnt, i)):
            bad.append(f"particle {i}: item_particle[{first}:{first + cnt}] = {item_particle[first:first + cnt]}")
    if (owner == -1).any():
        bad.append(f"{int((owner == -1).sum())} of {total} items belong to nobody")
    return bad


# ---------------------------------------------------------------- regions
def empty(cols, rows):
    return (cols, rows, 0, 0)


def area(r):
    return (r[2] - r[0]) * (r[3] - r[1]) if r[2] > r[0] and r[3] > r[1] else 0


def region(rect, parent, win_src, slots, rebase_box, cols, rows, slab_px):
    """One particle of an updating call on windowed planes -> dict(win_used, win_dst, reg_dst (None without slabs), parent (as
    stored), area (asked for), overflow)."""
    E = empty(cols, rows)
    rw = tuple(int(k) for k in rect) if rect[2] > rect[0] else E
    pw = tuple(int(k) for k in win_src[parent]) if 0 <= parent < slots else E
    u = union(pw, rw)
    if rebase_box is not None:
        u = union(u, tuple(int(k) for k in rebase_box))
    out = dict(win_used=u, win_dst=rw, reg_dst=None, parent=int(parent), area=area(u), overflow=False)
    if slab_px:
        if out["area"] > slab_px:
            out.update(win_used=E, win_dst=E, parent=-1, overflow=True)
        out["reg_dst"] = out["win_used"]
    return out


def check_region(got, want):
    return [f"{k}: {tuple(int(x) for x in got[k])} != {want[k]}" for k in ("win_used", "win_dst", "reg_dst")
            if want[k] is not None and tuple(int(x) for x in got[k]) != tuple(want[k])]


# ---------------------------------------------------------------- strips
def strip_mask(win_used, group_rects, cols, rows):
    """What the copy kernel writes of a particle's region: the region minus the union of its groups' rectangles, as pixels."""
    m = np.zeros((rows, cols), dtype=bool)
    x0, y0, x1, y1 = win_used
    if x1 > x0 and y1 > y0:
        m[y0:y1, x0:x1] = True
    for gx0, gy0, gx1, gy1 in group_rects:
        m[gy0:gy1, gx0:gx1] = False
    return m


def check_strips(n, first, box, win_used, group_rects, cols, rows):
    """n, first [MAX_STRIPS + 1], box [MAX_STRIPS][4] = (x0 / 4, x1 / 4, y0, y1) as stored."""
    bad = []
    if not 0 <= n <= MAX_STRIPS:
        return [f"{n} strips"]
    img = np.zeros((rows, cols), dtype=np.int32)
    cells = 0
    for s in range(n):
        bx0, bx1, by0, by1 = (int(k) for k in box[s])
        if int(first[s]) != cells:
            bad.append(f"strip {s}: first {int(first[s])}, the running cell count is {cells}")
        if not (bx0 < bx1 and by0 < by1 and 4 * bx1 <= cols and by1 <= rows):
            bad.append(f"strip {s}: box {(bx0, bx1, by0, by1)}")
            continue
        img[by0:by1, 4 * bx0:4 * bx1] += 1
        cells += (bx1 - bx0) * (by1 - by0)
    if int(first[n]) != cells:
        bad.append(f"first[n] = {int(first[n])}, the strips hold {cells} cells")
    if (img > 1).any():
        bad.append(f"{int((img > 1).sum())} pixels painted twice")
    want = strip_mask(win_used, group_rects, cols, rows)
    if not np.array_equal(img > 0, want):
        bad.append(f"strips cover {int((img > 0).sum())} px, the region minus the groups has {int(want.sum())}: "
                   f"{int(((img > 0) & ~want).sum())} too many, {int((~(img > 0) & want).sum())} missing")
    return bad


def strips(win_used, group_rects):
    """The twin's own strip list (bands between the rectangles' top and bottom edges, within a band the intervals no rectangle
    covers), for the CPU test: -> (n, first [MAX_STRIPS + 1], box [MAX_STRIPS][4])."""
    x0, y0, x1, y1 = win_used
    first, box = np.zeros(MAX_STRIPS + 1, dtype=np.int32), np.zeros((MAX_STRIPS, 4), dtype=np.int32)
    n = cells = 0
    if x1 > x0 and y1 > y0:
        ys = sorted({y0, y1} | {min(max(y, y0), y1) for r in group_rects for y in (r[1], r[3])})
        for ya, yb in zip(ys[:-1], ys[1:]):
            spans = sorted((max(r[0], x0), min(r[2], x1)) for r in group_rects if r[1] <= ya and r[3] >= yb and r[2] > r[0])
            cur = x0
            for a, b in spans + [(x1, x1)]:
                if a > cur:
                    first[n], box[n] = cells, (cur // 4, a // 4, ya, yb)
                    cells += (a - cur) // 4 * (yb - ya)
                    n += 1
                cur = max(cur, b)
    first[n] = cells
    return n, first, box
