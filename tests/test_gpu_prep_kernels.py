"""The rectangles kernel (dbot_ros_amd/csrc/rbsensor_kernels.hip prep_particles: rbs_prep_kernel, rbs_prep_deltas_kernel and the
prep blocks of rbs_frame_prep_kernel) ON THE DEVICE, output by output, against the plain reference tests/prep_twin.py.

The test build of the library (librbsensor_mi355x_hooks.so) has rbs_test_prep: it builds the kernels' parameter block from
host arrays (vertex clouds, poses, parent windows) and launches through launch_prep, the helper enqueue_loglikes itself calls;
every output comes back whole, with a sentinel-filled tail (tests/prep_probes.py).

Bars.  Everything integer is exact: groups as a set of (rectangle, mask) against the twin's finest
partition of the kernel's own per-body rectangles, item ranges, parents, regions, windows, slab flags, the strips as a painted
image against the region minus the groups.  The rectangle itself is float32 arithmetic behind a stated margin m and is held
between two integer bars from the long-double projection of the same float32 vertices: it contains floor(umin) ..
floor(umax) + 1 (clamped to the frame) and lies inside floor(umin - 2 m) .. ceil(umax + 2 m) + 1 (x aligned).  Composed poses
(rbs_prep_deltas_kernel): translations exact, rotation entries within 64 * 2^-53 of the long-double composition.

The probes exist in the hooks build only, and two builds of the library do not share a process: outside a process that has
loaded the hooks build, the first test here re-runs this file once in a child with RBS_LIB_PATH set to it, and every test
reports its own outcome of that run."""
import os

import numpy as np
import pytest

import prep_probes as pp
import prep_twin as tw
from dbot_ros_amd import _capi
from prep_probes import ROUTE_DELTAS, ROUTE_DEVICE, ROUTE_HOST, TAIL, untouched

pytestmark = pytest.mark.gpu

HOOKS = pp.hooks_path(_capi.LIB_PATH)
IN_HOOKS_PROCESS = os.path.abspath(_capi.LIB_PATH) == os.path.abspath(HOOKS)
_child = {}
figures = {"margin": 0.0, "slack": np.inf, "pose": 0.0}     # printed by the tests that measure them

SIZES = {64: (64, 48, (56.0, 56.0, 31.5, 23.5), (32, 8, 8192)), 160: (160, 120, (140.0, 140.0, 79.5, 59.5), (64, 16, 8192)),
         640: (640, 480, (560.0, 560.0, 319.5, 239.5), (256, 43, 11008))}      # cols, rows, K, (tile_w, tile_h, tile_px): 640 as the library runs
POSE_TOL = 64 * 2.0 ** -53
INT_OUTPUTS = ("rects", "groups", "strips", "parents", "ctr_this", "done", "win_used", "win_dst", "reg_dst", "err")


def _delegated(request):
    """True: this process has not loaded the hooks build -- the test's outcome is the one of the child run."""
    if IN_HOOKS_PROCESS:
        return False
    if not _child:
        assert os.path.exists(HOOKS), "build() makes librbsensor_mi355x_hooks.so"
        _child["outcome"], _child["out"] = pp.child_outcomes(__file__, HOOKS, 600)
    assert _child["outcome"].get(request.node.name) == "PASSED", _child["out"]
    return True


@pytest.fixture(scope="module")
def probe(gpu_lib):
    return pp.PrepProbe(HOOKS) if IN_HOOKS_PROCESS else None


# ---------------------------------------------------------------- inputs
def _rot(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _pose(t, R=None):
    return np.concatenate([(np.eye(3) if R is None else R).ravel(), np.asarray(t, dtype=np.float64)])


def _cloud(rng, nv, radius=0.04):
    return rng.uniform(-radius, radius, size=(nv, 3)).astype(np.float32)


def _at(K, u, v, z):
    return ((u - K[2]) / K[0] * z, (v - K[3]) / K[1] * z, z)


def _battery(cols, rows, K, body, rng):
    """[(name, pose)] of one small body: the poses of the issue's list that one set of vertices can take."""
    out = [("centred", _pose(_at(K, cols / 2, rows / 2, 0.6), _rot(rng)))]
    for name, (u, v) in dict(left=(0, rows / 2), right=(cols, rows / 2), top=(cols / 2, 0), bottom=(cols / 2, rows), tl=(0, 0), tr=(cols, 0),
                             bl=(0, rows), br=(cols, rows)).items():
        out.append(("straddling " + name, _pose(_at(K, u, v, 0.6), _rot(rng))))
    for name, (u, v) in dict(left=(-cols, rows / 2), right=(2 * cols, rows / 2), top=(cols / 2, -rows), bottom=(cols / 2, 2 * rows)).items():
        out.append(("off " + name, _pose(_at(K, u, v, 0.6), _rot(rng))))
    out.append(("just off right", _pose(_at(K, cols + 0.04 * K[0] / 0.6 + 1.5, rows / 2, 0.6))))
    for z in (0.3, 1.0, 3.0):
        out.append((f"z {z}", _pose(_at(K, cols * 0.4, rows * 0.6, z), _rot(rng))))
    out.append(("close", _pose((0.01, -0.01, 0.09), _rot(rng))))
    out.append(("behind", _pose((0.0, 0.0, 0.02))))                       # vertices at Z <= 0
    zlo = float(body[:, 2].astype(np.float64).min())
    for f in (0.5, 0.99, 1.011, 1.05, 2.0):                                # zmin on either side of 1e-4 (identity rotation: Z = z + tz, one rounding)
        out.append((f"zmin {f}e-4", _pose((0.003, -0.002, f * 1e-4 - zlo))))
    for k, bad in ((0, np.nan), (1, np.inf), (4, np.nan), (8, -np.inf), (6, np.nan), (9, np.nan), (10, np.inf), (11, np.nan), (9, -np.inf)):
        p = _pose(_at(K, cols / 2, rows / 2, 0.6), _rot(rng))
        p[k] = bad
        out.append((f"pose[{k}] = {bad}", p))
    return out


def _check_rects(res, bodies_of, poses, K, cols, rows, align, names=None):
    """Every particle's rectangle against the bars; notes the margin and the slack."""
    for i in range(res.n):
        e = tw.extents(bodies_of, poses[i], K)
        r = tuple(int(k) for k in res.rects[i])
        bad = tw.check_rect(r, e, K, cols, rows, align)
        assert not bad, (names[i] if names else i, r, bad, {k: float(v) for k, v in e.items()})
        if e["finite"] and e["zmin"] >= tw.LD(tw.Z_CLEAR) and r[2] > r[0] and r != (0, 0, cols, rows):
            figures["margin"] = max(figures["margin"], *tw.margin(e, K))
            figures["slack"] = min(figures["slack"], tw.rect_slack(r, e, cols, rows))


def _same_outputs(a, b, skip=()):
    """Two calls on the same inputs: every output but the items' PLACES (any free range will do: the blocks bump the counter
    in the order they run) is the same."""
    for k in INT_OUTPUTS:
        if k in skip or a[k] is None:
            continue
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(a.item_range[:, 1], b.item_range[:, 1])
    assert np.array_equal(a.poses.view(np.uint64), b.poses.view(np.uint64))


def _check_tails(res, groups=False, strips=False, regions=True):
    n = res.n
    for k in ("rects", "parents", "item_range", "done") + (("win_used", "win_dst") if regions else ()) + (("groups",) if groups else ()) + \
            (("strips",) if strips else ()):
        assert untouched(res[k][n:]), k
    assert untouched(res.poses[n * res.B * 12:]) and untouched(res.ctr_this[2:]) and untouched(res.err[2:])
    total = int(res.ctr_this[0])
    assert untouched(res.item_particle[total:]), "item_particle beyond the items allotted"
    assert int(res.ctr_this[1]) == 0


def _counts(res, tiles, groups):
    if groups:
        return [sum(tw.tile_count(r, *tiles) for r, _, _ in res.group_list(i)) or 1 for i in range(res.n)]
    return [tw.tile_count(res.rects[i], *tiles) for i in range(res.n)]


def _check_items(res, tiles, groups=False):
    total = int(res.ctr_this[0])
    bound = res.tiles_ub * (tw.MAX_GROUPS if groups else 1)
    assert res.tiles_ub == tw.tiles_upper_bound(res.cols_, res.rows_, tiles[0], tw.cap_px(*tiles))
    bad = tw.check_items(res.item_range[:res.n], res.item_particle, total, _counts(res, tiles, groups), bound)
    assert not bad, bad
    assert (res.done[:res.n] == 0).all()


def _run(probe, size, bodies, poses, indices=None, **kw):
    cols, rows, K, tiles = SIZES[size]
    kw.setdefault("tile_w", tiles[0]), kw.setdefault("tile_h", tiles[1]), kw.setdefault("tile_px", tiles[2])
    res = probe.run(rows, cols, K, bodies, poses, indices, **kw)
    res["cols_"], res["rows_"] = cols, rows
    return res


# ---------------------------------------------------------------- rectangles, one body
@pytest.mark.parametrize("align", [4, 8, 16])
@pytest.mark.parametrize("size", [64, 160, 640])
def test_rectangle_of_one_body_over_the_pose_battery(request, probe, size, align):
    """Every pose of the battery, on the device-array and the pinned-host route: the bars, the items, the tails; the two routes
    agree in every output."""
    if _delegated(request):
        return
    cols, rows, K, tiles = SIZES[size]
    rng = np.random.default_rng([size, align])
    figures.update(margin=0.0, slack=np.inf)
    body = _cloud(rng, 65)
    names, poses = zip(*_battery(cols, rows, K, body, rng))
    poses = np.array(poses)[:, None, :]
    idx = np.arange(len(poses), dtype=np.int32)
    a = _run(probe, size, [body], poses, idx, rect_align=align, windowed=0)
    _check_rects(a, [body], poses, K, cols, rows, align, names)
    _check_items(a, tiles)
    _check_tails(a, regions=False)
    assert untouched(a.win_used) and untouched(a.win_dst) and untouched(a.reg_dst) and (a.err[:2] == 0).all()     # whole planes: no regions
    assert np.array_equal(a.parents[:a.n], idx)
    assert np.array_equal(a.poses[:poses.size].view(np.uint64), poses.ravel().view(np.uint64))
    full = [n for n, r in zip(names, a.rects) if tuple(r) == (0, 0, cols, rows)]
    assert {"behind", "zmin 0.5e-4", "zmin 0.99e-4"} <= set(full) and "centred" not in full, full
    assert all(tuple(a.rects[names.index("off " + s)]) == (0, 0, 0, 0) for s in ("left", "right", "top", "bottom"))
    b = _run(probe, size, [body], poses, idx, rect_align=align, windowed=0, route=ROUTE_HOST)
    _same_outputs(a, b)
    print(f"\nrectangles {cols}x{rows} align {align}: stated margin up to {figures['margin']:.4g} px, least containment slack {figures['slack']:.4g} px")


def test_rectangle_on_either_side_of_the_camera_plane_threshold(request, probe):
    """Vertices on rays through the middle of the frame, the nearest at f * 1e-4 m, under the identity pose (Z is then the
    vertex's own float32 z, exactly): at or below 1e-4 the whole frame, from 1.01e-4 on the projection's rectangle."""
    if _delegated(request):
        return
    cols, rows, K, tiles = SIZES[160]
    rng = np.random.default_rng(4)
    for f, whole in ((0.5, True), (0.99, True), (1.0, True), (1.011, False), (1.05, False), (2.0, False)):
        u, v, z = rng.uniform(0.3 * cols, 0.6 * cols, 40), rng.uniform(0.4 * rows, 0.7 * rows, 40), f * 1e-4 * rng.uniform(1.0, 3.0, 40)
        z[7] = f * 1e-4
        body = np.stack([(u - K[2]) / K[0] * z, (v - K[3]) / K[1] * z, z], axis=1).astype(np.float32)
        poses = np.array([_pose((0, 0, 0)), _pose((0, 0, 0), np.diag([1.0, 1.0, 1.0])), _pose((2e-6 * f, -1e-6 * f, 0))])[:, None, :]
        res = _run(probe, 160, [body], poses, rect_align=4, windowed=0)
        assert float(tw.extents([body], poses[0], K)["zmin"]) == float(np.float32(f * 1e-4))
        _check_rects(res, [body], poses, K, cols, rows, 4, [f] * 3)
        assert all((tuple(r) == (0, 0, cols, rows)) == whole for r in res.rects[:3]), (f, res.rects[:3])


@pytest.mark.parametrize("axis", ["u", "v"])
@pytest.mark.parametrize("nv", [1, 3, 63, 64, 65, 511, 512, 513, 1100])
def test_rectangle_sees_the_extreme_vertex_wherever_it_sits(request, probe, nv, axis):
    """The vertex that alone decides an edge, at the first and the last position and on either side of the lanes' strides (64
    lanes, eight loads in flight: 512 per trip); the tail of the last trip repeats the last vertex and must not lose it."""
    if _delegated(request):
        return
    cols, rows, K, tiles = SIZES[160]
    rng = np.random.default_rng([nv, axis == "u"])
    figures.update(margin=0.0, slack=np.inf)
    poses = np.array([_pose(_at(K, 60.3, 50.2, 0.6)), _pose(_at(K, 100.7, 70.9, 0.45)), _pose(_at(K, 150.2, 20.1, 0.6)), _pose(_at(K, 80, 5.5, 1.0))])[:, None, :]
    for where in sorted({0, nv - 1} | {k for k in (63, 64, 511, 512) if k < nv}):
        for sign in (1.0, -1.0):
            body = _cloud(rng, nv, 0.03)
            body[where, 0 if axis == "u" else 1] = sign * 0.075                       # ~17 px beyond the others at 0.6 m
            res = _run(probe, 160, [body], poses, rect_align=4, windowed=0)
            _check_rects(res, [body], poses, K, cols, rows, 4, [(nv, where, sign)] * 4)
            _check_items(res, tiles)
    print(f"\nplanted vertices: stated margin up to {figures['margin']:.4g} px, least containment slack {figures['slack']:.4g} px")


@pytest.mark.parametrize("size", [160, 640])
def test_rectangle_near_the_camera_where_float32_is_coarsest(request, probe, size):
    """Vertices a few metres from the model's origin that the pose brings back to within zmin of the camera plane: R p and t
    cancel, and the float32 error of X, Y, Z -- which the margin has to cover -- is at its largest against Z."""
    if _delegated(request):
        return
    cols, rows, K, tiles = SIZES[size]
    rng = np.random.default_rng(size)
    figures.update(margin=0.0, slack=np.inf)
    for zmin in (2e-4, 1e-3, 0.02, 0.1):
        for tnorm in (0.5, 3.0):
            n = 8
            u, v, z = rng.uniform(-0.1 * cols, 1.1 * cols, 200), rng.uniform(-0.1 * rows, 1.1 * rows, 200), zmin * (1 + rng.uniform(0, 2.0, 200) ** 2)
            z[17] = zmin
            q = np.stack([(u - K[2]) / K[0] * z, (v - K[3]) / K[1] * z, z], axis=1)
            R, t = _rot(rng), rng.normal(size=3)
            t *= tnorm / np.linalg.norm(t)
            body = ((q - t) @ R).astype(np.float32)                                 # p = R^T (q - t)
            # the particles: the pose itself, and small shifts of it that keep the cloud in front of the camera
            poses = np.array([_pose(t + d, R) for d in [np.zeros(3)] + [np.array([*(rng.normal(size=2) * zmin * 0.2), abs(rng.normal()) * zmin]) for _ in range(n - 1)]])[:, None, :]
            res = _run(probe, size, [body], poses, rect_align=4, windowed=0)
            e0 = tw.extents([body], poses[0], K)
            assert abs(float(e0["zmin"]) / zmin - 1) < 0.01, float(e0["zmin"])
            _check_rects(res, [body], poses, K, cols, rows, 4, [(zmin, tnorm, k) for k in range(n)])
            _check_items(res, tiles)
    print(f"\nnear the camera {cols}x{rows}: stated margin up to {figures['margin']:.4g} px, least containment slack {figures['slack']:.4g} px")


# ---------------------------------------------------------------- composed poses
def test_composed_poses_and_their_rectangles(request, probe):
    if _delegated(request):
        return
    cols, rows, K, tiles = SIZES[160]
    rng = np.random.default_rng(11)
    bodies = [_cloud(rng, 65), _cloud(rng, 9, 0.02)]
    angles = [0.0, 1e-9, np.pi, np.pi - 1e-9, np.pi - 1e-3, 0.3, 1.0, 2.5, 1e-5]
    n = 2 * len(angles) + 1
    d = np.zeros((n + 1, 2, 6))
    d[:, :, 0:3] = rng.normal(0, 0.02, (n + 1, 2, 3))
    for i in range(n):
        for b in range(2):
            axis = rng.normal(size=3)
            d[i, b, 3:6] = axis / np.linalg.norm(axis) * angles[(i + b) % len(angles)]
    d[n, :, 0:3] = [(0.02, -0.01, 0.6), (-0.06, 0.03, 0.5)]                     # the default poses
    d[n, 0, 3:6], d[n, 1, 3:6] = (0.4, -0.2, 1.1), (0.0, 0.0, 0.0)
    d[n - 1, :, 3:6] = 0.0                                                        # no rotation at all
    idx = rng.integers(0, 4, n).astype(np.int32)
    a = _run(probe, 160, bodies, d, idx, route=ROUTE_DELTAS, windowed=0, groups=True)
    got = a.poses[:n * 24].reshape(n, 2, 12)
    worst = 0.0
    for i in range(n):
        for b in range(2):
            want = tw.compose_ld(d[i, b], d[n, b])
            assert np.array_equal(got[i, b, 9:], want[9:].astype(np.float64)), (i, b)           # one addition: exact
            diff = float(np.abs(got[i, b, :9].astype(tw.LD) - want[:9]).max())
            worst = max(worst, diff)
            assert diff <= POSE_TOL, (i, b, diff)
    figures["pose"] = max(figures["pose"], worst)
    print(f"\ncomposed poses: rotation entries within {worst:.3e} of the long-double composition (bar {POSE_TOL:.3e})")
    _check_tails(a, groups=True, regions=False)
    # the rectangle bars on the poses as read back; every other output as the device-array route gives it for those poses
    one = _run(probe, 160, bodies, got, idx, windowed=0)
    _check_rects(one, bodies, got, K, cols, rows, 4)
    b = _run(probe, 160, bodies, got, idx, windowed=0, groups=True)
    _same_outputs(a, b)
    assert np.array_equal(one.rects, b.rects)


# ---------------------------------------------------------------- groups
def _flat_body(K, w, h, z, rng, nv=12):
    """A planar cloud at depth z whose projection under the identity pose fills [cx + 0.5, cx + 0.5 + w] x [cy + 0.5, cy + 0.5 + h]."""
    a = np.concatenate([[[0, 0], [w, 0], [0, h], [w, h]], rng.uniform(0, 1, (nv - 4, 2)) * (w, h)])
    return np.stack([(a[:, 0] + 0.5) / K[0] * z, (a[:, 1] + 0.5) / K[1] * z, np.full(nv, z)], axis=1).astype(np.float32)


def _shift(K, z, du, dv):
    """The translation that puts such a body's corner at pixel (du + 0.5, dv + 0.5)."""
    return _pose(((du - K[2]) / K[0] * z, (dv - K[3]) / K[1] * z, 0.0))


def _group_scene(size, B, rng):
    """-> bodies, names, poses [cases][B][12]: the arrangements of the issue's list for B bodies."""
    cols, rows, K, _ = SIZES[size]
    s = cols // 64                                   # 64x48: 1, 160x120: 2
    dims = [(6 * s, 20 * s), (18 * s, 5 * s), (4 * s, 4 * s)] + [(4 * s, 3 * s)] * (B - 3)
    dims = dims[:B]
    z = 0.6
    bodies = [_flat_body(K, w, h, z, rng) for w, h in dims]
    OFF = (-3 * cols, -3 * rows)
    cases = {}
    # a place of its own for every body: the tall one, the wide one and the small one along the top, the rest in three rows below
    grid = [(2 * s, 2 * s), (12 * s, 2 * s), (36 * s, 2 * s)] + [(12 * s + 8 * s * (k % 6), 26 * s + 6 * s * (k // 6)) for k in range(13)]
    cases["apart"] = grid[:B]
    cases["all overlapping"] = [(20 * s, 10 * s)] * B
    cases["all off-screen"] = [OFF] * B
    cases["one off-screen"] = [OFF] + grid[1:B]
    cases["two apart, the rest off"] = [grid[0], grid[1]] + [OFF] * (B - 2)
    x1 = 8 * s + 6 * s + 2                           # body 0 at du = 8 s: its rectangle ends at align_up(du + w + 2)
    x1 = -(-x1 // 4) * 4
    cases["abut in x"] = [(8 * s, 4 * s), (x1, 4 * s)] + [OFF] * (B - 2)          # body 1 starts in the column body 0's rectangle ends at
    cases["abut in y"] = [(8 * s, 2 * s), (8 * s, 2 * s + 20 * s + 2)] + [OFF] * (B - 2)
    if B >= 3:
        cases["chain"] = [(8 * s, 4 * s), (12 * s, 22 * s), (28 * s, 25 * s)] + [OFF] * (B - 3)
        # body 0 (tall) and body 1 (wide) meet at the lower left; their box reaches over body 2, which touches neither
        cases["swallow"] = [(8 * s, 4 * s), (12 * s, 21 * s), (24 * s, 6 * s)] + [grid[15]] * (B - 3)
        cases["three apart"] = grid[:3] + [OFF] * (B - 3)
    if B >= 5:
        cases["four apart, the rest on the first"] = grid[:4] + [grid[0]] * (B - 4)
        cases["five apart"] = grid[:5] + [OFF] * (B - 5)
    names = sorted(cases)
    poses = np.array([[_shift(K, z, du, dv) for du, dv in cases[k]] for k in names])
    return bodies, names, poses


def _body_rects(probe, size, bodies, poses, **kw):
    """The kernel's own per-body rectangles: the probe on each body alone (the same arithmetic) -> [cases][B][4]."""
    return np.stack([_run(probe, size, [body], poses[:, b:b + 1], **kw).rects[:len(poses)] for b, body in enumerate(bodies)], axis=1)


@pytest.mark.parametrize("B", [2, 3, 5, 6, 16])
@pytest.mark.parametrize("size", [64, 160])
def test_groups_are_the_finest_partition_of_the_body_rectangles(request, probe, size, B):
    if _delegated(request):
        return
    cols, rows, K, tiles = SIZES[size]
    rng = np.random.default_rng([size, B])
    bodies, names, poses = _group_scene(size, B, rng)
    per_body = _body_rects(probe, size, bodies, poses, windowed=0)
    res = _run(probe, size, bodies, poses, windowed=0, groups=True)
    seen = set()
    for i, name in enumerate(names):
        br = [tuple(int(k) for k in r) for r in per_body[i]]
        dev = res.group_list(i)
        cnt = int(res.item_range[i][1])
        bad = tw.check_groups(dev, br, *tiles, cnt)
        assert not bad, (name, bad)
        assert tuple(int(k) for k in res.rects[i]) == tw.union_rect({(r, m) for r, m, _ in dev}), name
        g = res.groups[i]
        assert untouched(g[1:4]) and untouched(g[4 + 4 * len(dev):4 + 4 * tw.MAX_GROUPS]), name               # what lies beyond n is left alone
        seen.add((name, len(dev), len(tw.partition(br))))
        # the cases are what their names say
        live = [r for r in br if r[2] > r[0]]
        if name == "abut in x":
            assert br[0][2] == br[1][0] and len(dev) == 2, br
        if name == "abut in y":
            assert br[0][3] == br[1][1] and br[0][0] == br[1][0] and len(dev) == 2, br
        if name == "chain":
            assert tw.overlap(br[0], br[1]) and tw.overlap(br[1], br[2]) and not tw.overlap(br[0], br[2]) and len(dev) == 1
        if name == "swallow":
            assert not tw.overlap(br[2], br[0]) and not tw.overlap(br[2], br[1]) and tw.overlap(br[2], tw.union(br[0], br[1]))
            assert len(dev) == (1 if B == 3 else 2)
        if name == "all off-screen":
            assert not live and dev == [] and cnt == 1 and tuple(res.rects[i]) == (0, 0, 0, 0)
        if name == "one off-screen":
            assert not any(m & 1 for _, m, _ in dev)
        if name in ("five apart", "apart") and B >= 5:
            assert len(tw.partition(br)) >= 5 and len(dev) == 1 and dev[0][1] == sum(1 << b for b, r in enumerate(br) if r[2] > r[0])
        if name == "apart" and B <= 4:
            assert len(dev) == B
    _check_items(res, tiles, groups=True)
    _check_tails(res, groups=True, regions=False)


# ---------------------------------------------------------------- items
@pytest.mark.parametrize("n", [1, 7, 8, 9, 64, 65, 257])
def test_items_tile_the_counter_for_any_number_of_blocks(request, probe, n):
    if _delegated(request):
        return
    for size, groups in ((64, False), (160, True), (640, False)):
        cols, rows, K, tiles = SIZES[size]
        rng = np.random.default_rng([n, size])
        if groups:
            bodies, names, battery = _group_scene(size, 5, rng)
        else:
            bodies = [_cloud(rng, 65, 0.12)]
            battery = np.array([p for _, p in _battery(cols, rows, K, bodies[0], rng)])[:, None, :]
        poses = battery[rng.integers(0, len(battery), n)]
        idx = rng.integers(-1, 5, n).astype(np.int32)              # -1 and `slots` (4) included
        res = _run(probe, size, bodies, poses, idx, windowed=0, groups=groups, slots=4, win_src=np.zeros((4, 4), np.int32))
        _check_items(res, tiles, groups)
        _check_tails(res, groups=groups, regions=False)
        assert np.array_equal(res.parents[:n], idx)
        assert int(res.ctr_this[0]) == sum(int(c) for c in res.item_range[:n, 1])
        assert size != 640 or max(int(c) for c in res.item_range[:n, 1]) > 1 or n < 7      # full-frame rectangles split into several tiles


# ---------------------------------------------------------------- regions
def _region_inputs(size, rng):
    cols, rows, K, tiles = SIZES[size]
    body = _cloud(rng, 33)
    base = _pose(_at(K, cols * 0.45, rows * 0.5, 0.6), _rot(rng))
    off = _pose(_at(K, -cols, rows * 0.5, 0.6))
    s = cols // 16
    win = np.array([[cols, rows, 0, 0],                                     # empty
                    [7 * s, 7 * s // 2 + 4, 7 * s + 4, 7 * s // 2 + 6],                   # inside the rectangle
                    [4 * s, 2 * s, 8 * s, 6 * s],                                 # overlapping
                    [12 * s, 9 * s, 15 * s, 11 * s],                              # disjoint
                    [0, 0, cols, rows]], dtype=np.int32)                    # the whole frame
    idx = np.array([0, 1, 2, 3, 4, -1, 5, 3, 0, 2, 1], dtype=np.int32)       # -1 and `slots`: bad parents
    poses = np.array([base] * 8 + [off] * 3)[:, None, :]
    return body, poses, idx, win


def _check_regions(res, idx, win, rebase, slab_px, err0=(0, 0)):
    cols, rows = res.cols_, res.rows_
    worst, over, area8 = err0[1], False, 0
    for i in range(res.n):
        want = tw.region(tuple(res.rects[i]), int(idx[i]), win, len(win), rebase, cols, rows, slab_px)
        got = dict(win_used=res.win_used[i], win_dst=res.win_dst[i], reg_dst=res.reg_dst[i])
        bad = tw.check_region(got, want)
        assert not bad, (i, bad)
        assert int(res.parents[i]) == want["parent"], i
        worst, over = max(worst, want["area"]), over or want["overflow"]
        area8 += tw.area(want["win_used"]) if i % 8 == 0 else 0
    if slab_px:
        assert tuple(res.err[:2]) == (1 if over or err0[0] else 0, worst), res.err[:2]
    else:
        assert tuple(res.err[:2]) == tuple(err0) and untouched(res.reg_dst)
    if res.area_sum is not None:
        assert int(res.area_sum[0]) == area8
    return over


@pytest.mark.parametrize("size", [64, 160])
def test_regions_windows_and_slab_containment(request, probe, size):
    if _delegated(request):
        return
    cols, rows, K, tiles = SIZES[size]
    rng = np.random.default_rng(size + 1)
    body, poses, idx, win = _region_inputs(size, rng)
    kw = dict(slots=len(win), win_src=win, area=True)
    a = _run(probe, size, [body], poses, idx, **kw)
    assert not _check_regions(a, idx, win, None, 0)
    assert tuple(a.rects[0]) != (0, 0, 0, 0) and tuple(a.rects[8]) == (0, 0, 0, 0)
    _check_items(a, tiles)
    _check_tails(a)
    box = (cols - 12, 2, cols - 4, 9)
    b = _run(probe, size, [body], poses, idx, rebase_box=box, **kw)
    _check_regions(b, idx, win, box, 0)
    assert not np.array_equal(a.win_used, b.win_used) and np.array_equal(a.win_dst, b.win_dst)
    # a read-only call leaves the regions (and the area sum) alone
    c = _run(probe, size, [body], poses, idx, update=0, **kw)
    assert untouched(c.win_used) and untouched(c.win_dst) and untouched(c.reg_dst) and int(c.area_sum[0]) == 0 and (c.err[:2] == 0).all()
    _same_outputs(a, c, skip=("win_used", "win_dst", "reg_dst"))
    # slabs: the largest region but the whole frame's fits exactly / misses by one pixel / nothing but the empty regions fits
    areas = sorted({tw.region(tuple(a.rects[i]), int(idx[i]), win, len(win), None, cols, rows, 0)["area"] for i in range(a.n)})
    assert areas[0] == 0 and areas[-1] == cols * rows and len(areas) >= 4
    for slab, n_over in ((cols * rows, 0), (areas[-2], 1), (areas[-2] - 1, None), (16, None)):
        d = _run(probe, size, [body], poses, idx, slab_px=slab, err0=(0, 7), **kw)
        over = _check_regions(d, idx, win, None, slab, err0=(0, 7))
        assert over == (n_over != 0)
        assert np.array_equal(d.rects, a.rects) and np.array_equal(d.item_range[:, 1], a.item_range[:, 1])
        _check_items(d, tiles)
        contained = [i for i in range(d.n) if int(d.parents[i]) == -1 and int(idx[i]) != -1]
        assert n_over is None or len(contained) == n_over
        if slab == 16:
            assert len(contained) == 8       # every particle with a rectangle
    # a flag raised earlier stays raised, a larger area recorded earlier stays
    d = _run(probe, size, [body], poses, idx, slab_px=cols * rows, err0=(1, 1 << 30), **kw)
    assert tuple(d.err[:2]) == (1, 1 << 30)


# ---------------------------------------------------------------- strips
@pytest.mark.parametrize("B", [2, 3, 5])
@pytest.mark.parametrize("size", [64, 160])
def test_strips_paint_the_region_minus_the_groups(request, probe, size, B):
    if _delegated(request):
        return
    cols, rows, K, tiles = SIZES[size]
    rng = np.random.default_rng([size, B, 3])
    bodies, names, poses = _group_scene(size, B, rng)
    n = len(names)
    first = _run(probe, size, bodies, poses, windowed=0, groups=True)                 # the groups, to build parent windows from
    g0 = [first.group_list(i)[0][0] if first.group_list(i) else (cols, rows, 0, 0) for i in range(n)]
    s = cols // 16
    windows = {"empty": [(cols, rows, 0, 0)] * n, "frame": [(0, 0, cols, rows)] * n, "a group's own": g0,
               "staggered": [(4 * ((3 * i) % 5), (5 * i) % 7, cols - 4 * (i % 3), rows - (i % 4)) for i in range(n)],
               "inside": [(6 * s, 3 * s, 6 * s + 8, 3 * s + 3)] * n}
    counts = set()
    for wname, wl in windows.items():
        win = np.array(wl, dtype=np.int32)
        idx = np.arange(n, dtype=np.int32)
        for slab in (0, cols * rows, 64):
            res = _run(probe, size, bodies, poses, idx, groups=True, strips=True, slots=n, win_src=win, slab_px=slab)
            assert np.array_equal(res.groups, first.groups) and np.array_equal(res.rects, first.rects)
            _check_regions(res, idx, win, None, slab)
            for i, name in enumerate(names):
                dev = res.group_list(i)
                ns, sfirst, box = res.strip_list(i)
                u = tuple(int(k) for k in res.win_used[i])
                bad = tw.check_strips(ns, sfirst, box, u, [r for r, _, _ in dev], cols, rows)
                assert not bad, (wname, slab, name, bad)
                raw = res.strips[i]
                assert untouched(raw[1:4]) and untouched(raw[4 + ns + 1:4 + tw.MAX_STRIPS + 1]) and untouched(raw[4 + tw.MAX_STRIPS + 1 + 2 * ns:]), (wname, name)
                if u[2] <= u[0]:
                    assert ns == 0          # an empty region (nothing on screen and no parent window, or a slab that overflowed)
                counts.add((len(dev), ns > 0))
            _check_tails(res, groups=True, strips=True)
            _check_items(res, tiles, groups=True)
    assert {k for k, _ in counts} >= set(range(0, min(B, 4) + 1)), counts


def test_strips_are_written_by_updating_windowed_calls_only(request, probe):
    if _delegated(request):
        return
    rng = np.random.default_rng(8)
    bodies, names, poses = _group_scene(64, 3, rng)
    for kw in (dict(update=0), dict(windowed=0)):
        res = _run(probe, 64, bodies, poses, groups=True, strips=True, slots=1, win_src=np.array([[0, 0, 64, 48]], np.int32), **kw)
        assert untouched(res.strips) and untouched(res.win_used)


# ---------------------------------------------------------------- the frame launch
@pytest.mark.parametrize("rows,cols", [(16, 32), (48, 64)])
def test_frame_launch_gives_the_plain_launch_and_the_frame_terms(request, probe, rows, cols):
    """rbs_frame_prep_kernel: 16 x 32 pixels are one block of per-pixel terms behind the particles' blocks, 48 x 64 are six."""
    if _delegated(request):
        return
    import pixel_probes
    K = (56.0, 56.0, cols / 2 - 0.5, rows / 2 - 0.5)
    rng = np.random.default_rng(rows)
    bodies, _, scene = _group_scene(64, 3, rng)
    poses = scene[rng.integers(0, len(scene), 19)]
    idx = rng.integers(-1, 3, 19).astype(np.int32)
    win = np.array([[4, 2, 20, 9], [cols, rows, 0, 0]], dtype=np.int32)
    frame = rng.uniform(0.3, 3.0, rows * cols).astype(np.float32)
    frame[rng.random(frame.size) < 0.1] = np.nan
    frame[5] = np.inf
    frame[6] = 0.0
    model = (0.01, 0.003, 0.0014, np.log(2.0))
    kw = dict(rect_align=4, tile_w=32, tile_h=8, tile_px=8192, groups=True, strips=True, slots=2, win_src=win, model=model, area=True)
    plain = probe.run(rows, cols, K, bodies, poses, idx, **kw)
    for want_aux, want_keep in ((True, True), (True, False), (False, True)):
        fr = probe.run(rows, cols, K, bodies, poses, idx, frame=frame, want_aux=want_aux, want_keep=want_keep, **kw)
        _same_outputs(plain, fr)
        assert int(fr.area_sum[0]) == int(plain.area_sum[0])
        if want_aux:
            terms = pixel_probes.Probes(HOOKS).frame_terms(frame, *model)
            assert np.array_equal(fr.aux[:rows * cols].view(np.uint64), terms.view(np.uint64)) and untouched(fr.aux[rows * cols:])
        if want_keep:
            assert np.array_equal(fr.keep[:rows * cols].view(np.uint32), frame.view(np.uint32)) and untouched(fr.keep[rows * cols:])


def test_probe_refuses_what_it_cannot_run(request, probe):
    if _delegated(request):
        return
    rng = np.random.default_rng(0)
    body, pose = _cloud(rng, 5), _pose((0, 0, 0.6))[None, None, :]
    K = SIZES[64][2]
    for kw in (dict(rect_align=3), dict(rect_align=2), dict(tile_w=24), dict(tile_h=0), dict(tile_px=0), dict(route=3), dict(strips=True),
               dict(frame=np.ones(64 * 48, np.float32), route=ROUTE_HOST)):
        res = probe.run(48, 64, K, [body], pose, expect=pp.RBS_ERR_INVALID_ARGUMENT, **kw)
        assert untouched(res.rects) and untouched(res.item_particle)
    probe.run(48, 62, K, [body], pose, expect=pp.RBS_ERR_INVALID_ARGUMENT)
    assert probe.tiles_ub(64, 48, 8, 4, 64) == -1
