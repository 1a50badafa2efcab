"""The reference of the rectangles kernel (tests/prep_twin.py) and its checkers, on the CPU: every checker
tests/test_gpu_prep_kernels.py applies to the device's outputs accepts the twin's own outputs and rejects a planted mistake, and
the twin's tile_grid holds its three promises for every rectangle of four frame sizes."""
import numpy as np
import pytest

import prep_twin as tw

K160 = (140.0, 140.0, 79.5, 59.5)


def _cloud(rng, n, radius=0.05):
    return (rng.normal(size=(n, 3)) * radius / 2).clip(-radius, radius).astype(np.float32)


def _pose(t, R=None):
    return np.concatenate([(np.eye(3) if R is None else R).ravel(), np.asarray(t, dtype=np.float64)])


def _twin_rect(e, K, cols, rows, align):
    """A rectangle the bars accept: the exact projection's pixels grown by the stated margin."""
    mx, my = tw.margin(e, K)
    x0 = tw._clamp(np.floor(e["umin"] - tw.LD(mx)), cols) // align * align
    x1 = min(cols, -(-tw._clamp(np.ceil(e["umax"] + tw.LD(mx)) + 1, cols) // align) * align)
    y0, y1 = tw._clamp(np.floor(e["vmin"] - tw.LD(my)), rows), tw._clamp(np.ceil(e["vmax"] + tw.LD(my)) + 1, rows)
    return (x0, y0, x1, y1) if x1 > x0 and y1 > y0 else (0, 0, 0, 0)


# ---------------------------------------------------------------- rectangles
@pytest.mark.parametrize("t", [(0.0, 0.0, 0.6), (-0.33, 0.1, 0.6), (0.3, -0.24, 0.6), (0.02, 0.01, 0.08), (0.9, 0.0, 0.6), (0.0, 0.0, 3.0)])
@pytest.mark.parametrize("align", [4, 8, 16])
def test_rect_checker_accepts_the_twin_and_rejects_a_short_rectangle(t, align):
    rng = np.random.default_rng(1)
    body = _cloud(rng, 65)
    e = tw.extents([body], [_pose(t)], K160)
    r = _twin_rect(e, K160, 160, 120, align)
    assert tw.check_rect(r, e, K160, 160, 120, align) == []
    if r[2] > r[0]:
        # one column (one aligned step) short on either side, one row short above and below: rejected wherever the exact
        # projection reaches into what was cut off
        inner, _ = tw.rect_bars(e, K160, 160, 120, align)
        for k, d in ((0, align), (2, -align), (1, 1), (3, -1)):
            s = list(r)
            s[k] += d
            cut = inner is not None and (s[0] > inner[0] or s[1] > inner[1] or s[2] < inner[2] or s[3] < inner[3])
            assert bool(tw.check_rect(tuple(s), e, K160, 160, 120, align)) == cut, (r, s, inner)
        s = list(r)
        s[0], s[2] = inner[0] + 1 if inner else s[0], s[2]
        if inner and inner[0] + 1 < s[2]:
            assert tw.check_rect(tuple(s), e, K160, 160, 120, 1), "one column short"
        # far too wide: rejected by the tightness bar (unless the frame ends first)
        wide = (max(0, r[0] - 4 * align), r[1], r[2], r[3])
        _, outer = tw.rect_bars(e, K160, 160, 120, align)
        assert bool(tw.check_rect(wide, e, K160, 160, 120, align)) == (wide[0] < outer[0])
    else:
        assert tw.check_rect((0, 0, 160, 120), e, K160, 160, 120, align), "off screen, yet the whole frame"


def test_rect_checker_on_the_camera_plane_and_broken_poses():
    rng = np.random.default_rng(2)
    body = _cloud(rng, 64)
    zlo = float(body[:, 2].min())
    for zmin, full_needed, full_allowed in ((0.5e-4, True, True), (1.0e-4 * (1 - 1e-9), True, True), (1.005e-4, False, True), (1.02e-4, False, False),
                                            (-0.01, True, True)):
        e = tw.extents([body], [_pose((0.0, 0.0, zmin - zlo))], K160)
        assert abs(float(e["zmin"]) - zmin) < 1e-9
        assert (tw.check_rect((0, 0, 160, 120), e, K160, 160, 120, 4) == []) == full_allowed or tw.rect_bars(e, K160, 160, 120, 4)[1] == (0, 0, 160, 120)
        assert bool(tw.check_rect((16, 8, 64, 48), e, K160, 160, 120, 4)) or not full_needed
    for k, bad in ((0, np.nan), (4, np.inf), (9, np.nan), (10, -np.inf), (11, np.nan)):
        p = _pose((0.0, 0.0, 0.6))
        p[k] = bad
        e = tw.extents([body], [p], K160)
        assert tw.check_rect((0, 0, 160, 120), e, K160, 160, 120, 4) == []
        assert tw.check_rect((0, 0, 0, 0), e, K160, 160, 120, 4) and tw.check_rect((64, 40, 96, 80), e, K160, 160, 120, 4)
    assert tw.check_rect((0, 0, 0, 8), tw.extents([body], [_pose((9.0, 0.0, 0.6))], K160), K160, 160, 120, 4)   # empty is (0, 0, 0, 0)


def test_composition_is_a_rotation_and_adds_translations():
    rng = np.random.default_rng(3)
    for angle in (0.0, 1e-9, 0.3, np.pi - 1e-3, np.pi - 1e-9, np.pi):
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        d = np.concatenate([rng.normal(size=3), axis * angle])
        d0 = np.concatenate([rng.normal(size=3), rng.normal(size=3)])
        q = tw.compose_ld(d, d0)
        R = q[:9].reshape(3, 3)
        assert float(np.abs(R @ R.T - np.eye(3)).max()) < 1e-17 and abs(float(np.linalg.det(R.astype(np.float64))) - 1) < 1e-12
        assert np.array_equal(q[9:].astype(np.float64), d[:3] + d0[:3])
        Rd = tw.rotvec_matrix_ld(d[3:])
        assert abs(float(np.trace(Rd)) - (1 + 2 * np.cos(angle))) < 1e-15
        if angle > 1e-6:
            assert float(np.abs(Rd @ axis - axis).max()) < 1e-15      # (the axis is a unit vector to binary64 only)


# ---------------------------------------------------------------- groups
APART = [(0, 0, 16, 10), (32, 0, 48, 10), (64, 20, 80, 30), (100, 50, 120, 60)]
CHAIN = [(0, 0, 20, 20), (16, 10, 40, 30), (36, 20, 60, 40)]                      # A^B, B^C overlap, A^C do not
SWALLOW = [(0, 0, 20, 40), (16, 30, 60, 44), (40, 4, 52, 12), (100, 100, 104, 104)]  # A + B grows over C
ABUT = [(0, 0, 16, 10), (16, 0, 32, 10), (0, 10, 16, 20)]


def test_partition_is_the_finest_and_order_free():
    assert tw.groups(APART) == {(r, 1 << b) for b, r in enumerate(APART)}
    assert tw.groups(CHAIN) == {((0, 0, 60, 40), 7)}
    assert tw.groups(SWALLOW) == {((0, 0, 60, 44), 7), ((100, 100, 104, 104), 8)}
    assert tw.groups(ABUT) == {(r, 1 << b) for b, r in enumerate(ABUT)}
    assert tw.groups([(0, 0, 0, 0), (4, 4, 8, 8)]) == {((4, 4, 8, 8), 2)}
    assert tw.groups([(0, 0, 0, 0)] * 3) == set()
    five = APART + [(140, 100, 156, 110)]
    assert tw.groups(five) == {((0, 0, 156, 110), 31)}
    rng = np.random.default_rng(4)
    for _ in range(200):     # any order of the bodies: the same partition (masks permuted back)
        nb = int(rng.integers(2, 9))
        x0, y0 = rng.integers(0, 100, nb) // 4 * 4, rng.integers(0, 90, nb)
        rects = [(int(a), int(b), int(a + 4 * rng.integers(1, 12)), int(b + rng.integers(1, 30))) for a, b in zip(x0, y0)]
        perm = rng.permutation(nb)
        got = tw.partition([rects[k] for k in perm])
        back = {(r, sum(1 << int(perm[j]) for j in range(nb) if m >> j & 1)) for r, m in got}
        assert back == tw.partition(rects)
        lst = list(got)
        assert not any(tw.overlap(lst[i][0], lst[j][0]) for i in range(len(lst)) for j in range(i))


def _stored(group_set, tiles):
    out, at = [], 0
    for r, m in sorted(group_set):
        out.append((r, m, at))
        at += tw.tile_count(r, *tiles)
    return out, max(at, 1)


def test_group_checker_rejects_planted_mistakes():
    tiles = (32, 8, 256)
    for rects in (APART, CHAIN, SWALLOW, ABUT, APART + [(140, 100, 156, 110)], [(0, 0, 0, 0)] * 2):
        dev, cnt = _stored(tw.groups(rects), tiles)
        assert tw.check_groups(dev, rects, *tiles, cnt) == []
    # two overlapping groups left unmerged
    dev = [(CHAIN[0], 1, 0), (tw.union(CHAIN[1], CHAIN[2]), 6, tw.tile_count(CHAIN[0], *tiles))]
    cnt = dev[1][2] + tw.tile_count(dev[1][0], *tiles)
    assert any("overlap" in b for b in tw.check_groups(dev, CHAIN, *tiles, cnt))
    # abutting groups merged
    dev, cnt = _stored({(tw.union(ABUT[0], ABUT[1]), 3), (ABUT[2], 4)}, tiles)
    assert tw.check_groups(dev, ABUT, *tiles, cnt)
    # `first` off by one tile; a count that does not end where the spans end
    dev, cnt = _stored(tw.groups(APART), tiles)
    off = [dev[0], (dev[1][0], dev[1][1], dev[1][2] + 1)] + dev[2:]
    assert any("starts at item" in b for b in tw.check_groups(off, APART, *tiles, cnt))
    assert tw.check_groups(dev, APART, *tiles, cnt + 1)
    # a mask that lost a body
    dev, cnt = _stored(tw.groups(CHAIN), tiles)
    assert tw.check_groups([(dev[0][0], 5, 0)], CHAIN, *tiles, cnt)


# ---------------------------------------------------------------- items
def test_item_checker_rejects_planted_mistakes():
    counts = [1, 3, 2, 1, 4]
    first = [4, 0, 9, 3, 5]                       # any free range will do
    rng_ = np.array(list(zip(first, counts)), dtype=np.int32)
    owner = np.full(11 + 5, -7, dtype=np.int32)
    for i, (f, c) in enumerate(zip(first, counts)):
        owner[f:f + c] = i
    assert tw.check_items(rng_, owner, 11, counts, 4) == []
    bad = rng_.copy()
    bad[2][0] = 8                                 # overlaps its neighbour (and leaves an item to nobody)
    assert any("overlaps" in b for b in tw.check_items(bad, owner, 11, counts, 4))
    assert any("nobody" in b for b in tw.check_items(rng_, owner, 12, counts, 4))
    wrong = owner.copy()
    wrong[1] = 4
    assert any("item_particle" in b for b in tw.check_items(rng_, wrong, 11, counts, 4))
    assert any("bound" in b for b in tw.check_items(rng_, owner, 11, counts, 3))
    assert any("the twin has" in b for b in tw.check_items(rng_, owner, 11, [1, 3, 2, 1, 3], 4))


# ---------------------------------------------------------------- regions
def test_region_rules_and_their_checker():
    cols, rows = 160, 120
    win = np.array([[cols, rows, 0, 0], [40, 30, 60, 50], [20, 20, 100, 90], [120, 100, 140, 110]], dtype=np.int32)
    rect = (32, 24, 72, 64)
    want = {0: rect, 1: rect, 2: (20, 20, 100, 90), 3: (32, 24, 140, 110), -1: rect, 4: rect}
    for parent, u in want.items():
        g = tw.region(rect, parent, win, 4, None, cols, rows, 0)
        assert g["win_used"] == u and g["win_dst"] == rect and g["reg_dst"] is None and g["parent"] == parent and not g["overflow"]
        assert tw.check_region(dict(win_used=u, win_dst=rect, reg_dst=(1, 2, 3, 4)), g) == []
    g = tw.region(rect, 3, win, 4, None, cols, rows, 0)
    assert any("win_used" in b for b in tw.check_region(dict(win_used=rect, win_dst=rect, reg_dst=rect), g))     # the parent's window not united
    g = tw.region((0, 0, 0, 0), 0, win, 4, None, cols, rows, 0)
    assert g["win_used"] == g["win_dst"] == tw.empty(cols, rows) and g["area"] == 0
    g = tw.region((0, 0, 0, 0), 1, win, 4, (0, 0, 8, 4), cols, rows, 0)
    assert g["win_used"] == (0, 0, 60, 50) and g["win_dst"] == tw.empty(cols, rows)
    fit = tw.area((32, 24, 140, 110))
    for slab, over in ((fit, False), (fit - 1, True), (16, True)):
        g = tw.region(rect, 3, win, 4, None, cols, rows, slab)
        assert g["overflow"] == over and g["area"] == fit
        assert g["reg_dst"] == g["win_used"] == (tw.empty(cols, rows) if over else (32, 24, 140, 110))
        assert g["parent"] == (-1 if over else 3) and g["win_dst"] == (tw.empty(cols, rows) if over else rect)
        assert any("reg_dst" in b for b in tw.check_region(dict(win_used=g["win_used"], win_dst=g["win_dst"], reg_dst=rect), g))


# ---------------------------------------------------------------- strips
STRIP_CASES = {
    "one": ((8, 4, 120, 100), [(32, 24, 72, 64)]),
    "side by side": ((0, 10, 160, 60), [(8, 20, 40, 50), (48, 20, 80, 50), (96, 20, 120, 50), (128, 20, 156, 50)]),
    "stacked": ((20, 0, 100, 120), [(40, 4, 80, 20), (40, 24, 80, 50), (40, 50, 80, 70), (36, 90, 84, 118)]),
    "staggered": ((0, 0, 160, 120), [(8, 8, 60, 50), (64, 30, 100, 80), (20, 60, 56, 110), (104, 4, 152, 28)]),
    "touching": ((16, 10, 120, 90), [(16, 10, 40, 30), (96, 10, 120, 40), (16, 70, 60, 90), (100, 60, 120, 90)]),
    "equal": ((32, 24, 72, 64), [(32, 24, 72, 64)]),
    "none": ((16, 10, 120, 90), []),
    "empty": ((160, 120, 0, 0), [(32, 24, 72, 64)]),
}


@pytest.mark.parametrize("name", sorted(STRIP_CASES))
def test_strip_checker_accepts_the_twin_and_rejects_planted_mistakes(name):
    u, rects = STRIP_CASES[name]
    n, first, box = tw.strips(u, rects)
    assert n <= tw.MAX_STRIPS and tw.check_strips(n, first, box, u, rects, 160, 120) == []
    assert int(first[n]) * 4 == int(tw.strip_mask(u, rects, 160, 120).sum())
    if n == 0:
        assert name in ("equal", "empty")
        return
    k = n // 2
    short = box.copy()
    short[k][1] -= 1                              # one float4 short
    f2 = first.copy()
    f2[k + 1:] -= short[k][3] - short[k][2]
    assert any("missing" in b for b in tw.check_strips(n, f2, short, u, rects, 160, 120)) or short[k][1] == short[k][0]
    assert any("running cell count" in b or "first[n]" in b for b in tw.check_strips(n, first, short, u, rects, 160, 120))
    off = first.copy()
    off[n] += 1
    assert tw.check_strips(n, off, box, u, rects, 160, 120)
    if rects:                                     # a strip that reaches one float4 into a group
        g = rects[0]
        over = box.copy()
        hit = [s for s in range(n) if 4 * box[s][1] == g[0] and box[s][2] >= g[1] and box[s][3] <= g[3]]
        if hit:
            over[hit[0]][1] += 1
            assert any("too many" in b for b in tw.check_strips(n, first, over, u, rects, 160, 120))
        twice = box.copy()
        twice[n - 1] = twice[0]
        assert tw.check_strips(n, first, twice, u, rects, 160, 120)


def test_a_strip_overlapping_a_group_is_rejected():
    u, rects = STRIP_CASES["one"]
    n, first, box = tw.strips(u, rects)
    hit = [s for s in range(n) if 4 * box[s][1] == rects[0][0]]
    assert hit
    box[hit[0]][1] += 1
    assert any("too many" in b for b in tw.check_strips(n, first, box, u, rects, 160, 120))


# ---------------------------------------------------------------- tile_grid, exhaustively
# (tile_w, tile_h, tile_px): the library's tiles -- 11 008 px with three raster blocks per CU, 16 384 with two, 9 536 and 14 912 where
# the binary64 likelihood's tables share the LDS -- at tile_w = 256 and full height, at the least height (4), and small tiles
TILES = [(256, px // 256, px) for px in (11008, 16384, 9536, 14912)] + [(256, 4, 11008), (16, 4, 8192), (32, 8, 8192)]


@pytest.mark.parametrize("cols,rows", [(64, 48), (160, 120), (640, 480), (1280, 960)])
def test_tile_grid_covers_caps_and_stays_within_the_bound(cols, rows):
    rh = np.arange(1, rows + 1)
    for tile_w, tile_h, tile_px in TILES:
        cap = tw.cap_px(tile_w, tile_h, tile_px)
        ub = tw.tiles_upper_bound(cols, rows, tile_w, cap)
        for rw in range(4, cols + 1, 4):
            # (vectorised over every height; the scalar function is compared on a few)
            nx = max(1, -(-rw // tile_w))
            t_w = max(16, (-(-rw // nx) + 15) // 16 * 16)
            hmax = max(1, cap // t_w)
            ny = np.maximum(1, -(-rh // hmax))
            th = np.maximum(1, -(-rh // ny))
            for h in (1, rows // 2, rows):
                assert tw.tile_grid(rw, h, tile_w, cap) == (t_w, int(th[h - 1]), nx, int(ny[h - 1]))
            assert t_w <= tile_w and t_w % 16 == 0
            assert nx * t_w >= rw and (ny * th >= rh).all(), (rw, tile_w, tile_h, tile_px)
            assert (t_w * th <= cap).all() or cap < 16, (rw, tile_w, tile_h, tile_px)
            assert int((nx * ny).max()) <= ub, (rw, tile_w, tile_h, tile_px, ub)
