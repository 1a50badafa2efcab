"""The shared planes kernel (dbot_ros_amd/csrc/rbs_pose_planes.h, rbs_planes_render_kernel) across its consumers ON THE DEVICE:
rbs_render_depth, the assessor's per-body planes, the Gaussian tracker's sigma renders and rbs_occlusion_bodies' owner rule,
on a model of two overlapping bodies (the assess scenes' meshes m1 and m2).

Two shapes (cols x rows), chosen on the CPU (test_the_chosen_poses_take_the_paths_they_are_chosen_for, which needs no device):
  small  100 x 76: the pose's rectangle is 100 x 71 pixels exactly -- wider and taller than a 64-pixel tile and no multiple of
         it, so it is cut into 2 x 2 tiles with a partial tile at the right and at the bottom -- and each body's own rectangle
         is cut into two tile columns, the right one partial;
  large  520 x 330: a pose that fills the view; each body's rectangle is cut into 48 tiles, more than the 32 blocks of a
         plane's row, so the strided walk over the tiles runs.
At both, two more poses move body 1 away: behind the camera (its rectangle is then the WHOLE frame -- bodies_rect's rule for a
vertex behind the camera plane -- and nothing is drawn into it) and off screen (its rectangle is empty).  Either way the body
contributes an all-+inf plane and a record with rendered == 0.

No tolerance anywhere: depths are compared bit for bit, counts are integers."""
import functools

import numpy as np
import pytest

import assess_scenes as asc
import gauss_twin as gt
import prep_twin as pt
from dbot_ros_amd import RbSensor, synth
from dbot_ros_amd.assess import PoseAssessor
from dbot_ros_amd.gaussian import GaussianTracker, GaussianTrackerBuilder

MESHES = ("m1", "m2")
# body 0 at (-a, dy, z), body 1 at (+a, dy, z): the two interpenetrate, each is the nearer one over part of the overlap
SHAPES = {"small": (100, 76, dict(z=0.105, a=0.004, dy=0.006)), "large": (520, 330, dict(z=0.08, a=0.015, dy=0.0))}
TILE_W, TILE_PX, SPLIT = 64, 4096, 32       # kPlaneTileW, kPlaneTilePx, kPlaneRenderSplit
ALIGN = 16                                  # the coarser of the two rectangle alignments: the outer bar holds for both
PARAMS = PoseAssessor.Parameters(**asc.PARAMS)


@functools.lru_cache(maxsize=None)
def case(shape):
    """(Scene, {name: pose [2, 12]}, frame): shared by the tests, read-only."""
    cols, rows, g = SHAPES[shape]
    s = asc.Scene(MESHES, cols, rows)
    main = s.truth.copy()
    main[0, 9:12] = (-g["a"], g["dy"], g["z"])
    main[1, 9:12] = (g["a"], g["dy"], g["z"])
    behind, off = main.copy(), main.copy()
    behind[1, 11] = -1.0
    off[1, 9] += 5.0
    frame = synth.make_frame(s.orc.render_depth(main), rows, cols, np.random.default_rng(5), occluder=False)
    return s, {"main": main, "behind": behind, "off": off}, np.asarray(frame, dtype=np.float32).ravel()


def extents(s, pose, bodies):
    """(extents, K) of the projection of `bodies` of `pose` (tests/prep_twin.py)."""
    K = s.cam.camera_matrix
    Kt = (K[0, 0], K[1, 1], K[0, 2], K[1, 2])
    return pt.extents([np.asarray(s.om.vertices[b], dtype=np.float32) for b in bodies], [pose[b] for b in bodies], Kt), Kt


def bars(s, pose, bodies):
    """(extents, K, inner, outer) of the rectangle of `bodies` of `pose`: the device's rectangle contains inner and lies
    inside outer."""
    e, Kt = extents(s, pose, bodies)
    return (e, Kt) + pt.rect_bars(e, Kt, s.cols, s.rows, ALIGN)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_the_chosen_poses_take_the_paths_they_are_chosen_for(shape):
    s, poses, _ = case(shape)
    main = poses["main"]
    pl = s.planes(main)
    both = np.isfinite(pl[0]) & np.isfinite(pl[1])
    near0, near1 = int((both & (pl[0] < pl[1])).sum()), int((both & (pl[1] < pl[0])).sum())
    print(shape, "covered by both", int(both.sum()), "body 0 nearer", near0, "body 1 nearer", near1)
    assert near0 > 500 and near1 > 500                      # the owner rule decides, both ways
    rects = [bars(s, main, [b])[2:] for b in (0, 1)]
    for inner, outer in rects:
        assert inner is not None and outer[2] > outer[0]
    (a, _), (b, _) = rects
    assert max(a[0], b[0]) < min(a[2], b[2]) and max(a[1], b[1]) < min(a[3], b[3])      # the rectangles overlap
    if shape == "small":
        _, _, inner, outer = bars(s, main, [0, 1])
        assert inner == outer == (0, 5, 100, 76)            # so the device's rectangle is this one
        w, h = outer[2] - outer[0], outer[3] - outer[1]
        tw, th, nx, ny = pt.tile_grid(w, h, TILE_W, TILE_PX)
        assert w > 64 and h > 64 and w % 64 and h % 64 and (nx, ny) == (2, 2) and w % tw and h % th
        for inner, outer in rects:                          # per body: several tiles, whichever bar the rectangle is nearer to
            for r in (inner, outer):
                tw, th, nx, ny = pt.tile_grid(r[2] - r[0], r[3] - r[1], TILE_W, TILE_PX)
                assert nx == 2 and ny in (1, 2)
            assert (inner[2] - inner[0]) % 64 and (outer[2] - outer[0]) % 64
    else:
        for inner, outer in rects:
            for r in (inner, outer):
                tw, th, nx, ny = pt.tile_grid(r[2] - r[0], r[3] - r[1], TILE_W, TILE_PX)
                assert nx * ny > SPLIT, (r, nx, ny)
    # body 1 moved away: behind the camera plane the rectangle is the whole frame, off screen it is empty; nothing is covered
    e, _ = extents(s, poses["behind"], [1])
    assert e["zmin"] < 0 and not np.isfinite(float(e["umin"]))         # no vertex in front of the camera
    e, Kt, inner, _ = bars(s, poses["off"], [1])
    assert inner is None and e["zmin"] > pt.Z_CLEAR and float(e["umin"]) - 2 * pt.margin(e, Kt)[0] >= s.cols
    for name in ("behind", "off"):
        assert not np.isfinite(s.planes(poses[name])[1]).any() and np.isfinite(s.planes(poses[name])[0]).any()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(SHAPES))
def test_one_render_kernel_behind_the_hook_the_assessor_the_gaussian_tracker_and_the_occlusion_summary(gpu_lib, shape):
    s, poses, frame = case(shape)
    npx = s.rows * s.cols
    with RbSensor(s.om, s.cam, s.P, max_particles=1) as sensor:
        gp = GaussianTrackerBuilder.Parameters()
        gp.object_transition.part_count = s.B
        tracker = GaussianTracker(sensor, s.om, gp)
        tracker.initialize([tracker._from_model(gt.truth_state(poses["main"]))])
        tracker.track(frame)
        q = tracker.sigma_poses()[0]                         # the pose as the tracker composed it: THE pose of every render below
        assert np.abs(q - poses["main"]).max() < 1e-12
        gauss = tracker.render(0)
        tracker.close()
        named = {"main": q, "behind": poses["behind"], "off": poses["off"]}
        a = PoseAssessor(sensor, PARAMS)
        res = a.assess(np.stack(list(named.values())), frame)
        planes = {n: np.stack([a.plane(k, b) for b in range(s.B)]) for k, n in enumerate(named)}
        hook = {n: sensor.render_depth(p) for n, p in named.items()}
        # one pose, three consumers, the same bits -- and they are the oracle's
        assert np.array_equal(bits(hook["main"]), bits(gauss))
        assert np.array_equal(bits(planes["main"].min(axis=0)), bits(hook["main"]))
        assert np.array_equal(bits(hook["main"]), bits(s.orc.render_depth(q)))
        assert np.isfinite(hook["main"]).sum() > 0.4 * npx
        for n, p in named.items():
            assert np.array_equal(bits(planes[n].min(axis=0)), bits(hook[n])), n
            for b in range(s.B):
                assert np.array_equal(bits(planes[n][b]), bits(s.planes(p)[b])), (n, b)
        # outside a body's rectangle its plane is +inf
        for b in range(s.B):
            x0, y0, x1, y1 = bars(s, q, [b])[3]
            outside = np.ones((s.rows, s.cols), dtype=bool)
            outside[y0:y1, x0:x1] = False
            assert np.isposinf(planes["main"][b].reshape(s.rows, s.cols)[outside]).all(), b
        # body 1 moved away: an all-+inf plane and rendered == 0; body 0 keeps its plane and owns all it covers
        for k, n in enumerate(named):
            print(shape, n, "counts", res.counts[k].tolist())
            if n == "main":
                assert (res.counts[k][:, 0] > 500).all()
                continue
            assert np.isposinf(planes[n][1]).all() and not res.counts[k][1].any(), n
            assert np.array_equal(bits(planes[n][0]), bits(planes["main"][0])), n
            assert res.counts[k][0, 0] == int(np.isfinite(planes[n][0]).sum()) > res.counts[0][0, 0], n
        owned = np.stack([[int((np.isfinite(planes[n][b]) & (planes[n][b] == planes[n].min(axis=0)) &
                                ((b == 0) | (planes[n][b] < planes[n][0]))).sum()) for b in range(s.B)] for n in named])
        assert np.array_equal(res.counts[:, :, 0], owned)    # the owner rule: nearest, a tie to the lower body
        # rbs_occlusion_bodies on an all-zero map: the assessor's owners, and its planes are what rbs_assess_get_plane hands out
        occ = sensor.occlusion_bodies(np.zeros(npx, dtype=np.float32), np.stack(list(named.values())[::-1]))
        assert np.array_equal(occ[::-1, :, 0], res.counts[:, :, 0]) and not occ[:, :, 1:].any()
        for k, n in enumerate(list(named)[::-1]):
            for b in range(s.B):
                assert np.array_equal(bits(a.plane(k, b)), bits(planes[n][b])), (n, b)
