"""Parity of the HIP path (through the C-ABI) against the CPU oracle on identical seeded inputs.

Bars (written here, as DESIGN.md states them):
  * coverage + rendered depth:            bit-exact (integer/compare work in binary64, one float rounding)
  * log-likelihood vs the EAGER oracle    |d| <= 1e-9 * max(1,|ll|)   (same rule, only libm-vs-ocml ulps)
    (the device's occlusion rule):
  * occlusion planes vs the EAGER oracle: <= 1 float ulp on <= 1e-4 of the pixels, rest bit-exact
  * log-likelihood vs the LAZY oracle     |d| <= 1e-5 * max(1,|ll|)   (north_star's tolerance)
    (reference CPU semantics):
"""
import numpy as np
import pytest

import oracle_binding as ob
import scenarios as sc
from dbot_ros_amd import RbSensor, RbSensorError, synth
from mesh_cases import mesh_variants

pytestmark = pytest.mark.gpu

TOL_EAGER = 1e-9
TOL_LAZY = 1e-5


@pytest.fixture(autouse=True, params=["window", "dense"])
def state_layout(request, monkeypatch):
    """Every parity test runs on both layouts of the occlusion state: windowed planes (default)
    and whole planes (RBS_STATE=dense).  The numbers must not depend on the layout."""
    monkeypatch.setenv("RBS_STATE", request.param)
    # the bars of this module are those of likelihood precision F64, the library's default (pinned
    # here all the same; the opt-in F32: tests/test_gpu_f32.py)
    monkeypatch.setenv("RBS_PRECISION", "f64")
    return request.param


def rel_err(a, b):
    return np.abs(a - b) / np.maximum(1.0, np.abs(b))


def assert_planes_match(g, o):
    """bit-exact except a vanishing fraction of 1-ulp float differences (posterior b/(a+b)
    rounded from doubles that differ in the last place between libm and ocml)."""
    diff = g != o
    # NaN never appears in an occlusion plane
    assert not np.isnan(g).any() and not np.isnan(o).any()
    frac = diff.mean()
    assert frac <= 1e-4, f"{diff.sum()} of {diff.size} occlusion values differ"
    if diff.any():
        ulp = np.abs(g[diff].view(np.int32).astype(np.int64) - o[diff].view(np.int32).astype(np.int64))
        assert ulp.max() <= 1, f"max ulp distance {ulp.max()}"


@pytest.mark.parametrize("mesh,cols,rows", [("m1", 640, 480), ("m3", 640, 480), ("m2", 640, 480),
                                             ("box12", 640, 480), ("m1", 80, 60), ("m3", 80, 60),
                                             ("m1_l2", 322, 241), ("m4", 1280, 960)])
def test_render_depth_bit_exact(gpu_lib, mesh, cols, rows):
    om, cam, P = sc.make_scene((mesh,), cols, rows, max_particles=2)
    o = ob.Oracle(om, cam, P, max_particles=2)
    with RbSensor(om, cam, P, max_particles=2) as g:
        rng = np.random.default_rng(5)
        for k in range(5):
            pose = synth.particle_poses(synth.truth_pose(1, z=0.5 + 0.15 * k, frame=3 * k), 1, rng,
                                        scale=4.0)[0]
            dg, do = g.render_depth(pose), o.render_depth(pose)
            assert np.isfinite(do).sum() > 0
            assert np.array_equal(dg.view(np.uint32), do.view(np.uint32)), \
                f"{(dg.view(np.uint32) != do.view(np.uint32)).sum()} depth pixels differ"


@pytest.mark.parametrize("pose_case", ["near_fills_image", "behind_camera", "off_screen",
                                       "straddles_image_edge", "crosses_camera_plane"])
def test_render_edge_poses(gpu_lib, pose_case):
    om, cam, P = sc.make_scene(("m1",), 640, 480, max_particles=2)
    o = ob.Oracle(om, cam, P, max_particles=2)
    pose = synth.truth_pose(1).copy()
    t = {"near_fills_image": (0.0, 0.0, 0.07), "behind_camera": (0.0, 0.0, -0.7),
         "off_screen": (2.0, 0.0, 0.7), "straddles_image_edge": (0.38, 0.27, 0.7),
         "crosses_camera_plane": (0.0, 0.0, 0.01)}[pose_case]
    pose[0, 9:12] = t
    with RbSensor(om, cam, P, max_particles=2) as g:
        dg, do = g.render_depth(pose), o.render_depth(pose)
    assert np.array_equal(dg.view(np.uint32), do.view(np.uint32))
    if pose_case in ("behind_camera", "off_screen"):
        assert not np.isfinite(do).any()
    if pose_case == "near_fills_image":
        assert np.isfinite(do).mean() > 0.5


@pytest.mark.parametrize("meshes,cols,rows,n", [(("m1",), 640, 480, 24), (("m3",), 640, 480, 16),
                                                 (("m1",), 80, 60, 64), (("box12",), 640, 480, 8),
                                                 (("m1", "m2", "m3"), 640, 480, 12),
                                                 (("m1_l2",), 322, 241, 16),
                                                 (("m4",), 1280, 960, 4),
                                                 # the rbs_raster_kernel_many_* instantiations (a body of > 256 clusters): with small
                                                 # bodies beside it, and a body of more clusters than one stretch of the shared cull
                                                 (("m1", "m4", "m2"), 640, 480, 6), (("m4_fine",), 640, 480, 3)])
def test_sequence_matches_oracle(gpu_lib, meshes, cols, rows, n):
    """set_observation -> loglikes(update) -> resample, 4 frames; eager and lazy oracles."""
    om, cam, P = sc.make_scene(meshes, cols, rows, max_particles=n)
    nb = len(meshes)
    eager = ob.Oracle(om, cam, P, max_particles=n, mode=ob.EAGER)
    lazy = ob.Oracle(om, cam, P, max_particles=n, mode=ob.LAZY)
    frames = sc.make_frames(eager, nb, 4, seed=3)
    with RbSensor(om, cam, P, max_particles=n) as g:
        ll_g = sc.run_sequence(g, frames, n, n_bodies=nb)
        ll_e = sc.run_sequence(eager, frames, n, n_bodies=nb)
        ll_l = sc.run_sequence(lazy, frames, n, n_bodies=nb)
        for k in range(len(frames)):
            assert np.isfinite(ll_g[k]).all()
            assert rel_err(ll_g[k], ll_e[k]).max() <= TOL_EAGER, (k, rel_err(ll_g[k], ll_e[k]).max())
            assert rel_err(ll_g[k], ll_l[k]).max() <= TOL_LAZY, (k, rel_err(ll_g[k], ll_l[k]).max())
        for slot in range(n):
            assert_planes_match(g.get_occlusion(slot), eager.get_occlusion(slot))
            # reference semantics: occlusion "as of now" of the lazy model
            assert np.abs(g.get_occlusion(slot) - lazy.get_occlusion(slot, now=True)).max() <= 2e-6


@pytest.mark.parametrize("meshes,cols,rows,n,precision", [(("m1", "m2", "m3"), 640, 480, 12, "f64"), (("m4",), 1280, 960, 4, "f64"),
                                                           (("m1_l2",), 322, 241, 16, "f32"), (("m1", "m4", "m2"), 640, 480, 6, "f32")])
def test_both_sets_of_raster_kernels_agree_bit_for_bit(gpu_lib, monkeypatch, meshes, cols, rows, n, precision):
    """The kernels with the cluster cull shared by a block's waves (picked for a body of more than 256 clusters) and the ones
    where every wave culls for itself, forced either way (RBS_SHARED_CULL, read at create time) on the same scenes:
    identical log-likelihoods and identical planes -- the cull only decides which clusters are looked at."""
    om, cam, P = sc.make_scene(meshes, cols, rows, max_particles=n)
    nb = len(meshes)
    eager = ob.Oracle(om, cam, P, max_particles=n, mode=ob.EAGER)
    frames = sc.make_frames(eager, nb, 3, seed=5)
    got = []
    for forced in ("0", "1"):
        monkeypatch.setenv("RBS_SHARED_CULL", forced)
        with RbSensor(om, cam, P, max_particles=n, precision=precision) as g:
            ll = sc.run_sequence(g, frames, n, n_bodies=nb)
            got.append((ll, [g.get_occlusion(slot) for slot in range(n)]))
    for a, b in zip(got[0][0], got[1][0]):
        assert np.array_equal(a, b)
    for a, b in zip(got[0][1], got[1][1]):
        assert np.array_equal(a, b)


def test_update_false_leaves_state_untouched(gpu_lib):
    """Non-final sampling blocks of a multi-object frame evaluate with update=false."""
    n = 16
    om, cam, P = sc.make_scene(("m1", "m3"), 640, 480, max_particles=n)
    eager = ob.Oracle(om, cam, P, max_particles=n, mode=ob.EAGER)
    frames = sc.make_frames(eager, 2, 2, seed=9)
    rng = np.random.default_rng(2)
    with RbSensor(om, cam, P, max_particles=n) as g:
        for s in (g, eager):
            s.reset()
        idx_g, idx_o = np.zeros(n, np.int32), np.zeros(n, np.int32)
        for truth, frame in frames:
            poses_a = synth.particle_poses(truth, n, rng)
            poses_b = synth.particle_poses(truth, n, rng)
            for s, idx in ((g, idx_g), (eager, idx_o)):
                s.set_observation(frame)
            before = g.get_occlusion(3)
            la_g = g.loglikes_poses(poses_a, idx_g, update=False)
            la_o = eager.loglikes_poses(poses_a, idx_o, update=False)
            assert np.array_equal(before, g.get_occlusion(3))
            lb_g = g.loglikes_poses(poses_b, idx_g, update=True)
            lb_o = eager.loglikes_poses(poses_b, idx_o, update=True)
            assert rel_err(la_g, la_o).max() <= TOL_EAGER
            assert rel_err(lb_g, lb_o).max() <= TOL_EAGER
            perm = rng.permutation(n).astype(np.int32)
            idx_g, idx_o = perm.copy(), perm.copy()
        for slot in range(n):
            assert_planes_match(g.get_occlusion(slot), eager.get_occlusion(slot))


def test_skipped_frames_advance_occlusion(gpu_lib):
    """Two set_observation calls between updating evaluations: the occlusion process runs
    over 2*delta_time."""
    n = 8
    om, cam, P = sc.make_scene(("m1",), 160, 120, max_particles=n)
    eager = ob.Oracle(om, cam, P, max_particles=n, mode=ob.EAGER)
    lazy = ob.Oracle(om, cam, P, max_particles=n, mode=ob.LAZY)
    frames = sc.make_frames(eager, 1, 3, seed=4)
    rng = np.random.default_rng(8)
    with RbSensor(om, cam, P, max_particles=n) as g:
        sensors = (g, eager, lazy)
        idx = [np.zeros(n, np.int32) for _ in sensors]
        for s in sensors:
            s.reset()
        out = []
        for k, (truth, frame) in enumerate(frames):
            poses = synth.particle_poses(truth, n, rng)
            res = []
            for s, ix in zip(sensors, idx):
                s.set_observation(frame)
                if k == 1:
                    s.set_observation(frame)  # a dropped evaluation
                res.append(s.loglikes_poses(poses, ix, update=True))
            out.append(res)
        for lg, le, ll_ in out:
            assert rel_err(lg, le).max() <= TOL_EAGER
            assert rel_err(lg, ll_).max() <= TOL_LAZY


def test_all_nan_frame_and_offscreen_particles(gpu_lib):
    n = 8
    om, cam, P = sc.make_scene(("m1",), 640, 480, max_particles=n)
    eager = ob.Oracle(om, cam, P, max_particles=n, mode=ob.EAGER)
    rng = np.random.default_rng(0)
    poses = synth.particle_poses(synth.truth_pose(1), n, rng)
    poses[1, 0, 9:12] = (5.0, 0.0, 0.7)    # off screen
    poses[2, 0, 9:12] = (0.0, 0.0, -1.0)   # behind the camera
    frame = np.full(640 * 480, np.nan)
    with RbSensor(om, cam, P, max_particles=n) as g:
        for s in (g, eager):
            s.reset()
            s.set_observation(frame)
        ig, io = np.zeros(n, np.int32), np.zeros(n, np.int32)
        lg = g.loglikes_poses(poses, ig, update=True)
        lo = eager.loglikes_poses(poses, io, update=True)
        assert np.array_equal(lg, np.zeros(n)) and np.array_equal(lo, np.zeros(n))
        a, b = eager.eager_coeffs(1)
        expect = np.float32(a) * np.float32(P.occlusion.initial_occlusion_prob) + np.float32(b)
        for slot in range(n):
            pl = g.get_occlusion(slot)
            assert np.array_equal(pl, eager.get_occlusion(slot))
            assert np.allclose(pl, expect, rtol=0, atol=1e-7)
        # now a real frame: off-screen / behind-camera particles contribute exactly 0
        d = eager.render_depth(synth.truth_pose(1))
        fr = synth.make_frame(d, 480, 640, rng)
        for s in (g, eager):
            s.set_observation(fr)
        lg = g.loglikes_poses(poses, ig, update=True)
        lo = eager.loglikes_poses(poses, io, update=True)
        assert lg[1] == 0.0 and lg[2] == 0.0
        assert rel_err(lg, lo).max() <= TOL_EAGER


def test_errors_through_the_c_abi(gpu_lib):
    om, cam, P = sc.make_scene(("m1_l2",), 80, 60, max_particles=4)
    with RbSensor(om, cam, P, max_particles=4) as g:
        with pytest.raises(RbSensorError):
            g.set_observation(np.zeros(10))
        poses = synth.particle_poses(synth.truth_pose(1), 5, np.random.default_rng(0))
        with pytest.raises(RbSensorError):  # n > max_particles
            g.loglikes_poses(poses, np.zeros(5, np.int32))
        with pytest.raises(RbSensorError):  # parent slot out of range
            g.loglikes_poses(poses[:2], np.array([0, 9], np.int32))
        assert g.loglikes_poses(poses[:0], np.zeros(0, np.int32)).size == 0
    bad = sc.make_scene(("m1_l2",), 80, 60, max_particles=4)
    bad[1].camera_matrix[0, 1] = 0.3  # skew is not supported
    with pytest.raises(RbSensorError):
        RbSensor(*bad, max_particles=4)


def test_create_destroy_repeatedly_from_threads(gpu_lib):
    """The service node builds and tears down a tracker per session on a worker thread
    (R:source/dbot_ros/tracker/object_tracker_service_node.cpp:233-256)."""
    import threading
    om, cam, P = sc.make_scene(("m1_l2",), 80, 60, max_particles=8)
    eager = ob.Oracle(om, cam, P, max_particles=8, mode=ob.EAGER)
    frames = sc.make_frames(eager, 1, 2, seed=1)
    ref = sc.run_sequence(eager, frames, 8)
    errs = []

    def session():
        try:
            with RbSensor(om, cam, P, max_particles=8) as g:
                got = sc.run_sequence(g, frames, 8)
            for a, b in zip(got, ref):
                assert rel_err(a, b).max() <= TOL_EAGER
        except Exception as e:  # surfaced below
            errs.append(e)

    for _ in range(3):
        th = threading.Thread(target=session)
        th.start()
        th.join()
    assert not errs, errs


def test_full_size_properties(gpu_lib):
    """BASELINE C1 size (2 000 particles, VGA, 5 120 triangles) through properties that do not
    need the oracle at full size: determinism, slot-permutation equivariance, the first 32
    particles against the oracle, untouched-pixel invariant."""
    n = 2000
    om, cam, P = sc.make_scene(("m1",), 640, 480, max_particles=n)
    eager = ob.Oracle(om, cam, P, max_particles=32, mode=ob.EAGER)
    rng = np.random.default_rng(11)
    truth = synth.truth_pose(1)
    frame = synth.make_frame(eager.render_depth(truth), 480, 640, rng)
    poses = synth.particle_poses(truth, n, rng, scale=2.0)
    with RbSensor(om, cam, P, max_particles=n) as g:
        g.reset()
        g.set_observation(frame)
        idx = np.zeros(n, np.int32)
        ll1 = g.loglikes_poses(poses, idx, update=True)
        # determinism: same call again from a fresh state is bitwise identical
        g.reset()
        g.set_observation(frame)
        idx = np.zeros(n, np.int32)
        ll2 = g.loglikes_poses(poses, idx, update=True)
        assert np.array_equal(ll1, ll2)
        # oracle on the first 32 particles
        eager.reset()
        eager.set_observation(frame)
        io = np.zeros(32, np.int32)
        lo = eager.loglikes_poses(poses[:32], io, update=True)
        assert rel_err(ll1[:32], lo).max() <= TOL_EAGER
        for slot in (0, 7, 31):
            assert_planes_match(g.get_occlusion(slot), eager.get_occlusion(slot))
        # second frame with a permutation of parents: evaluating child j from parent p(j) must
        # equal evaluating with the planes physically permuted
        perm = rng.permutation(n).astype(np.int32)
        g.set_observation(frame)
        ll_perm = g.loglikes_poses(poses, perm.copy(), update=False)
        ll_id = g.loglikes_poses(poses[np.argsort(perm)], np.arange(n, dtype=np.int32), update=False)
        # particle j with parent perm[j]  ==  particle at position perm[j] holding pose j
        assert np.array_equal(ll_perm[np.argsort(perm)], ll_id)
        # untouched pixels: a corner pixel is never covered -> pure occlusion process
        a, b = eager.eager_coeffs(1)
        corner = g.get_occlusion(1999)[0]
        assert corner == np.float32(np.float32(a) * np.float32(0.1) + np.float32(b)) or \
            abs(corner - (a * 0.1 + b)) < 1e-7


@pytest.mark.parametrize("name,meshes,cols,rows", [("single", ("m1_l2",), 80, 60),
                                                    ("multi", ("m1_l2", "box12"), 160, 120)])
def test_golden_sequences(gpu_lib, name, meshes, cols, rows):
    """The committed golden vectors (tests/golden/sequences.npz, tests/golden/coverage.npz)."""
    import os
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    g = np.load(os.path.join(gold, "sequences.npz"))
    n = 16
    om, cam, P = sc.make_scene(meshes, cols, rows, max_particles=n)
    frames = list(zip(g[f"{name}_truth"], g[f"{name}_frames"]))
    with RbSensor(om, cam, P, max_particles=n) as s:
        lls = np.array(sc.run_sequence(s, frames, n, n_bodies=len(meshes)))
        assert rel_err(lls, g[f"{name}_eager_loglik"]).max() <= TOL_EAGER
        assert rel_err(lls, g[f"{name}_lazy_loglik"]).max() <= TOL_LAZY
        assert_planes_match(s.get_occlusion(0), g[f"{name}_eager_occ_slot0"])
        assert_planes_match(s.get_occlusion(5), g[f"{name}_eager_occ_slot5"])


@pytest.mark.parametrize("mesh,cols,rows", [("m1_l2", 80, 60), ("m3", 160, 120), ("box12", 160, 120)])
def test_golden_coverage(gpu_lib, mesh, cols, rows):
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "coverage.npz"))
    om, cam, P = sc.make_scene((mesh,), cols, rows, max_particles=1)
    with RbSensor(om, cam, P, max_particles=1) as s:
        for pose, ref in zip(g[f"{mesh}_{cols}x{rows}_poses"], g[f"{mesh}_{cols}x{rows}_depth"]):
            assert np.array_equal(s.render_depth(pose).view(np.uint32), ref.view(np.uint32))


def test_filter_resampling_indices_match_oracle(gpu_lib):
    """north_star: 'likelihoods and resampling indices match the reference CPU path'.  The same
    filter block (weights, KL test, multinomial resampling from the SAME host-supplied
    uniforms) driven by the HIP sensor and by the lazy (reference-semantics) oracle must pick
    identical parents on every frame."""
    from dbot_ros_amd import filter as flt
    n = 64
    om, cam, P = sc.make_scene(("m1",), 640, 480, max_particles=n)
    lazy = ob.Oracle(om, cam, P, max_particles=n, mode=ob.LAZY)
    frames = sc.make_frames(lazy, 1, 5, seed=13)
    with RbSensor(om, cam, P, max_particles=n) as g:
        blocks = [flt.RbcFilterBlock(n, 2.0), flt.RbcFilterBlock(n, 2.0)]
        sensors = [g, lazy]
        for s in sensors:
            s.reset()
        rng = np.random.default_rng(99)
        n_resampled = 0
        for truth, frame in frames:
            poses = synth.particle_poses(truth, n, rng, scale=2.0)
            u = rng.random(n)
            out = []
            for s, b in zip(sensors, blocks):
                s.set_observation(frame)
                out.append(b.step(s, poses, u, update=True))
            (pg, lg), (po, lo) = out
            assert rel_err(lg, lo).max() <= TOL_LAZY
            assert (pg is None) == (po is None)
            if pg is not None:
                n_resampled += 1
                assert np.array_equal(pg, po)
        assert n_resampled >= 2


@pytest.mark.parametrize("slab_px", [0, 256])
def test_two_rank_sharding_on_one_gpu(gpu_lib, tmp_path, slab_px, state_layout):
    """dbot_ros_amd.dist.ShardedSensor over two processes (gloo rendezvous, both on cuda:0)
    with the PRODUCT sensor: log-likelihoods and parents equal the single-handle run, planes
    migrate across ranks as windows (rbs_export_window / rbs_import_window).  slab_px = 256: the ranks'
    handles start with slabs smaller than the object's region and enlarge them on their own schedules."""
    import subprocess
    import sys
    import os
    if slab_px and state_layout == "dense":
        pytest.skip("slabs are a windowed layout")
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dist_gpu_worker.py")
    port = 29700 + os.getpid() % 1000
    r = subprocess.run([sys.executable, script, str(port), str(slab_px)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "SHARDED_OK" in r.stdout


@pytest.mark.parametrize("factor,width,height", [(8, 640, 480), (1, 160, 120), (3, 322, 241)])
def test_native_frame_ingest_subsampling(gpu_lib, factor, width, height):
    """eval(row, col) = native(row*f, col*f), rows = height//f, cols = width//f
    (ri::to_eigen_vector, R:source/dbot_ros/util/ros_interface.h:152-168); bit-exact."""
    from dbot_ros_amd import CameraData
    rows, cols = height // factor, width // factor
    om, _, P = sc.make_scene(("m1_l2",), cols, rows, max_particles=4)
    K = synth.camera_matrix(width, height)
    cam = CameraData.from_native(K, width, height, factor)
    assert (cam.rows, cam.cols) == (rows, cols)
    rng = np.random.default_rng(1)
    native = rng.uniform(0.4, 2.0, size=(height, width)).astype(np.float32)
    native[rng.random(native.shape) < 0.05] = np.nan
    ref = native[: rows * factor: factor, : cols * factor: factor]
    assert ref.shape == (rows, cols)
    with RbSensor(om, cam, P, max_particles=4) as g:
        g.reset()
        g.set_observation_native(native, factor)
        got = g.get_observation().reshape(rows, cols)
        assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(ref).view(np.uint32))
        with pytest.raises(RbSensorError):
            g.set_observation_native(native[:-factor * 2], factor)
        # the same frame through the double-precision entry point gives the same likelihoods
        poses = synth.particle_poses(synth.truth_pose(1), 4, rng)
        i1, i2 = np.zeros(4, np.int32), np.zeros(4, np.int32)
        a = g.loglikes_poses(poses, i1, update=False)
        g.reset()  # same elapsed time (one frame) for the second evaluation
        g.set_observation(ref.astype(np.float64).ravel())
        b = g.loglikes_poses(poses, i2, update=False)
        assert np.array_equal(a, b)


@pytest.mark.parametrize("seed", range(40))
def test_randomized_scenes_match_oracle(gpu_lib, seed):
    """Random triangle soups (incl. slivers, huge and degenerate triangles, triangles crossing
    the camera plane), random intrinsics and odd resolutions, 1-3 bodies, NaN/inf pixels, random
    parent slots: depth bit-exact, log-likelihoods and planes as the oracle (device rule)."""
    from dbot_ros_amd import CameraData, ObjectModel, RbSensorBuilder
    rng = np.random.default_rng(1000 + seed)
    cols = int(rng.choice([5, 33, 64, 80, 97, 160, 322]))
    rows = int(rng.choice([7, 24, 60, 61, 120]))
    nb = int(rng.integers(1, 4))
    vs, ts = [], []
    for b in range(nb):
        nv = int(rng.integers(4, 60))
        v = rng.normal(size=(nv, 3)) * rng.choice([0.01, 0.05, 0.3])
        nt = int(rng.integers(1, 150))
        t = rng.integers(0, nv, size=(nt, 3)).astype(np.int32)   # duplicates -> degenerate triangles too
        vs.append(v)
        ts.append(t)
    om = ObjectModel(vs, ts, center=bool(rng.integers(0, 2)))
    f = float(rng.uniform(0.4, 1.5)) * cols
    K = np.array([[f, 0, rng.uniform(0.3, 0.7) * cols], [0, f * rng.uniform(0.8, 1.2), rng.uniform(0.3, 0.7) * rows],
                  [0, 0, 1.0]])
    cam = CameraData(K, rows, cols)
    n = int(rng.integers(1, 9))
    P = RbSensorBuilder.Parameters(sample_count=n)
    eager = ob.Oracle(om, cam, P, max_particles=n, mode=ob.EAGER)
    with RbSensor(om, cam, P, max_particles=n) as g:
        for s in (g, eager):
            s.reset()
        idx_g, idx_o = np.zeros(n, np.int32), np.zeros(n, np.int32)
        for k in range(3):
            from dbot_ros_amd.pose import pack_Rt, rotvec_to_matrix
            R = rotvec_to_matrix(rng.normal(size=(n, nb, 3)))
            t = np.stack([rng.normal(0, 0.1, (n, nb)), rng.normal(0, 0.1, (n, nb)),
                          rng.uniform(-0.1, 1.2, (n, nb))], -1)      # some bodies behind / across the camera plane
            poses = pack_Rt(R, t)
            frame = rng.uniform(0.2, 2.0, rows * cols)
            frame[rng.random(frame.size) < 0.1] = np.nan
            frame[rng.random(frame.size) < 0.02] = np.inf
            for i in range(min(n, 2)):
                dg, do = g.render_depth(poses[i]), eager.render_depth(poses[i])
                assert np.array_equal(dg.view(np.uint32), do.view(np.uint32))
            for s in (g, eager):
                s.set_observation(frame)
            upd = bool(rng.integers(0, 2)) or k == 2
            lg = g.loglikes_poses(poses, idx_g, update=upd)
            lo = eager.loglikes_poses(poses, idx_o, update=upd)
            assert np.isfinite(lo).all() and rel_err(lg, lo).max() <= TOL_EAGER, (k, lg, lo)
            idx_g = rng.integers(0, n, n).astype(np.int32)
            idx_o = idx_g.copy()
        for slot in range(n):
            assert_planes_match(g.get_occlusion(slot), eager.get_occlusion(slot))


def test_long_sequence_against_reference_semantics(gpu_lib):
    """120 frames at the reference's 80x60 operating point, resampling every frame: the device
    (eager float occlusion state) stays within north_star's 1e-5 (relative) of the oracle in
    reference (lazy, per-pixel time stamp) mode -- the rounding of the eager state is bounded,
    it does not accumulate with sequence length."""
    n = 24
    om, cam, P = sc.make_scene(("m1_l2",), 80, 60, max_particles=n)
    lazy = ob.Oracle(om, cam, P, max_particles=n, mode=ob.LAZY)
    eager = ob.Oracle(om, cam, P, max_particles=n, mode=ob.EAGER)
    rng = np.random.default_rng(21)
    worst_lazy = worst_eager = 0.0
    with RbSensor(om, cam, P, max_particles=n) as g:
        sensors = (g, lazy, eager)
        for s in sensors:
            s.reset()
        idx = [np.zeros(n, np.int32) for _ in sensors]
        for k in range(120):
            truth = synth.truth_pose(1, frame=k % 40)
            frame = synth.make_frame(lazy.render_depth(truth), 60, 80, rng)
            poses = synth.particle_poses(truth, n, rng, scale=1.0 + (k % 7))
            lls = []
            for s, ix in zip(sensors, idx):
                s.set_observation(frame)
                lls.append(s.loglikes_poses(poses, ix, update=True))
            worst_lazy = max(worst_lazy, float(rel_err(lls[0], lls[1]).max()))
            worst_eager = max(worst_eager, float(rel_err(lls[0], lls[2]).max()))
            w = np.exp(lls[1] - lls[1].max())
            parents = np.sort(rng.choice(n, size=n, p=w / w.sum())).astype(np.int32)
            idx = [parents.copy() for _ in sensors]
    assert worst_eager <= TOL_EAGER, worst_eager
    assert worst_lazy <= TOL_LAZY, worst_lazy


def test_create_destroy_does_not_leak_device_memory(gpu_lib):
    import torch
    om, cam, P = sc.make_scene(("m1_l2",), 160, 120, max_particles=64)
    poses = synth.particle_poses(synth.truth_pose(1), 64, np.random.default_rng(0))

    def cycle():
        with RbSensor(om, cam, P, max_particles=64) as g:
            g.set_observation(np.full(160 * 120, 0.8))
            g.loglikes_poses(poses, np.zeros(64, np.int32), update=True)

    for _ in range(3):
        cycle()
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    for _ in range(40):
        cycle()
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    assert free0 - free1 < 8 << 20, f"leaked {(free0 - free1) / 2**20:.1f} MiB over 40 create/destroy cycles"


def test_device_plane_export_import(gpu_lib):
    """rbs_export_plane / rbs_import_plane: the device-to-device leg of cross-GPU plane migration."""
    import torch
    n = 6
    om, cam, P = sc.make_scene(("m1_l2",), 160, 120, max_particles=n)
    eager = ob.Oracle(om, cam, P, max_particles=n, mode=ob.EAGER)
    frames = sc.make_frames(eager, 1, 2, seed=2)
    with RbSensor(om, cam, P, max_particles=n) as a, RbSensor(om, cam, P, max_particles=n) as b:
        sc.run_sequence(a, frames, n)
        buf = torch.empty(160 * 120, dtype=torch.float32, device="cuda")
        st = torch.cuda.current_stream().cuda_stream
        for slot in range(n):
            a.export_plane(slot, buf.data_ptr(), st)          # right after an updating call: must see the finished plane
            b.import_plane(n - 1 - slot, buf.data_ptr(), st)
            torch.cuda.current_stream().synchronize()
            assert np.array_equal(buf.cpu().numpy(), a.get_occlusion(slot))
        for slot in range(n):
            assert np.array_equal(b.get_occlusion(n - 1 - slot), a.get_occlusion(slot))
        with pytest.raises(RbSensorError):
            a.export_plane(n, buf.data_ptr(), st)


def test_device_api_bad_parent_slot_is_contained(gpu_lib):
    """The device-pointer API cannot validate parent slots on the host; an out-of-range slot
    must give NaN for that particle, not a wild read, and leave the others untouched."""
    import torch
    n = 8
    om, cam, P = sc.make_scene(("m1_l2",), 160, 120, max_particles=n)
    eager = ob.Oracle(om, cam, P, max_particles=n, mode=ob.EAGER)
    frames = sc.make_frames(eager, 1, 1, seed=2)
    poses = synth.particle_poses(frames[0][0], n, np.random.default_rng(0))
    with RbSensor(om, cam, P, max_particles=n) as g:
        for s in (g, eager):
            s.reset()
            s.set_observation(frames[0][1])
        ref = eager.loglikes_poses(poses, np.zeros(n, np.int32), update=True)
        d_poses = torch.from_numpy(poses.reshape(n, -1)).cuda()
        idx = np.zeros(n, np.int32)
        idx[3], idx[5] = 10 ** 6, -7
        d_idx = torch.from_numpy(idx).cuda()
        d_out = torch.empty(n, dtype=torch.float64, device="cuda")
        g.loglikes_device(d_poses.data_ptr(), d_idx.data_ptr(), n, True, d_out.data_ptr(), None)
        g.synchronize()
        out = d_out.cpu().numpy()
        assert np.isnan(out[3]) and np.isnan(out[5])
        ok = np.array([i not in (3, 5) for i in range(n)])
        assert rel_err(out[ok], ref[ok]).max() <= TOL_EAGER


@pytest.mark.parametrize("mesh", ["m1", "m3", "box12"])
def test_golden_coverage_vga(gpu_lib, mesh):
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "coverage_vga.npz"))
    om, cam, P = sc.make_scene((mesh,), 640, 480, max_particles=1)
    with RbSensor(om, cam, P, max_particles=1) as s:
        for k in range(5):
            d = s.render_depth(g[f"{mesh}_{k}_pose"])
            ids = np.nonzero(np.isfinite(d))[0]
            assert np.array_equal(ids, g[f"{mesh}_{k}_ids"])
            assert np.array_equal(d[ids].view(np.uint32), g[f"{mesh}_{k}_depth"].view(np.uint32))


def test_windows_follow_the_object(gpu_lib, state_layout):
    """An object sweeps across the image and then rests.  Planes stay those of the whole-plane
    oracle throughout; the stored windows (windowed layout) cover the swept region while its
    values still differ from the background and shrink back around the object afterwards."""
    n, cols, rows = 12, 160, 120
    om, cam, P = sc.make_scene(("m1_l2",), cols, rows, max_particles=n)
    P.delta_time = 0.5          # fast occlusion dynamics: the sweep decays within this test
    eager = ob.Oracle(om, cam, P, max_particles=n, mode=ob.EAGER)
    rng = np.random.default_rng(5)
    areas = []
    with RbSensor(om, cam, P, max_particles=n) as g:
        assert g.get_window(0) == ((cols, rows, 0, 0) if state_layout == "window" else (0, 0, cols, rows))
        idx_g = np.zeros(n, np.int32)
        idx_o = np.zeros(n, np.int32)
        for k in range(90):
            truth = synth.truth_pose(1, z=0.7).copy()
            truth[0, 9] = -0.12 + 0.008 * min(k, 30)      # 30 frames of motion, then rest
            frame = synth.make_frame(eager.render_depth(truth), rows, cols, rng)
            poses = synth.particle_poses(truth, n, rng, scale=2.0)
            g.set_observation(frame)
            eager.set_observation(frame)
            ll_g = g.loglikes_poses(poses, idx_g, update=True)
            ll_o = eager.loglikes_poses(poses, idx_o, update=True)
            assert rel_err(ll_g, ll_o).max() <= TOL_EAGER
            assert g.get_background() == eager.background()
            if k % 10 == 9 or k == 31:
                ws = [g.get_window(s) for s in range(n)]   # before get_occlusion makes them whole
                areas.append((k, max((w[2] - w[0]) * (w[3] - w[1]) for w in ws)))
                for slot in range(n):
                    assert_planes_match(g.get_occlusion(slot), eager.get_occlusion(slot))
            w = np.exp(ll_o - ll_o.max())
            parents = np.sort(rng.choice(n, size=n, p=w / w.sum())).astype(np.int32)
            idx_g, idx_o = parents.copy(), parents.copy()
        shared = g.shared_trail_state()[0]
    a = dict(areas)
    if state_layout == "dense":
        assert all(v == cols * rows for v in a.values())
    elif shared:
        # (forced runs of the suite with RBS_STP_ENTER=0: the trail the particles share is not in anybody's window)
        assert a[89] <= 64 * 64 and a[31] < cols * rows, areas
    else:
        assert a[31] >= 1.5 * a[89], areas         # swept region held at the end of the motion ...
        assert a[89] <= 64 * 64, areas             # ... and released once it has decayed
        assert a[31] < cols * rows


@pytest.mark.parametrize("variant", ["closed", "closed_inward", "with_holes", "mixed_winding", "two_shells",
                                     "unwelded", "one_shell_inside_out"])
def test_backface_culling_never_changes_a_depth(gpu_lib, variant):
    """Back faces are dropped only where that is exact: closed, consistently oriented bodies
    wholly in front of the camera.  Whatever the mesh -- inward winding, holes that show the
    inside, inconsistent winding, several shells, unwelded vertices -- and wherever it is (also
    around and across the camera plane), the rendered depth is the oracle's, bit for bit."""
    from dbot_ros_amd import CameraData, ObjectModel, RbSensorBuilder
    v, t = mesh_variants()[variant]
    cols, rows = 320, 240
    om = ObjectModel([v], [t], center=True)
    cam = CameraData(synth.camera_matrix(cols, rows), rows, cols)
    P = RbSensorBuilder.Parameters(sample_count=2)
    o = ob.Oracle(om, cam, P, max_particles=2)
    rng = np.random.default_rng(11)
    with RbSensor(om, cam, P, max_particles=2) as g:
        for k in range(14):
            z = [0.7, 0.4, 0.25, 0.12, 0.06, 0.03, 0.0][k % 7]      # far ... camera inside the body
            pose = synth.particle_poses(synth.truth_pose(1, z=z, frame=5 * k), 1, rng, scale=20.0)[0]
            pose[0, 9:11] *= 0.3 if z < 0.2 else 1.0
            dg, do = g.render_depth(pose), o.render_depth(pose)
            assert np.array_equal(dg.view(np.uint32), do.view(np.uint32)), \
                f"{variant} pose {k}: {(dg.view(np.uint32) != do.view(np.uint32)).sum()} depth pixels differ"


def test_many_particles_and_many_tiles(gpu_lib):
    """More than 4 096 particles (separate rectangle and scan kernels) and rectangles that split
    into several work items (several blocks add up one particle's log-likelihood): the first 48
    particles against the oracle over two frames, the rest through determinism."""
    n = 5000
    om, cam, P = sc.make_scene(("m1_l2",), 320, 240, max_particles=n)
    eager = ob.Oracle(om, cam, P, max_particles=48, mode=ob.EAGER)
    rng = np.random.default_rng(17)
    truth = synth.truth_pose(1, z=0.16)            # close: the rectangle is most of the image
    poses = synth.particle_poses(truth, n, rng, scale=2.0)
    runs = []
    with RbSensor(om, cam, P, max_particles=n) as g:
        for rep in range(2):
            g.reset()
            eager.reset()
            idx, io = np.zeros(n, np.int32), np.zeros(48, np.int32)
            lls = []
            frng = np.random.default_rng(3)
            for k in range(2):
                frame = synth.make_frame(eager.render_depth(truth), 240, 320, frng)
                g.set_observation(frame)
                eager.set_observation(frame)
                ll = g.loglikes_poses(poses, idx, update=True)
                lo = eager.loglikes_poses(poses[:48], io, update=True)
                assert rel_err(ll[:48], lo).max() <= TOL_EAGER
                lls.append(ll)
            assert_planes_match(g.get_occlusion(47), eager.get_occlusion(47))
            runs.append(np.concatenate(lls))
    assert np.array_equal(runs[0], runs[1])


def test_device_resident_frames(gpu_lib):
    """rbs_set_observation_device: frames already in HBM give exactly what the host-pointer
    ingest gives -- through the asynchronous device-pointer loglikes (where the ingest shares a
    launch with the call), through the host-pointer loglikes, with a frame nobody evaluated in
    between, and rbs_get_observation sees the pending frame."""
    import torch
    n, cols, rows = 40, 160, 120
    om, cam, P = sc.make_scene(("m1_l2",), cols, rows, max_particles=n)
    o = ob.Oracle(om, cam, P, max_particles=n, mode=ob.EAGER)
    rng = np.random.default_rng(9)
    truths = [synth.truth_pose(1, frame=k) for k in range(5)]
    frames = [synth.make_frame(o.render_depth(t), rows, cols, rng).astype(np.float32) for t in truths]
    poses = [synth.particle_poses(t, n, rng) for t in truths]
    dev = torch.device("cuda", 0)
    d_frames = [torch.from_numpy(f).to(dev) for f in frames]
    stream = torch.cuda.Stream(device=dev)
    with RbSensor(om, cam, P, max_particles=n) as a, RbSensor(om, cam, P, max_particles=n) as b:
        ia, ib = np.zeros(n, np.int32), np.zeros(n, np.int32)
        for k in range(5):
            a.set_observation(frames[k])
            if k == 2:                       # a frame that is never evaluated: time still advances
                a.set_observation(frames[k])
                b.set_observation_device(d_frames[k - 1].data_ptr(), stream.cuda_stream)
            b.set_observation_device(d_frames[k].data_ptr(), stream.cuda_stream)
            if k == 1:
                assert np.array_equal(b.get_observation(), frames[k], equal_nan=True)
            la = a.loglikes_poses(poses[k], ia, update=True)
            if k % 2 == 0:                   # host-pointer call picks the pending frame up
                lb = b.loglikes_poses(poses[k], ib, update=True)
            else:                            # device-pointer call on the frame's stream
                dp = torch.from_numpy(poses[k].reshape(n, -1)).to(dev)
                di = torch.from_numpy(ib).to(dev)
                do = torch.empty(n, dtype=torch.float64, device=dev)
                torch.cuda.synchronize()
                b.loglikes_device(dp.data_ptr(), di.data_ptr(), n, True, do.data_ptr(), stream.cuda_stream)
                b.synchronize()
                torch.cuda.synchronize()
                lb = do.cpu().numpy()
                ib[:] = np.arange(n)
            assert np.array_equal(la, lb)
            par = rng.permutation(n).astype(np.int32)
            ia, ib = par.copy(), par.copy()
        assert np.array_equal(a.get_occlusion(3), b.get_occlusion(3))


def test_layouts_agree_through_the_device_tracker(gpu_lib, monkeypatch):
    """The whole filter loop (transition, loglikes, weights, resampling on the device) run on
    windowed planes and on whole planes from the same seed, with an occluder passing through: the
    same estimates frame after frame.  (Planes are bit-identical across layouts; a log-likelihood
    can differ in its last bits because the rectangles are aligned differently, hence summed in a
    different order -- 1e-15 relative, far too little to change a resampling draw here.)"""
    from dbot_ros_amd import CameraData, ObjectModel, RbSensorBuilder, pose
    from dbot_ros_amd.tracker import DeviceParticleTracker, ObjectTransitionBuilder, ParticleTrackerBuilder
    n, cols, rows = 192, 160, 120
    v, f = synth.mesh_m1(level=2)
    om = ObjectModel([v], [f])
    cam = CameraData(synth.camera_matrix(cols, rows), rows, cols)
    P = RbSensorBuilder.Parameters(sample_count=n)

    def truth_state(k):
        Rt = synth.truth_pose(1, frame=k)[0]
        st = np.zeros(12)
        st[3:6] = pose.matrix_to_rotvec(Rt[:9].reshape(3, 3))
        st[0:3] = Rt[9:] - Rt[:9].reshape(3, 3) @ om.centers[0]
        return st

    out = {}
    for layout in ("window", "dense"):
        monkeypatch.setenv("RBS_STATE", layout)
        with RbSensor(om, cam, P, max_particles=n) as s:
            tr = DeviceParticleTracker(ObjectTransitionBuilder(ObjectTransitionBuilder.Parameters()).build(), s, om,
                                       ParticleTrackerBuilder.Parameters(evaluation_count=n), device_rng=True, seed=3)
            tr.initialize([truth_state(0)])
            rng = np.random.default_rng(0)
            ests = []
            for k in range(1, 121):
                kk = k % 40 if k % 40 < 20 else 40 - (k % 40)
                fr = synth.make_frame(s.render_depth(synth.truth_pose(1, frame=kk)), rows, cols, rng,
                                      occluder=(k % 50 > 35))
                ests.append(tr.track(fr).copy())
            w = s.get_window(0)
            out[layout] = (np.array(ests), w)
            tr.close()
    assert np.allclose(out["window"][0], out["dense"][0], rtol=0, atol=1e-9)
    assert np.isfinite(out["window"][0]).all()
    ww = out["window"][1]
    assert (ww[2] - ww[0]) * (ww[3] - ww[1]) < cols * rows // 2
    assert out["dense"][1] == (0, 0, cols, rows)


def test_wide_windows_take_the_streaming_path(gpu_lib, monkeypatch, state_layout):
    """Windowed planes whose windows cover most of the frame are copied by the whole-plane
    streaming kernel (window-aware) and re-tightened from per-block flags: same numbers, and the
    windows come back down once the planes have decayed."""
    if state_layout != "window":
        pytest.skip("windowed layout only")
    monkeypatch.setenv("RBS_WIDE_ENTER", "0.0")      # always take the wide path
    monkeypatch.setenv("RBS_TIMING_EVERY", "1")      # sample the stored area on every call
    n, cols, rows = 10, 160, 120
    om, cam, P = sc.make_scene(("m1_l2",), cols, rows, max_particles=n)
    P.delta_time = 0.5
    eager = ob.Oracle(om, cam, P, max_particles=n, mode=ob.EAGER)
    rng = np.random.default_rng(8)
    full = np.full(rows * cols, 0.8, np.float32)
    with RbSensor(om, cam, P, max_particles=n) as g:
        for slot in range(n):
            g.set_occlusion(slot, full)
            eager.set_occlusion(slot, full)
        ig, io = np.arange(n, dtype=np.int32), np.arange(n, dtype=np.int32)
        areas = []
        for k in range(70):
            truth = synth.truth_pose(1, frame=k % 10)
            frame = synth.make_frame(eager.render_depth(truth), rows, cols, rng)
            poses = synth.particle_poses(truth, n, rng, scale=2.0)
            g.set_observation(frame)
            eager.set_observation(frame)
            lg = g.loglikes_poses(poses, ig, update=True)
            lo = eager.loglikes_poses(poses, io, update=True)
            assert rel_err(lg, lo).max() <= TOL_EAGER
            w = g.get_window(3)
            areas.append((w[2] - w[0]) * (w[3] - w[1]))
            if k in (0, 20, 69):
                for slot in (0, 3, 9):
                    assert_planes_match(g.get_occlusion(slot), eager.get_occlusion(slot))
            par = rng.permutation(n).astype(np.int32)
            ig, io = par.copy(), par.copy()
    assert areas[0] == cols * rows            # everything differs from the background at first
    assert areas[-1] < cols * rows // 3       # ... and the block flags let the window shrink again


@pytest.mark.parametrize("seed", range(4))
def test_varying_particle_counts_and_call_patterns(gpu_lib, seed):
    """Twenty frames with the number of particles changing from call to call, read-only calls,
    skipped frames and an object that wanders: parents always index slots the latest updating
    call wrote.  Log-likelihoods and every live plane as the oracle (device rule)."""
    rng = np.random.default_rng(70 + seed)
    nmax, cols, rows = 24, 160, 120
    om, cam, P = sc.make_scene(("m1_l2", "box12")[: 1 + seed % 2], cols, rows, max_particles=nmax)
    nb = 1 + seed % 2
    eager = ob.Oracle(om, cam, P, max_particles=nmax, mode=ob.EAGER)
    with RbSensor(om, cam, P, max_particles=nmax) as g:
        live = 1                                  # after reset every slot holds the initial plane
        parents_ok = nmax
        for k in range(20):
            truth = synth.truth_pose(nb, frame=int(rng.integers(0, 40)), z=float(rng.uniform(0.5, 0.9)))
            frame = synth.make_frame(eager.render_depth(truth), rows, cols, rng)
            for _ in range(int(rng.integers(1, 3))):          # sometimes a frame nobody evaluates
                g.set_observation(frame)
                eager.set_observation(frame)
            n = int(rng.integers(1, nmax + 1))
            poses = synth.particle_poses(truth, n, rng, scale=float(rng.uniform(0.5, 4.0)))
            par = rng.integers(0, parents_ok, n).astype(np.int32)
            upd = bool(rng.random() < 0.7)
            ig, io = par.copy(), par.copy()
            lg = g.loglikes_poses(poses, ig, update=upd)
            lo = eager.loglikes_poses(poses, io, update=upd)
            assert rel_err(lg, lo).max() <= TOL_EAGER, (k, n, upd)
            if upd:
                parents_ok = live = n
                for slot in rng.choice(n, size=min(n, 3), replace=False):
                    assert_planes_match(g.get_occlusion(int(slot)), eager.get_occlusion(int(slot)))
        assert live >= 1


def test_stress_config_against_the_oracle(gpu_lib):
    """BASELINE C4's shape (50 880-triangle mesh at 1280x960, rectangles of many tiles whose
    partial sums several blocks add up) on a handful of particles over three frames."""
    n = 6
    om, cam, P = sc.make_scene(("m4",), 1280, 960, max_particles=n)
    eager = ob.Oracle(om, cam, P, max_particles=n, mode=ob.EAGER)
    rng = np.random.default_rng(4)
    with RbSensor(om, cam, P, max_particles=n) as g:
        ig, io = np.zeros(n, np.int32), np.zeros(n, np.int32)
        for k in range(3):
            truth = synth.truth_pose(1, z=0.5, frame=2 * k)
            frame = synth.make_frame(eager.render_depth(truth), 960, 1280, rng)
            poses = synth.particle_poses(truth, n, rng, scale=1.5)
            g.set_observation(frame)
            eager.set_observation(frame)
            lg = g.loglikes_poses(poses, ig, update=True)
            lo = eager.loglikes_poses(poses, io, update=True)
            assert rel_err(lg, lo).max() <= TOL_EAGER
            par = rng.integers(0, n, n).astype(np.int32)
            ig, io = par.copy(), par.copy()
        for slot in (0, n - 1):
            assert_planes_match(g.get_occlusion(slot), eager.get_occlusion(slot))


def test_out_of_device_memory_is_an_error_not_a_wreck(gpu_lib, state_layout):
    """More occlusion slots than the GPU has memory for: rbs_create reports RBS_ERR_OUT_OF_MEMORY,
    gives back what it had allocated, and leaves no sticky HIP error behind -- the next handle
    works."""
    if state_layout != "window":
        pytest.skip("layout-independent")
    import torch
    from dbot_ros_amd import _capi
    om, cam, P = sc.make_scene(("m1_l2",), 640, 480, max_particles=4)
    free0 = torch.cuda.mem_get_info()[0]
    too_many = int(free0 // (640 * 480 * 4)) // 2 + 2000      # two buffers of this many planes do not fit
    with pytest.raises(RbSensorError) as e:
        RbSensor(om, cam, P, max_particles=too_many, slab_px=-1)   # whole planes (the library's own choice would be slabs)
    assert e.value.code == _capi.RBS_ERR_OUT_OF_MEMORY
    assert torch.cuda.mem_get_info()[0] > 0.9 * free0
    with RbSensor(om, cam, P, max_particles=4) as g:
        assert np.isfinite(g.render_depth(synth.truth_pose(1))).any()


def test_hostile_inputs_match_the_oracle(gpu_lib):
    """NaN / infinite / astronomically large poses, a body without triangles, a frame of
    infinities: nothing crashes, nothing hangs, and the numbers are the oracle's."""
    from dbot_ros_amd import CameraData, ObjectModel, RbSensorBuilder
    v, t = synth.mesh_m1(level=2)
    empty_t = np.zeros((0, 3), np.int32)
    om = ObjectModel([v, v[:3] * 0.5], [t, empty_t], center=True)
    cols, rows, n = 96, 64, 8
    cam = CameraData(synth.camera_matrix(cols, rows), rows, cols)
    P = RbSensorBuilder.Parameters(sample_count=n)
    eager = ob.Oracle(om, cam, P, max_particles=n, mode=ob.EAGER)
    rng = np.random.default_rng(2)
    with RbSensor(om, cam, P, max_particles=n) as g:
        ig, io = np.zeros(n, np.int32), np.zeros(n, np.int32)
        for k in range(4):
            truth = synth.truth_pose(2, frame=k)
            poses = synth.particle_poses(truth, n, rng, scale=2.0)
            poses[1, 0, 9] = np.nan                  # NaN translation
            poses[2, 0, 0] = np.inf                  # infinite rotation entry
            poses[3, 0, 11] = 1e300                  # astronomically far
            poses[4, 0, 9:12] = (1e-300, -1e-300, 1e-310)   # at the camera centre, denormal depth
            poses[5, 0, :9] = 0.0                    # collapsed rotation: every triangle degenerate
            frame = synth.make_frame(eager.render_depth(truth), rows, cols, rng)
            if k == 2:
                frame[:] = np.inf
            g.set_observation(frame)
            eager.set_observation(frame)
            lg = g.loglikes_poses(poses, ig, update=True)
            lo = eager.loglikes_poses(poses, io, update=True)
            same_nan = np.isnan(lg) == np.isnan(lo)
            assert same_nan.all(), (lg, lo)
            ok = ~np.isnan(lo)
            assert rel_err(lg[ok], lo[ok]).max() <= TOL_EAGER
            par = rng.integers(0, n, n).astype(np.int32)
            ig, io = par.copy(), par.copy()
        for slot in range(n):
            a, b = g.get_occlusion(slot), eager.get_occlusion(slot)
            assert np.array_equal(np.isnan(a), np.isnan(b))
            assert_planes_match(np.nan_to_num(a, nan=0.5), np.nan_to_num(b, nan=0.5))


def test_layouts_hold_the_same_planes_under_stress(gpu_lib, monkeypatch, state_layout):
    """Differential test of the two layouts on identical inputs: random poses (some at or behind
    the camera plane, some far off screen), dense random frames, read-only calls, everybody
    inheriting one parent now and then.  Planes bit for bit; log-likelihoods to 1e-12 relative
    (the rectangles are aligned differently, so the additions come in a different order)."""
    if state_layout != "window":
        pytest.skip("runs both layouts itself")
    from dbot_ros_amd.pose import pack_Rt, rotvec_to_matrix
    n, cols, rows = 48, 160, 120
    om, cam, P = sc.make_scene(("m1_l2",), cols, rows, max_particles=n)
    monkeypatch.setenv("RBS_TIMING_EVERY", "1")
    monkeypatch.setenv("RBS_STATE", "window")
    a = RbSensor(om, cam, P, max_particles=n)
    monkeypatch.setenv("RBS_STATE", "dense")
    b = RbSensor(om, cam, P, max_particles=n)
    try:
        rng = np.random.default_rng(12)
        ia, ib = np.zeros(n, np.int32), np.zeros(n, np.int32)
        center = np.array([0.0, 0.0, 0.7])
        for k in range(80):
            center = center + rng.normal(0, 0.03, 3)
            center[2] = abs(center[2])
            R = rotvec_to_matrix(rng.normal(size=(n, 1, 3)))
            tt = center[None, None, :] + rng.normal(0, 0.05, (n, 1, 3))
            if k % 7 == 3:
                tt[:8, 0, 2] = rng.uniform(-0.05, 0.05, 8)
            if k % 5 == 2:
                tt[8:16, 0, 0] += 3.0
            poses = pack_Rt(R, tt)
            frame = rng.uniform(0.3, 1.5, rows * cols).astype(np.float32)
            frame[rng.random(frame.size) < 0.05] = np.nan
            a.set_observation(frame)
            b.set_observation(frame)
            upd = bool(rng.random() < 0.8)
            la = a.loglikes_poses(poses, ia, update=upd)
            lb = b.loglikes_poses(poses, ib, update=upd)
            assert np.array_equal(np.isnan(la), np.isnan(lb))
            ok = ~np.isnan(lb)
            assert rel_err(la[ok], lb[ok]).max() <= 1e-12
            if upd:
                par = rng.integers(0, n, n).astype(np.int32)
                if k % 3 == 0:
                    par[:] = par[0]
                ia, ib = par.copy(), par.copy()
                if k % 10 == 0:
                    for slot in (0, n // 2, n - 1):
                        assert np.array_equal(a.get_occlusion(slot), b.get_occlusion(slot))
    finally:
        a.close()
        b.close()


def test_sharded_tracker_matches_the_single_gpu_tracker(gpu_lib, state_layout):
    """tools/tracker_fps_dist.py with two ranks (gloo rendezvous, both on cuda:0) against the
    same tracker on one rank: every particle's log-likelihood comes from the same device code
    whatever rank evaluates it, so the estimates are identical -- and planes did migrate."""
    if state_layout != "window":
        pytest.skip("layout-independent")
    import json
    import os
    import subprocess
    import sys
    tool = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "tracker_fps_dist.py")
    env = dict(os.environ, RBS_BENCH_BACKEND="gloo")
    out = {}
    for world in (1, 2):
        port = 29300 + (os.getpid() + world) % 600
        r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
                            "--master-addr", "127.0.0.1", "--master-port", str(port), tool, "96", "6"],
                           capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
        out[world] = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert out[1]["estimate_digest"] == out[2]["estimate_digest"]
    assert out[2]["planes_migrated"] > 0 and out[1]["planes_migrated"] == 0
    assert out[2]["final_position_error_m"] < 0.01


def test_prefetched_frames_give_the_same_numbers(gpu_lib):
    """rbs_loglikes_prefetch hands frame k+1 over with call k (uploaded behind the call's kernels),
    rbs_set_observation_prefetched makes it the observation: log-likelihoods, planes and the model clock are those of
    rbs_set_observation_f32 + rbs_loglikes, bit for bit, in both precisions; a prefetched frame that another
    set_observation overtakes is abandoned, and a second activation is refused."""
    from dbot_ros_amd.sensor import RbSensorError
    n = 24
    om, cam, P = sc.make_scene(("m1_l2",), 160, 120, max_particles=n)
    orc = ob.Oracle(om, cam, P, max_particles=n, mode=ob.EAGER)
    frames = sc.make_frames(orc, 1, 6, seed=31)
    rng = np.random.default_rng(8)
    poses = [synth.particle_poses(t, n, rng, scale=2.0) for t, _ in frames]
    parents = [rng.integers(0, n, n).astype(np.int32) for _ in frames]
    for precision in ("f64", "f32"):
        with RbSensor(om, cam, P, max_particles=n, precision=precision) as a, RbSensor(om, cam, P, max_particles=n, precision=precision) as b:
            a.reset(); b.reset()
            idx_a, idx_b = np.zeros(n, np.int32), np.zeros(n, np.int32)
            b.set_observation(frames[0][1].astype(np.float32))
            for k in range(len(frames)):
                a.set_observation(frames[k][1].astype(np.float32))
                la = a.loglikes_poses(poses[k], idx_a, update=True)
                if k + 1 < len(frames):
                    lb = b.loglikes_poses_prefetch(poses[k], idx_b, frames[k + 1][1], update=True)
                    b.set_observation_prefetched()
                else:
                    lb = b.loglikes_poses(poses[k], idx_b, update=True)
                assert np.array_equal(la, lb), (precision, k)
                idx_a, idx_b = parents[k].copy(), parents[k].copy()
            for slot in (0, n // 2, n - 1):
                assert np.array_equal(a.get_occlusion(slot), b.get_occlusion(slot))
            assert a.get_background() == b.get_background()
            with pytest.raises(RbSensorError):
                b.set_observation_prefetched()                                   # nothing uploaded ahead
            b.loglikes_poses_prefetch(poses[0], idx_b.copy(), frames[1][1], update=False)
            b.set_observation(frames[2][1].astype(np.float32))                    # overtakes the prefetched frame
            with pytest.raises(RbSensorError):
                b.set_observation_prefetched()
            a.set_observation(frames[2][1].astype(np.float32))
            assert np.array_equal(a.loglikes_poses(poses[2], idx_a.copy(), update=False), b.loglikes_poses(poses[2], idx_b.copy(), update=False))
