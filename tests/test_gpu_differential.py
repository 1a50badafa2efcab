"""Differential tests across the CONFIGURATIONS of one build: whole planes on one device are the
reference; windowed planes, slabs, handles over several shards (and their combinations) must hold
the same planes bit for bit and return the same log-likelihoods (to 1e-12 where the tiling, hence
the order of the additions, may differ), under randomized call patterns -- varying particle
counts, read-only calls, skipped frames, everybody inheriting one parent, poses at and behind the
camera plane or far off screen."""
import numpy as np
import pytest

import scenarios as sc
from dbot_ros_amd import RbSensor, synth
from dbot_ros_amd.pose import pack_Rt, rotvec_to_matrix

pytestmark = pytest.mark.gpu


def rel_err(a, b):
    return np.abs(a - b) / np.maximum(1.0, np.abs(b))


CONFIGS = {
    "window": dict(state_layout="window"),
    "window x2 shards": dict(state_layout="window", device_ids=[0, 0]),
    "dense x3 shards": dict(state_layout="dense", device_ids=[0, 0, 0]),
}


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_wild_poses_and_dense_frames(gpu_lib, precision):
    """Windows grow to the whole frame here (dense random frames, objects all over the place): the
    windowed layouts go through their mid- and wide-window modes."""
    n, cols, rows = 48, 160, 120
    om, cam, P = sc.make_scene(("m1_l2",), cols, rows, max_particles=n)
    ref = RbSensor(om, cam, P, max_particles=n, precision=precision, state_layout="dense")
    others = {k: RbSensor(om, cam, P, max_particles=n, precision=precision, **kw) for k, kw in CONFIGS.items()}
    try:
        rng = np.random.default_rng(12)
        idx = np.zeros(n, np.int32)
        center = np.array([0.0, 0.0, 0.7])
        m = n
        for k in range(60):
            center = center + rng.normal(0, 0.03, 3)
            center[2] = abs(center[2])
            m = int(rng.integers(n // 2, n + 1)) if k % 4 == 1 else n
            R = rotvec_to_matrix(rng.normal(size=(m, 1, 3)))
            tt = center[None, None, :] + rng.normal(0, 0.05, (m, 1, 3))
            if k % 7 == 3:
                tt[:8, 0, 2] = rng.uniform(-0.05, 0.05, 8)
            if k % 5 == 2:
                tt[8:16, 0, 0] += 3.0
            poses = pack_Rt(R, tt)
            frame = rng.uniform(0.3, 1.5, rows * cols).astype(np.float32)
            frame[rng.random(frame.size) < 0.05] = np.nan
            upd = bool(rng.random() < 0.8)
            par = idx[:m].copy()
            ref.set_observation(frame)
            lr = ref.loglikes_poses(poses, par.copy(), update=upd)
            for name, s in others.items():
                s.set_observation(frame)
                lo = s.loglikes_poses(poses, par.copy(), update=upd)
                assert np.array_equal(np.isnan(lo), np.isnan(lr)), (name, k)
                ok = ~np.isnan(lr)
                assert rel_err(lo[ok], lr[ok]).max() <= 1e-12, (name, k, rel_err(lo[ok], lr[ok]).max())
            if upd:
                idx = rng.integers(0, m, n).astype(np.int32)        # parents among the slots just written
                if k % 3 == 0:
                    idx[:] = idx[0]
                if k % 10 == 0:
                    for slot in (0, m // 2, m - 1):
                        pr = ref.get_occlusion(slot)
                        for name, s in others.items():
                            assert np.array_equal(s.get_occlusion(slot), pr), (name, k, slot)
    finally:
        ref.close()
        for s in others.values():
            s.close()


SLAB_CONFIGS = {
    "slabs": dict(state_layout="window", slab_px=6400),
    "slabs x2 shards": dict(state_layout="window", slab_px=6400, device_ids=[0, 0]),
    "window x3 shards": dict(state_layout="window", device_ids=[0, 0, 0]),
}


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("meshes", [("m1_l2",), ("m1_l2", "box12")])
def test_wandering_objects_with_random_call_patterns(gpu_lib, precision, meshes):
    """A tracked scene (windows stay a few percent of the frame, so a third of the frame per slab is
    plenty): forty frames with changing particle counts, read-only calls, skipped frames."""
    nmax, cols, rows = 40, 160, 120
    nb = len(meshes)
    om, cam, P = sc.make_scene(meshes, cols, rows, max_particles=nmax)
    ref = RbSensor(om, cam, P, max_particles=nmax, precision=precision, state_layout="dense")
    others = {k: RbSensor(om, cam, P, max_particles=nmax, precision=precision, **kw) for k, kw in SLAB_CONFIGS.items()}
    try:
        rng = np.random.default_rng(70)
        parents_ok = nmax
        for k in range(40):
            truth = synth.truth_pose(nb, frame=int(rng.integers(0, 40)), z=float(rng.uniform(0.6, 0.9)))
            frame = synth.make_frame(ref.render_depth(truth), rows, cols, rng)
            for _ in range(int(rng.integers(1, 3))):          # sometimes a frame nobody evaluates
                ref.set_observation(frame)
                for s in others.values():
                    s.set_observation(frame)
            n = int(rng.integers(1, nmax + 1))
            poses = synth.particle_poses(truth, n, rng, scale=float(rng.uniform(0.5, 3.0)))
            par = rng.integers(0, parents_ok, n).astype(np.int32)
            upd = bool(rng.random() < 0.7)
            lr = ref.loglikes_poses(poses, par.copy(), update=upd)
            for name, s in others.items():
                lo = s.loglikes_poses(poses, par.copy(), update=upd)
                assert rel_err(lo, lr).max() <= 1e-12, (name, k, n, upd)
            if upd:
                parents_ok = n
                for slot in rng.choice(n, size=min(n, 3), replace=False):
                    pr = ref.get_occlusion(int(slot))
                    for name, s in others.items():
                        assert np.array_equal(s.get_occlusion(int(slot)), pr), (name, k, slot)
    finally:
        ref.close()
        for s in others.values():
            s.close()


@pytest.mark.parametrize("meshes,n", [(("m1_l2",), 240), (("m1_l2", "box12", "m1_l2"), 330)])
def test_device_tracker_across_configurations(gpu_lib, meshes, n):
    """rbs_tracker_* (transition, sensor, weights, KL, resampling, mean) with the same host-supplied
    randomness on every configuration: the same estimates and the same resampling decisions.  With
    three bodies there are two read-only sampling blocks and resamplings between them."""
    from dbot_ros_amd import pose
    from dbot_ros_amd.tracker import DeviceParticleTracker, ObjectTransitionBuilder, ParticleTrackerBuilder
    nb = len(meshes)
    per = n // nb
    cols, rows = 160, 120
    om, cam, P = sc.make_scene(meshes, cols, rows, max_particles=per)
    rng = np.random.default_rng(3)
    with RbSensor(om, cam, P, max_particles=1) as r:
        frames = [synth.make_frame(r.render_depth(synth.truth_pose(nb, frame=k)), rows, cols, rng, occluder=False).astype(np.float32)
                  for k in range(1, 9)]
    randomness = [(rng.standard_normal((nb, per, 6)), rng.random((nb, per))) for _ in frames]
    init = np.zeros(12 * nb)
    for b in range(nb):
        Rt = synth.truth_pose(nb, frame=0)[b]
        init[12 * b + 3:12 * b + 6] = pose.matrix_to_rotvec(Rt[:9].reshape(3, 3))
        init[12 * b:12 * b + 3] = Rt[9:] - Rt[:9].reshape(3, 3) @ om.centers[b]
    configs = {"dense": dict(state_layout="dense"), "window": dict(state_layout="window"),
               "slabs": dict(state_layout="window", slab_px=cols * rows // 2),
               "window x3 shards": dict(state_layout="window", device_ids=[0, 0, 0]),
               "slabs x2 shards": dict(state_layout="window", slab_px=cols * rows // 2, device_ids=[0, 0])}
    results = {}
    for name, kw in configs.items():
        with RbSensor(om, cam, P, max_particles=per, precision="f64", **kw) as s:
            trans = ObjectTransitionBuilder(ObjectTransitionBuilder.Parameters(part_count=nb)).build()
            tr = DeviceParticleTracker(trans, s, om, ParticleTrackerBuilder.Parameters(evaluation_count=n), np.random.default_rng(5))
            tr.initialize([init])
            ests = np.array([tr.track(f, nz, u) for f, (nz, u) in zip(frames, randomness)])
            results[name] = (ests, tr.n_resamplings)
            tr.close()
    ref, nres = results["dense"]
    assert nres >= 1
    for name, (ests, r_) in results.items():
        assert r_ == nres, name
        assert np.abs(ests - ref).max() <= 1e-9, (name, np.abs(ests - ref).max())


@pytest.mark.parametrize("precision,layout,ids", [("f32", "window", None), ("f32", "dense", None), ("f64", "window", None),
                                                  ("f32", "window", [0, 0])])
def test_host_call_routes_agree_bit_for_bit(gpu_lib, precision, layout, ids):
    """The host-pointer call's route -- frame read where it was uploaded, poses and parent slots
    pulled from pinned memory by the rectangles kernel, log-likelihoods stored into pinned memory
    by the raster kernel -- against the device-pointer route (rbs_set_observation_device +
    rbs_loglikes_device from device tensors: frame ingested into the handle's buffer, poses,
    parents and results in device memory): the same numbers and planes bit for bit over a
    resampled sequence with repeated, skipped and frame-buffer frames."""
    import torch
    n, cols, rows = 64, 160, 120
    om, cam, P = sc.make_scene(("m1_l2", "box12"), cols, rows, max_particles=n)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    host = RbSensor(om, cam, P, max_particles=n, precision=precision, state_layout=layout, device_ids=ids)
    devp = RbSensor(om, cam, P, max_particles=n, precision=precision, state_layout=layout, device_ids=ids)
    try:
        rng = np.random.default_rng(21)
        with RbSensor(om, cam, P, max_particles=1) as r:
            frames = [synth.make_frame(r.render_depth(synth.truth_pose(2, frame=k)), rows, cols, rng).astype(np.float32) for k in range(12)]
        d_frames = [torch.from_numpy(f).to(dev) for f in frames]
        torch.cuda.synchronize()
        for k in range(40):
            f = k % len(frames)
            m = n if k % 5 else n // 2
            poses = synth.particle_poses(synth.truth_pose(2, frame=f), m, rng)
            parents = rng.integers(0, n, m).astype(np.int32)
            upd = k % 4 != 3
            if k % 6 == 2:                          # two frames, the first never evaluated
                host.set_observation(frames[(k + 1) % len(frames)])
                devp.set_observation_device(d_frames[(k + 1) % len(frames)].data_ptr(), stream.cuda_stream)
            if k % 3 == 1:                          # through the handle's pinned buffer
                np.copyto(host.frame_buffer(), frames[f])
                host.commit_frame()
            elif k % 7 != 6:                        # (k % 7 == 6: the previous frame again, no new observation)
                host.set_observation(frames[f])
            if k % 3 == 1 or k % 7 != 6:
                devp.set_observation_device(d_frames[f].data_ptr(), stream.cuda_stream)
            got_host = host.loglikes_poses(poses, parents.copy(), update=upd)
            dp = torch.from_numpy(np.ascontiguousarray(poses.reshape(m, -1))).to(dev)
            di = torch.from_numpy(parents.copy()).to(dev)
            do = torch.empty(m, dtype=torch.float64, device=dev)
            torch.cuda.synchronize()
            devp.loglikes_device(dp.data_ptr(), di.data_ptr(), m, upd, do.data_ptr(), stream.cuda_stream)
            devp.synchronize()
            torch.cuda.synchronize()
            assert np.array_equal(got_host, do.cpu().numpy(), equal_nan=True), k
            if k % 10 == 9:
                assert np.array_equal(host.get_observation(), devp.get_observation(), equal_nan=True), k
        for slot in range(0, n, 7):
            assert np.array_equal(host.get_window(slot), devp.get_window(slot)), slot
            assert np.array_equal(host.get_occlusion(slot), devp.get_occlusion(slot)), slot
    finally:
        host.close()
        devp.close()


@pytest.mark.parametrize("precision", ["f32", "f64"])
def test_results_do_not_depend_on_the_raster_grid(gpu_lib, monkeypatch, precision):
    """The raster kernel's grid varies at run time (the raster / copy balance rule gives blocks to
    the copy kernel and takes them back; small calls split tiles by the number of blocks): the
    first round of items is static, the rest is drawn from a ticket counter, multi-tile particles
    are summed in item order.  Whatever the grid, the same log-likelihoods and planes bit for bit."""
    n, cols, rows = 96, 320, 240
    om, cam, P = sc.make_scene(("m1_l2", "box12"), cols, rows, max_particles=n)
    sensors = []
    for blocks in ("768", "640", "97", "8"):
        monkeypatch.setenv("RBS_RASTER_BLOCKS", blocks)
        sensors.append(RbSensor(om, cam, P, max_particles=n, precision=precision))
    monkeypatch.delenv("RBS_RASTER_BLOCKS")
    try:
        rng = np.random.default_rng(33)
        with RbSensor(om, cam, P, max_particles=1) as r:
            frames = [synth.make_frame(r.render_depth(synth.truth_pose(2, frame=k)), rows, cols, rng).astype(np.float32) for k in range(6)]
        for k in range(18):
            m = n if k % 4 else 17
            poses = synth.particle_poses(synth.truth_pose(2, frame=k % 6), m, rng)
            if k % 5 == 2:
                poses = poses.copy().reshape(m, 2, 12)
                poses[: m // 3, :, 11] *= 0.45          # close to the camera: rectangles of several tiles
                poses = poses.reshape(m, -1)
            parents = rng.integers(0, n, m).astype(np.int32)
            outs = []
            for s in sensors:
                s.set_observation(frames[k % 6])
                outs.append(s.loglikes_poses(poses, parents.copy(), update=k % 3 != 2))
            for o in outs[1:]:
                assert np.array_equal(outs[0], o, equal_nan=True), k
        for slot in range(0, n, 11):
            for s in sensors[1:]:
                assert np.array_equal(sensors[0].get_occlusion(slot), s.get_occlusion(slot)), slot
    finally:
        for s in sensors:
            s.close()


def test_host_frame_sent_in_pieces_arrives_whole(gpu_lib, monkeypatch):
    """A caller's host frame is staged and sent in pieces while the device is quiet (RBS_UPLOAD_CHUNKS,
    default 2; floats and doubles take different routes): whatever the number of pieces and wherever
    their boundaries fall -- frame sizes that are no multiple of the piece granularity included --
    the observation the device holds is the frame, and the log-likelihoods are those of one piece."""
    for cols, rows in ((640, 480), (324, 244), (80, 60)):
        n = 24
        om, cam, P = sc.make_scene(("m1_l2",), cols, rows, max_particles=n)
        truth = synth.truth_pose(1, frame=3)
        poses = synth.particle_poses(truth, n, np.random.default_rng(4)).reshape(n, 1, 12)
        runs = {}
        for chunks in ("1", "2", "3", "16"):
            monkeypatch.setenv("RBS_UPLOAD_CHUNKS", chunks)      # read when the handle is created
            rng = np.random.default_rng(5)
            with RbSensor(om, cam, P, max_particles=n) as s:
                idx = np.arange(n, dtype=np.int32)
                lls = []
                for k in range(6):
                    frame = rng.uniform(0.4, 1.2, rows * cols).astype(np.float32)
                    frame[rng.random(frame.size) < 0.03] = np.nan
                    # (k = 0: nothing has run yet -- one piece; afterwards the synchronous call before it left the device quiet)
                    s.set_observation(frame if k % 2 == 0 else frame.astype(np.float64))
                    np.testing.assert_array_equal(s.get_observation(), frame)
                    lls.append(s.loglikes_poses(poses, idx.copy(), update=True))
                runs[chunks] = np.stack(lls)
            assert np.isfinite(runs[chunks]).all()
            np.testing.assert_array_equal(runs[chunks], runs["1"])
