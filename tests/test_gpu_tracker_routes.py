"""rbs_tracker_* through the public API on every launch chain rbs_tracker_submit takes, where
tests/test_tracker.py reaches the fused chain only:

  - against oracle/tracker_oracle.c with host randomness at 512 particles (filter_step), 513 (filter_tail + gather, the
    re-centring deferred), 2 x 550 (separate launches on the first block, the tail on the last) and 9 001 (grid kernels);
  - once with host normals and DEVICE uniforms, against the oracle fed the twin's uniforms (tests/filter_twin.py);
  - the three A/B switches, each in a process of its own, against the default route bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest

import filter_twin as ft
import oracle_binding as ob
import scenarios as sc
from dbot_ros_amd import RbSensor, pose, synth
from dbot_ros_amd.tracker import DeviceParticleTracker, ObjectTransitionBuilder, ParticleTrackerBuilder

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
COLS, ROWS, TOL = 160, 120, 1e-9
SEED = 0x5EED0123456789AB


def _model_init(om, nb):
    init = np.zeros(12 * nb)
    for b in range(nb):
        Rt = synth.truth_pose(nb, frame=0)[b]
        init[12 * b + 3:12 * b + 6] = pose.matrix_to_rotvec(Rt[:9].reshape(3, 3))
        init[12 * b:12 * b + 3] = Rt[9:]            # model coordinates: pose of the centred mesh
    return init


def _against_the_oracle(meshes, n, frames, max_kl, device_uniforms=False):
    """The bars of test_device_tracker_matches_the_c_oracle_tracker: estimate and particles 1e-9, equal slot maps and
    resampling counts; max_kl chosen (on the oracle alone) so that blocks with and without a resampling both occur."""
    nb = len(meshes)
    per = n // nb
    om, cam, P = sc.make_scene(meshes, COLS, ROWS, max_particles=n)
    tp = ParticleTrackerBuilder.Parameters(evaluation_count=n, max_kl_divergence=max_kl, center_object_frame=False)
    orc = ob.Oracle(om, cam, P, max_particles=per, mode=ob.EAGER)
    trans = ObjectTransitionBuilder(ObjectTransitionBuilder.Parameters(part_count=nb)).build()
    ref = ob.OracleTracker(orc, per, trans.sigma, trans.vf, max_kl)
    with RbSensor(om, cam, P, max_particles=per) as s:
        dev = DeviceParticleTracker(trans, s, om, tp, np.random.default_rng(2), device_rng=device_uniforms, seed=SEED)
        assert dev.n == per
        init = _model_init(om, nb)
        dev.initialize([init])
        ref.initialize(init)
        rng, draw = np.random.default_rng(10), np.random.default_rng(2)
        for k in range(1, frames + 1):
            frame = synth.make_frame(orc.render_depth(synth.truth_pose(nb, frame=k)), ROWS, COLS, rng, occluder=False)
            normals, uniforms = draw.standard_normal((nb, per, 6)), draw.random((nb, per))
            if device_uniforms:     # the device draws them; the oracle gets the plain reference's
                uniforms = np.stack([ft.device_uniforms(SEED, k - 1, b, per) for b in range(nb)])
            ed = dev.track(frame, normals, None if device_uniforms else uniforms)
            er, nres = ref.track(frame, normals, uniforms)
            print(f"{meshes} n={n} frame {k}: estimate differs by {np.abs(ed - er).max():.3e}, resamplings {dev.n_resamplings} / {nres}")
            assert np.abs(ed - er).max() <= TOL, (k, np.abs(ed - er).max())
            pd, wd, idd = dev.get_state()
            pr, wr, idr = ref.get_state()
            assert np.abs(pd - pr).max() <= TOL and np.array_equal(idd, idr) and dev.n_resamplings == nres
        dev.close()
    assert 1 <= nres < frames * nb, nres       # a resampling, and a block without one


@pytest.mark.parametrize("meshes,n,frames,max_kl", [(("m1_l2",), 512, 5, 5.8), (("m1_l2",), 513, 5, 5.8),
                                                     (("m1_l2", "box12"), 1100, 5, 5.8), (("m1_l2",), 9001, 3, 8.0)],
                         ids=["fused_512", "tail_513", "separate_then_tail_2x550", "grid_9001"])
def test_every_chain_matches_the_c_oracle_tracker(gpu_lib, meshes, n, frames, max_kl):
    _against_the_oracle(meshes, n, frames, max_kl)


def test_device_uniforms_inside_the_real_call_sequence(gpu_lib):
    """Host normals, device uniforms (uniforms null, a seed): the oracle tracker fed the twin's uniforms."""
    _against_the_oracle(("m1_l2", "box12"), 1100, 5, 5.8, device_uniforms=True)


# ---------------------------------------------------------------- the A/B switches
_runs = {}


def _route(tmp_path_factory, n, switch):
    """Estimates and states of six frames in a fresh process with `switch` set; every child under its own time limit,
    and no further child once one has failed."""
    key = (n, switch)
    if key not in _runs:
        assert not _runs.get("failed"), "an earlier child did not exit 0: " + str(_runs.get("failed"))
        out = str(tmp_path_factory.mktemp("route") / "run.npz")
        env = {k: v for k, v in os.environ.items() if not k.startswith("RBS_TRACKER_")}
        if switch:
            env[switch[0]] = switch[1]
        r = subprocess.run([sys.executable, os.path.join(HERE, "tracker_route_worker.py"), out, str(n)], capture_output=True,
                           text=True, timeout=120, env=env)
        if r.returncode != 0:
            _runs["failed"] = (key, r.returncode)
        assert r.returncode == 0, (key, r.returncode, r.stdout[-2000:], r.stderr[-2000:])
        _runs[key] = dict(np.load(out))
    return _runs[key]


@pytest.mark.parametrize("n,switch", [(600, ("RBS_TRACKER_TAIL", "0")), (600, ("RBS_TRACKER_RECENTRE_NOW", "1")),
                                      (300, ("RBS_TRACKER_FUSED", "0"))], ids=["tail_off", "recentre_now", "fused_off"])
def test_switched_route_has_the_bits_of_the_default_route(gpu_lib, tmp_path_factory, n, switch):
    ref = _route(tmp_path_factory, n, None)
    got = _route(tmp_path_factory, n, switch)
    assert ref["resamplings"][-1] >= 1
    for k in ("estimates", "particles", "log_weights", "indices", "resamplings"):
        assert ref[k].dtype == got[k].dtype and ref[k].shape == got[k].shape, k
        same = ref[k].tobytes() == got[k].tobytes()
        assert same, (switch, k, float(np.abs(ref[k].astype(np.float64) - got[k]).max()))
