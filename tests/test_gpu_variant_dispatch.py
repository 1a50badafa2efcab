"""Which kernel a configuration launches (dbot_ros_amd/csrc: launch_raster, the copy-window / eval / depth launches of
enqueue_loglikes): every combination of the switches that select a template instantiation, each against the oracle.

A launch that names the wrong instantiation still launches a valid kernel -- one that reads slabs as whole planes, ignores the
shared plane, skips the update -- so every case runs three updating calls and one read-only call and checks every log-likelihood;
the read-only call must leave every plane and window as it found them, and one more updating call behind it is checked like the rest:

  precision F32 / F64, occlusion_mode DEVICE / REFERENCE, state_slab_px 0 / 256, RBS_SHARED_CULL 0 / 1 (the kernels for bodies of
  many clusters), one body / two bodies, shared trail off / forced (rbs_shared_trail_rebase), RBS_SPLIT 0 / 1 (two-kernel launch),
  RBS_FUSED_COPY 0 / 1 (the window copy inside the raster kernel / on the side stream).

8 particles at 80x60 (the golden size); one more case at 160x120 with two bodies.  Bars -- the ones the suite already applies to
the same configuration:
  F64, DEVICE      1e-9  relative to max(1, |ll|), EAGER oracle   (test_gpu_parity, test_gpu_slabs, test_gpu_round5, test_gpu_round6)
  F64, REFERENCE   1e-11 relative to max(1, |ll|), LAZY oracle    (test_gpu_exact_occlusion: whole planes, slabs, read-only calls)
  F32, DEVICE      test_gpu_f32's pair of bars against the EAGER oracle (1e-5 of |ll| on well-conditioned sums, 1e-6 of the sum of
                   term magnitudes for all); with the shared trail 1e-3 (test_gpu_round5 / test_gpu_round6: float32-level agreement)
Pairs the project asserts to be bit-identical elsewhere are bit-identical here: RBS_SHARED_CULL 0 / 1 (test_gpu_parity), RBS_SPLIT
0 / 1 (test_gpu_round6: the two launch forms on one handle), shared trail / scalar background (test_gpu_round5, test_gpu_round6).

rbs_create refuses F32 with REFERENCE ("occlusion_mode REFERENCE needs the binary64 likelihood (likelihood_precision F64) and the
windowed state layout (cols a multiple of 4)"): those 64 combinations are checked to be refused, nothing else is left out."""
import functools
import itertools

import numpy as np
import pytest

import oracle_binding as ob
import scenarios as sc
from dbot_ros_amd import RbSensor, RbSensorError, synth

pytestmark = pytest.mark.gpu

N = 8
READ_ONLY = 3          # the call that only looks, of the five of a case
SIZES = {"golden": (80, 60), "larger": (160, 120)}
MESHES = {1: ("m1_l2",), 2: ("m1_l2", "box12")}
REFUSAL = "occlusion_mode REFERENCE needs the binary64 likelihood"

# (precision, occlusion, slab_px, shared_cull, bodies, trail, split, fused)
AXES = (("f64", "f32"), ("device", "reference"), (0, 256), (0, 1), (1, 2), (0, 1), (0, 1), (0, 1))
ALL = list(itertools.product(*AXES))
REFUSED = [c for c in ALL if c[0] == "f32" and c[1] == "reference"]
ACCEPTED = [c for c in ALL if c not in REFUSED]


def _id(case):
    p, o, slab, cull, nb, trail, split, fused = case[:8]
    return f"{p}-{o}-slab{slab}-cull{cull}-bodies{nb}-trail{trail}-split{split}-fused{fused}" + (f"-{case[8]}" if len(case) > 8 else "")


def rel_err(a, b):
    return np.abs(a - b) / np.maximum(1.0, np.abs(b))


@functools.lru_cache(maxsize=None)
def _scene(nb, size):
    """Frames, poses, parents and both oracles' answers (LAZY: with the sums of term magnitudes) of one scene: computed once."""
    cols, rows = SIZES[size]
    om, cam, P = sc.make_scene(MESHES[nb], cols, rows, max_particles=N)
    rng = np.random.default_rng(17 + nb)
    with pytest.MonkeyPatch.context() as mp:
        mp.delenv("RBS_OCC", raising=False)      # (tooling that turns every EAGER oracle into the LAZY one: the modes are named here)
        oracles = {mode: ob.Oracle(om, cam, P, max_particles=N, mode=mode) for mode in (ob.EAGER, ob.LAZY)}
    frames = sc.make_frames(oracles[ob.EAGER], nb, 5, seed=11)
    poses = [synth.particle_poses(t, N, rng, scale=1.0 + 0.5 * k) for k, (t, _) in enumerate(frames)]
    parents = [np.zeros(N, np.int32)] + [np.sort(rng.choice(N, size=N)).astype(np.int32) for _ in range(4)]
    ref, S = {}, []
    for mode, o in oracles.items():
        o.reset()
        ref[mode] = []
        for k, (_, frame) in enumerate(frames):
            o.set_observation(frame)
            ref[mode].append(o.loglikes_poses(poses[k], parents[k].copy(), update=k != READ_ONLY))   # the fourth call only looks
            if mode == ob.LAZY:
                S.append(o.last_abs_sums(N))
        o.close()
    for a in ref[ob.EAGER] + ref[ob.LAZY] + S:
        a.setflags(write=False)
    return om, cam, P, frames, poses, parents, ref, S


@functools.lru_cache(maxsize=None)
def _run(case):
    """The case's five log-likelihood arrays: three updating calls, one read-only call, one more updating call."""
    precision, occlusion, slab, cull, nb, trail, split, fused = case[:8]
    om, cam, P, frames, poses, parents, _, _ = _scene(nb, case[8] if len(case) > 8 else "golden")
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("RBS_SHARED_CULL", str(cull))
        mp.setenv("RBS_SPLIT", str(split))
        mp.setenv("RBS_FUSED_COPY", str(fused))
        mp.delenv("RBS_SHARED_TRAIL", raising=False)
        mp.delenv("RBS_COPY_WALK", raising=False)
        g = RbSensor(om, cam, P, max_particles=N, precision=precision, occlusion=occlusion, slab_px=slab, state_layout="window")
    with g:
        if not trail:
            g.set_option("shared_trail", 0)
        g.reset()
        out = []
        for k, (_, frame) in enumerate(frames):
            g.set_observation(frame)
            if trail and k == 1:
                g.shared_trail_rebase(0)      # this updating call enters the shared trail; the next ones (and the read-only one) run in it
            if k == READ_ONLY:
                # (reading a windowed plane makes it dense in place: the planes first, then the windows as that leaves them)
                before = [(g.get_occlusion(q), g.get_window(q)) for q in range(N)]
            out.append(g.loglikes_poses(poses[k], parents[k].copy(), update=k != READ_ONLY))
            if k == READ_ONLY:
                for q, (plane, win) in enumerate(before):
                    assert g.get_window(q) == win and np.array_equal(g.get_occlusion(q), plane), q
        assert g.shared_trail_state()[0] == bool(trail)
    for a in out:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("case", ACCEPTED + [("f64", "device", 0, 0, 2, 0, 0, 1, "larger")], ids=_id)
def test_every_variant_against_the_oracle(gpu_lib, case):
    precision, occlusion, trail = case[0], case[1], case[5]
    *_, ref, S = _scene(case[4], case[8] if len(case) > 8 else "golden")
    want = ref[ob.LAZY if occlusion == "reference" else ob.EAGER]
    got = _run(case)
    for k, (a, b) in enumerate(zip(got, want)):
        assert np.isfinite(a).all(), k
        d = np.abs(a - b)
        print(f"{_id(case)} call {k}: {rel_err(a, b).max():.3e} relative, {(d / np.maximum(1.0, S[k])).max():.3e} of the term magnitudes")
        if precision == "f64":
            assert rel_err(a, b).max() <= (1e-11 if occlusion == "reference" else 1e-9), (k, rel_err(a, b).max())
        elif trail:
            assert rel_err(a, b).max() <= 1e-3, (k, rel_err(a, b).max())
        else:
            well = np.abs(b) >= 0.1 * S[k]
            assert (d[well] <= 1e-5 * np.maximum(1.0, np.abs(b[well]))).all(), (k, rel_err(a, b)[well].max())
            assert (d <= 1e-6 * np.maximum(1.0, S[k])).all(), (k, (d / np.maximum(1.0, S[k])).max())


@pytest.mark.parametrize("axis", [3, 5, 6], ids=["shared_cull", "shared_trail", "split"])
@pytest.mark.parametrize("case", [c for c in ACCEPTED if c[3] == 0 and c[5] == 0 and c[6] == 0], ids=_id)
def test_paired_variants_give_the_same_bits(gpu_lib, case, axis):
    """`case` has the three paired switches off: each of them on, alone, gives the same log-likelihoods bit for bit."""
    other = list(case)
    other[axis] = 1
    for k, (a, b) in enumerate(zip(_run(case), _run(tuple(other)))):
        assert np.array_equal(a, b), (k, int((a != b).sum()), float(np.abs(a - b).max()))


@pytest.mark.parametrize("case", [c for c in ACCEPTED if c[3] == 1 and c[5] == 1 and c[6] == 1], ids=_id)
def test_paired_variants_give_the_same_bits_with_all_of_them_on(gpu_lib, case):
    """... and so do all three together (the instantiations with more than one of these flags set)."""
    other = list(case)
    other[3] = other[5] = other[6] = 0
    for k, (a, b) in enumerate(zip(_run(case), _run(tuple(other)))):
        assert np.array_equal(a, b), (k, int((a != b).sum()), float(np.abs(a - b).max()))


@pytest.mark.parametrize("case", REFUSED, ids=_id)
def test_refused_combinations_are_refused(gpu_lib, case):
    precision, occlusion, slab, cull, nb = case[:5]
    om, cam, P = _scene(nb, "golden")[:3]
    with pytest.raises(RbSensorError, match=REFUSAL):
        RbSensor(om, cam, P, max_particles=N, precision=precision, occlusion=occlusion, slab_px=slab, state_layout="window")
