#!/usr/bin/env python3
"""bench.py -- particle-likelihoods/s of the RbSensor hot path on MI355X (BASELINE.json metric).

A "step" is one frame of BASELINE.json config C1 on one GPU: set_observation(frame k) +
RbSensor::loglikes(update=true) over 2 000 particles, one 5 120-triangle mesh (M1), 640x480
synthetic frames of SURVEY 8d's sequence (the object translates 2 mm and turns 1 degree per
frame; 30 frames played forwards and backwards), every child inheriting from a distinct random
parent slot (permutation: no occlusion plane is read twice, the worst case for HBM traffic).

`value` (the contract's number): inputs (frames, poses, parent indices, occlusion planes) resident
in HBM before the timed region, device-pointer API.  `--steps K` is the number of timed steps in all
(up to REPEATS regions, median region -> `ms_per_step`); `--dump-outputs DIR` writes the last timed
step's log-likelihoods as DIR/loglikes.npy (seeded inputs: the same for the same arguments, run after
run).

A plain run does only what `value` needs: set-up, warm-up, the timed steps, --dump-outputs, one JSON
line of the contract's keys.  Everything else the bench measures or checks runs with `--full` only,
after the headline, and the same JSON line then carries, as flat keys,

  host_api_*      the SAME steps through the host-pointer API the reference's filter would call:
                  frame upload, pose upload and log-likelihood download inside the clock
                  (SURVEY 8d's definition of the metric)
  tracker_fps_*   frames/s of the full per-frame step (frame upload + transition + loglikes +
                  weights + KL + resampling + mean) at 200 / 2 000 / 20 000 particles
  f32_*           the same resident steps with the opt-in float32 likelihood (the headline is F64,
                  the library default and the reference CPU model's arithmetic)
  roofline        dominant kernel of the headline run (windowed planes: the raster kernel, bound by
                  VALU issue): achieved = VALU wave-instructions/s from a LIVE rocprofv3 PMC pass
                  of this very command (child process) / live HIP-event kernel time; frac <= 1;
                  plus the measured HBM traffic (PMC, separate passes, gfx950 corrections) and the
                  algorithmic-bytes figure of SURVEY 8d for comparison
  dense_*         the same steps on whole planes (state_layout=dense), where the copy kernel is
                  dominant and HBM bound: algorithmic bytes / its live duration vs 8 TB/s
  cpu_baseline    the CPU oracle (reference CPU-path semantics) on this host: 1 thread (as dbot's
                  CPU model runs) and all cores
  configs / sweep / filter_step / exact_occlusion: the other BASELINE configurations, the moving-object
                  legs, the multi-rank step on one rank, occlusion_mode REFERENCE

With `torch.distributed.run` (--gpus N, one rank per GPU) a step is SURVEY 8(e)'s whole exchange: each rank's
2 000-particle shard (weak scaling) evaluated with GLOBAL parent slots -- the ranks' handles are attached to each
other over HIP IPC, a parent on another GPU is read in place over xGMI --, the RCCL all-gather of the
log-likelihoods, multinomial resampling over all ranks' particles and this rank's plan in one library call
(rbs_peer_resample), shared remote parents staged once; then the same step at C3 / C4's per-GPU sizes and the
one-handle tracker over the job's devices (a time-limited child process) -- with `--full`, which also runs the multi-GPU
self-check before anything is timed.  Ranks that cannot attach fall back to shards with local parents + the all-gather,
and the line says so (`peer_step`).

`python bench.py --gpus N` WITHOUT torch.distributed.run (WORLD_SIZE unset) measures the other
multi-GPU form: ONE process, one handle over N devices (rbs_config.n_devices; --device-ids to
list them, an ordinal may repeat on a one-GPU box): N x 2 000 particles per step through
rbs_loglikes from host memory (frame + pose upload and log-likelihood download inside the
clock), plus (`--full`) the sharded device tracker's frames/s.
"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_PEAK_GBPS = 8000.0        # MI355X_MICROARCH.md: 8.0 TB/s spec (6.29 TB/s measured float4 copy)
HBM_COPY_MEASURED_GBPS = 6290.0
# VALU issue ceilings of this chip in G wave64-instructions/s, chip-wide (1 024 SIMDs).
# MEASURED (tools/valu_bench.hip, profiles/r04_valu_issue_microbench.txt: kernels of 6-55 ms, every block's
# start / end and cycle count logged, 1..8 waves per SIMD; wall-clock rates cross-checked against the chip's own
# counters, SQ_INSTS_VALU / (SQ_BUSY_CYCLES / 32 / clock): profiles/r04_valu_issue_pmc.txt, profiles/README.md):
# the rates SATURATE at -- float32 / integer add 1 000-1 023 (v_fma_f32 868-1 074), binary64 add / mul / fma / min
# 576-592, v_rcp_f64 (every division) 151.  (Round 3 quoted 735 / 454 / 142 from 60-180 us kernels whose launch and
# ramp were a sixth of the measurement.)  The SIMD issues its OLDEST wave first: pure-VALU waves finish staggered,
# which is why round 3's per-wave cycle counts did not add up to the wall clock.
VALU_PEAK_F32_GINST = 1020.0
VALU_PEAK_F64_GINST = 590.0
VALU_PEAK_TRANS_F64_GINST = 151.0
# The guide's figures (MI355X_MICROARCH.md, per-instruction cycle constants): v_fma_f32 wave64 = 2 cycles per SIMD,
# binary64 at half rate = 4, at 2.4 GHz; a binary64 transcendental holds the pipe 16 cycles (measured, above).
GUIDE_PEAK_F32_GINST = 1024 * 2.4 / 2.0      # 1 228.8
GUIDE_PEAK_F64_GINST = 1024 * 2.4 / 4.0      # 614.4
GUIDE_PEAK_TRANS_F64_GINST = 1024 * 2.4 / 16.0   # 153.6
REPEATS = 5                   # the headline is the median of up to this many timed regions, --steps steps in all
MIN_REGION_STEPS = 20         # ... of at least this many steps each (fewer steps in all: one region)
MIN_WARMUP_STEPS = 100        # the headline's untimed steps at the least, whatever --warmup says: the first ~50 steps after a
                              # short warm-up run ~4 % slow (a fixed count, not a time: the dumped outputs stay reproducible)
DUMP_BYTES = 64 << 20         # --dump-outputs: at most this many bytes in all (a fixed, seeded sample beyond)
WORKLOAD_FLAGS = ("particles", "cols", "rows", "mesh", "parents", "update", "sequence", "precision", "layout", "slab_px")


# BASELINE.json's configurations as single-GPU workloads (C3 / C4: the 1/8 slice one GPU of the 8 carries)
PRESETS = {"c1": {}, "c1_readonly": {"update": 0},
           "c2": {"mesh": "m1,m2,m3", "particles": 6666, "steps": 50},
           "c3_slice": {"particles": 25000, "steps": 20, "warmup": 3},
           "c4_slice": {"mesh": "m4", "cols": 1280, "rows": 960, "particles": 6250, "steps": 5, "warmup": 2},
           "default_res": {"cols": 80, "rows": 60}}


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None,
                    help="timed steps of the headline in all (default 500, or the --config preset's), split into up to "
                         f"{REPEATS} timed regions of at least {MIN_REGION_STEPS} steps")
    ap.add_argument("--warmup", type=int, default=None,
                    help=f"untimed steps before the first timed region (default 20, or the preset's; at least {MIN_WARMUP_STEPS} are run)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write what the timed path returned in its last step as DIR/<name>.npy")
    ap.add_argument("--particles", type=int, default=2000, help="particles per GPU")
    ap.add_argument("--cols", type=int, default=640)
    ap.add_argument("--rows", type=int, default=480)
    ap.add_argument("--mesh", default="m1")
    ap.add_argument("--parents", default="permutation",
                    choices=["permutation", "identity", "resampled", "peaked", "peaked_unsorted"])
    ap.add_argument("--update", type=int, default=1, help="0: read-only evaluation (non-final blocks)")
    ap.add_argument("--sequence", type=int, default=30, help="frames in the moving-object sequence (0: one static frame)")
    ap.add_argument("--config", default=None, choices=["c1", "c1_readonly", "c2", "c3_slice", "c4_slice", "default_res"],
                    help="a row of BASELINE.md section 3 (sets mesh / particles / resolution / steps; c1 = no flags)")
    ap.add_argument("--fill-planes", type=float, default=None,
                    help="start from planes that differ from the background everywhere (windows = whole frame): "
                         "the windowed layout's worst case")
    ap.add_argument("--fill-fraction", type=float, default=1.0,
                    help="with --fill-planes: only a central rectangle of this fraction of the frame")
    ap.add_argument("--precision", default="f64", choices=["f64", "f32"],
                    help="likelihood precision of the headline run (f64 = the library default, the reference CPU model's arithmetic)")
    ap.add_argument("--layout", default="window", choices=["window", "dense"], help="occlusion state layout of the headline run")
    ap.add_argument("--occlusion", default=None, choices=["reference", "device"],
                    help="rbs_config.occlusion_mode of the headline run (default: the library's)")
    ap.add_argument("--slab-px", type=int, default=0, help="floats per occlusion slot (rbs_config.state_slab_px; 0 = whole planes)")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, everything else: its kernel times and roofline (live counters), the dense / other-precision / "
                         "occlusion-mode / configuration / sweep / host / tracker legs, the CPU baseline; several ranks: the self-check and "
                         "the multi-rank legs (without it: set-up, warm-up, the timed steps, --dump-outputs and the line, nothing else)")
    ap.add_argument("--quick", action="store_true",
                    help="with --full: the headline's kernel times and roofline (committed counters) only: no dense / f64 / host / tracker / cpu / pmc legs")
    ap.add_argument("--no-dense-leg", action="store_true", help="skip the whole-plane (state_layout=dense) comparison run")
    ap.add_argument("--no-f32-leg", action="store_true", help="skip the opt-in float32-likelihood comparison run")
    ap.add_argument("--no-host-leg", action="store_true")
    ap.add_argument("--no-tracker-fps", action="store_true")
    ap.add_argument("--no-configs-leg", action="store_true", help="skip the C2 / C3-slice / C4-slice / read-only / 80x60 runs")
    ap.add_argument("--no-sweep-leg", action="store_true", help="skip the moving-object / window-fraction legs")
    ap.add_argument("--sweep-only", action="store_true", help="only the moving-object / window-fraction legs (prints their keys)")
    ap.add_argument("--no-pmc", action="store_true", help="no live rocprofv3 counter passes (roofline falls back to profiles/)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-seconds", type=float, default=12.0)
    ap.add_argument("--device-ids", default=None, help="in-process multi-device mode: comma-separated HIP ordinals (default 0..N-1)")
    ap.add_argument("--in-process", action="store_true",
                    help="ONE process, one handle over --gpus devices through the host-pointer API (the default for --gpus > 1 "
                         "without torch.distributed.run; with --gpus 1 the same steps on a plain handle, for comparison)")
    ap.add_argument("--resample-temperature", type=float, default=1.0,
                    help="several ranks: weights = exp((ll - max) / T) in the global resampling of every step (1 = the filter's own weights)")
    ap.add_argument("--pmc-child", action="store_true", help=argparse.SUPPRESS)   # the process rocprofv3 wraps
    ap.add_argument("--sharded-tracker-child", action="store_true", help=argparse.SUPPRESS)   # one handle over --device-ids: tracker frames/s
    a = ap.parse_args()
    explicit = {k: getattr(a, k) for k in ("steps", "warmup") if getattr(a, k) is not None}   # (win over a preset)
    a.steps, a.warmup = 500, 20
    for k, v in PRESETS.get(a.config, {}).items():
        setattr(a, k, v)
    for k, v in explicit.items():
        setattr(a, k, v)
    if a.steps < 1 or a.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if a.quick or a.config not in (None, "c1") or not a.full:
        a.no_dense_leg = a.no_f32_leg = a.no_host_leg = a.no_tracker_fps = a.no_cpu_baseline = a.no_configs_leg = a.no_sweep_leg = True
        a.no_pmc = a.no_pmc or a.quick or not a.full
    return a


# --------------------------------------------------------------------------------- scene
def build_scene(a):
    from dbot_ros_amd import CameraData, ObjectModel, RbSensorBuilder, synth
    mesh_fns = {"m1": synth.mesh_m1, "m2": synth.mesh_m2, "m3": synth.mesh_m3, "m4": synth.mesh_m4,
                "box12": synth.mesh_box12}
    meshes = [mesh_fns[m]() for m in a.mesh.split(",")]
    om = ObjectModel([v for v, _ in meshes], [t for _, t in meshes], center=True)
    cam = CameraData(synth.camera_matrix(a.cols, a.rows), a.rows, a.cols)
    P = RbSensorBuilder.Parameters(sample_count=a.particles)
    return om, cam, P, sum(len(t) for _, t in meshes), len(meshes)


class Workload:
    """Frames, poses and parent indices of the moving-object sequence, on the host and in HBM."""

    def __init__(self, a, om, cam, P, nb, device, rank):
        from dbot_ros_amd import RbSensor, synth
        n = a.particles
        rng = np.random.default_rng(0)
        prng = np.random.default_rng(1 + rank)
        F = max(1, a.sequence)
        self.truths = [synth.truth_pose(nb, frame=k) for k in range(F)]
        with RbSensor(om, cam, P, device_id=device.index, max_particles=1) as r:   # the product's own render hook
            self.frames = np.stack([synth.make_frame(r.render_depth(t), a.rows, a.cols, rng) for t in self.truths]).astype(np.float32)
        self.poses = np.stack([synth.particle_poses(t, n, prng).reshape(n, -1) for t in self.truths])
        self.order = list(range(F)) + list(range(F - 2, 0, -1))      # forwards, then backwards
        if a.parents == "permutation":
            parents = synth.resample_like_indices(n, prng)
        elif a.parents == "identity":
            parents = np.arange(n, dtype=np.int32)
        elif a.parents == "resampled":
            parents = synth.resample_like_indices(n, prng, concentration=1.0)
        else:  # a tracker's usual regime: few survivors, many siblings
            parents = synth.resample_like_indices(n, prng, concentration=0.02)
            if a.parents == "peaked_unsorted":
                parents = prng.permutation(parents).astype(np.int32)
        self.parents = parents
        self.d_poses = torch.from_numpy(self.poses).to(device)             # [F][n][12*bodies]
        self.d_frames = torch.from_numpy(self.frames).to(device)           # [F][rows*cols]
        self.d_idx = torch.from_numpy(parents).to(device)
        self.pose_bytes = self.d_poses[0].numel() * 8
        self.frame_bytes = self.d_frames[0].numel() * 4


def fill_planes(sensor, a):
    plane = np.full((a.rows, a.cols), np.float32(0.1), dtype=np.float32)      # = the background after reset
    fr = float(np.sqrt(min(1.0, max(0.0, a.fill_fraction))))
    r0, c0 = int(a.rows * (1 - fr) / 2), int(a.cols * (1 - fr) / 2)
    plane[r0:a.rows - r0, c0:a.cols - c0] = a.fill_planes
    for slot in range(a.particles):
        sensor.set_occlusion(slot, plane.ravel())


class ResidentRun:
    """set_observation_device + loglikes_device on a caller-owned stream, everything in HBM."""

    def __init__(self, a, W, sensor, stream, d_out):
        self.a, self.W, self.sensor, self.stream, self.d_out = a, W, sensor, stream, d_out
        self.count = 0

    def launch(self):
        a, W = self.a, self.W
        k = W.order[self.count % len(W.order)]
        self.count += 1
        if a.sequence > 0:
            self.sensor.set_observation_device(W.d_frames.data_ptr() + k * W.frame_bytes, self.stream.cuda_stream)
        self.sensor.loglikes_device(W.d_poses.data_ptr() + k * W.pose_bytes, W.d_idx.data_ptr(), a.particles,
                                    bool(a.update), self.d_out.data_ptr(), self.stream.cuda_stream)

    def timed(self, steps, warmup, after=None, barrier=None):
        for _ in range(warmup):
            self.launch()
            if after:
                after()
        torch.cuda.synchronize()
        if barrier:
            barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            self.launch()
            if after:
                after()
        torch.cuda.synchronize()
        if barrier:
            barrier()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def kernel_times(self, launches=512):
        """Average kernel durations over >= 200 launches, from the HIP events the library records
        on the streams its kernels run on (every 2nd call carries events in this pass)."""
        self.sensor.set_timing_every(2)
        for _ in range(launches):
            self.launch()
        torch.cuda.synchronize()
        call_ms, copy_ms, n_used = self.sensor.timing_summary(launches)
        raster_ms = self.sensor.raster_kernel_ms(launches)
        self.sensor.set_timing_every(8)
        return raster_ms, copy_ms, call_ms, n_used


class PeerRun(ResidentRun):
    """world > 1, one process per GPU: SURVEY 8(e)'s step with its hard part inside the clock --
    set_observation_device + loglikes_device(update) on this rank's shard with GLOBAL parent slots (parents in
    other ranks' handles are read in place over xGMI through HIP-IPC mappings; parents that several local
    children share are pulled once by rbs_stage_windows), the all-gather of the log-likelihoods (RCCL), and a
    multinomial resampling over ALL ranks' particles (device-resident torch arithmetic, identical on every rank)
    that produces the next step's parents.  dbot_ros_amd/dist.py PeerShardedStep; nothing touches the host."""

    def __init__(self, a, W, sensor, stream, step, uniforms):
        super().__init__(a, W, sensor, stream, step.d_out)
        self.step, self.uniforms = step, uniforms
        self.distinct = torch.zeros(1, dtype=torch.int64, device=step.d_out.device)
        self.steps_done = 0
        self.reduce = None                 # sums a small int64 tensor over the ranks (setup_peer_run)

    def launch(self):
        a, W = self.a, self.W
        k = W.order[self.count % len(W.order)]
        u = self.uniforms[self.count % len(self.uniforms)]
        self.count += 1
        if a.sequence > 0:
            self.sensor.set_observation_device(W.d_frames.data_ptr() + k * W.frame_bytes, self.stream.cuda_stream)
        ps = self.step.step(W.d_poses[k], u)
        if not self.step.fused:            # (the library kernel counts the distinct parents of this rank's children itself)
            self.distinct += (ps[1:] != ps[:-1]).sum() + 1
        self.steps_done += 1

    def reset_stats(self):
        self.step.counts.zero_()
        self.step.children = 0
        self.distinct.zero_()
        self.steps_done = 0

    def stats(self):
        """Job-wide: the ranks' counters summed (every rank calls this at the same point)."""
        c = self.step.counts.to(torch.int64).clone()
        if self.step.fused:
            runs = c[3:4]
        else:
            runs = self.distinct.clone()
            c = c[:3]
        t = torch.cat([c[:3], runs, torch.tensor([self.step.children], dtype=torch.int64, device=c.device)])
        if self.reduce is not None:
            t = self.reduce(t)
        c = t.cpu().numpy().astype(np.float64)
        ch = max(1.0, c[4])
        world = max(1, self.step.world)
        steps = max(1, self.steps_done)
        return {"remote_parent_frac": c[0] / ch, "remote_children_served_from_staging_frac": (c[1] / c[0]) if c[0] else 0.0,
                "planes_staged_per_step_per_rank": c[2] / steps / world,
                # (fused: runs of equal parents per rank, summed -- a parent whose children straddle two ranks counts twice;
                #  tensor path: distinct parents of the whole job as every rank sees them, hence / world)
                "distinct_parents_per_step": c[3] / steps / (1 if self.step.fused else world)}


def single_rank_filter_step_leg(a, om, cam, P, W, dev, stream, steps=300):
    """N = 1 only: the step the multi-rank lines time -- loglikes(update) with the parents the previous step's resampling chose,
    the (here trivial) exchange of the log-likelihoods, multinomial resampling + plan in one library call (rbs_peer_resample),
    staging -- on ONE rank.  The headline times rbs_loglikes alone (BASELINE's metric); `--gpus N` times this step, so its
    values are to be set against THIS figure, not against the headline."""
    from dbot_ros_amd import dist as rdist
    n = a.particles
    sensor = make_sensor(a, om, cam, P, dev, n=2 * n)
    try:
        prime(sensor, a, W)
        pstep = rdist.PeerShardedStep(sensor, n, 2 * n, device=dev, min_share=2, stream=stream.cuda_stream,
                                      temperature=a.resample_temperature, fused=True, world=1, rank=0)
        gen = torch.Generator().manual_seed(1234)
        uniforms = [torch.rand(n, dtype=torch.float64, generator=gen).sort().values.to(dev) for _ in range(16)]
        run = PeerRun(a, W, sensor, stream, pstep, uniforms)
        el = run.timed(steps, a.warmup)
        st = run.stats()
        ll = pstep.d_out.cpu().numpy()
        return {"filter_step_value": n * steps / el, "filter_step_ms_per_step": el / steps * 1e3,
                "filter_step_finite": bool(np.isfinite(ll).all()),
                "filter_step_distinct_parents_per_step": st["distinct_parents_per_step"],
                "filter_step_note": "ONE rank doing what every rank of `--gpus N` does per step: loglikes(update) with the parents the previous step's "
                                    "resampling chose + exchange of the log-likelihoods (a copy here) + multinomial resampling and plan (rbs_peer_resample) + "
                                    "staging, all on one stream.  The multi-rank `value`s are to be compared with N x THIS figure (the headline times "
                                    "rbs_loglikes alone, on permutation parents: every particle its own plane -- after a resampling the children of one "
                                    "parent share its lines)"}
    finally:
        sensor.close()


class LocalShardRun(ResidentRun):
    """The multi-rank step WITHOUT cross-rank parents (every rank's children inherit from its own slots) + the
    all-gather of the log-likelihoods: what bench.py --gpus N falls back to when the ranks' handles cannot be
    attached to each other (rbs_ipc_attach); the line says so (`peer_step`)."""

    def __init__(self, a, W, sensor, stream, d_out, d_all, gather):
        super().__init__(a, W, sensor, stream, d_out)
        self.d_all, self.gather = d_all, gather

    def launch(self):
        super().launch()
        self.sensor.stream_join(self.stream.cuda_stream)
        self.gather(self.d_all, self.d_out)


def setup_peer_run(a, om, cam, P, W, dev, stream, dist, backend, world):
    """One rank's handle (n own slots + n staging slots), attached to the other ranks', and its PeerRun."""
    from dbot_ros_amd import dist as rdist
    n = a.particles
    sensor = make_sensor(a, om, cam, P, dev, n=2 * n)
    prime(sensor, a, W)
    try:
        if os.environ.get("RBS_BENCH_FAIL_ATTACH") == "1":      # (tests: the fallback of a job whose handles cannot attach)
            raise RuntimeError("attach_peers failed -- RBS_BENCH_FAIL_ATTACH=1")
        rdist.attach_peers(sensor)
    except RuntimeError:
        torch.cuda.synchronize()
        dist.barrier()
        sensor.close()
        raise

    def gather(out_t, inp_t):
        if backend == "nccl":
            dist.all_gather_into_tensor(out_t, inp_t)      # RCCL over xGMI, on `stream`
        else:                                              # (functional tests on a box with fewer GPUs than ranks)
            host = [torch.empty(n, dtype=torch.float64) for _ in range(world)]
            dist.all_gather(host, inp_t.cpu())
            out_t.copy_(torch.cat(host))

    # resampling + this rank's plan in ONE library launch (rbs_peer_resample) at sorted uniforms; RBS_BENCH_TENSOR_RESAMPLE=1:
    # the same arithmetic as ~45 tensor kernels (dist.global_resample + dist.plan_shard), for comparison
    fused = os.environ.get("RBS_BENCH_TENSOR_RESAMPLE") != "1"
    pstep = rdist.PeerShardedStep(sensor, n, 2 * n, device=dev, min_share=2, stream=stream.cuda_stream, all_gather=gather,
                                  temperature=a.resample_temperature, fused=fused,
                                  shared_trail=os.environ.get("RBS_BENCH_PEER_SHARED_TRAIL", "1") != "0")   # (agreed by one all-reduce every 32 steps)
    gen = torch.Generator().manual_seed(1234)        # the same uniforms on every rank
    uniforms = [torch.rand(n * world, dtype=torch.float64, generator=gen) for _ in range(16)]
    if fused:
        uniforms = [u.sort().values for u in uniforms]
    uniforms = [u.to(dev) for u in uniforms]
    run = PeerRun(a, W, sensor, stream, pstep, uniforms)

    def reduce(t):
        if backend == "nccl":
            dist.all_reduce(t)
            return t
        h = t.cpu()
        dist.all_reduce(h)
        return h

    run.reduce = reduce
    return sensor, run


def multi_gpu_selfcheck(a, dev, stream, dist, backend, world, rank, n=256, steps=4, temperature=60.0):
    """SURVEY 8(e)'s equality test on the job's OWN devices, before anything is timed (the first run on a
    multi-GPU node must validate itself): `steps` steps of the multi-rank step -- loglikes(update) with GLOBAL parents,
    the all-gather, the resampling over all ranks' particles, staging -- at n particles per rank, then ONE handle on
    rank 0 holding all world * n particles replays the same poses, frames and uniforms.  Equal means: every rank's
    gathered log-likelihood vector agrees with the single handle's to 1e-12 relative (the order of a particle's partial
    sums depends on the call's particle count), and every rank's slice of the resampled parents is identical.  Never raises: a failure is reported in the line and the job goes on to its timed run."""
    import copy
    from dbot_ros_amd import RbSensor, synth
    from dbot_ros_amd import dist as rdist
    res = {"multi_gpu_check": f"{steps} steps x {n} particles per rank x {world} ranks against one handle holding {n * world} (rank 0), "
                              f"resampling temperature {temperature:g}"}
    b = copy.copy(a)
    b.particles = n
    om, cam, P, n_tri, nb = build_scene(b)
    N = n * world
    sensor = None
    errs = []
    try:
        with RbSensor(om, cam, P, max_particles=1, device_id=dev.index, precision=a.precision) as r1:
            rng = np.random.default_rng(0)
            truths = [synth.truth_pose(nb, frame=k) for k in range(steps)]
            frames = [synth.make_frame(r1.render_depth(t), cam.rows, cam.cols, rng) for t in truths]
        rng = np.random.default_rng(12)
        poses = [synth.particle_poses(t, N, rng, scale=2.0).reshape(N, -1) for t in truths]     # by global SLOT
        gen = torch.Generator().manual_seed(5)
        uniforms = [torch.rand(N, dtype=torch.float64, generator=gen).sort().values for _ in range(steps)]
        sensor = RbSensor(om, cam, P, max_particles=2 * n, device_id=dev.index, precision=a.precision, state_layout=a.layout)
        sensor.reset()
    except Exception as e:   # noqa: BLE001
        errs.append(f"setup: {e!r}")
    attach_ok = False
    if sensor is not None:
        try:
            if os.environ.get("RBS_BENCH_FAIL_ATTACH") == "1":
                raise RuntimeError("attach_peers failed -- RBS_BENCH_FAIL_ATTACH=1")
            rdist.attach_peers(sensor)     # (raises on EVERY rank when any rank fails, after all of them left the hand-shake)
            attach_ok = True
        except RuntimeError as e:
            errs.append(str(e))
    flags = [None] * world
    dist.all_gather_object(flags, (sensor is not None, attach_ok))
    res["ipc_attach_ok"] = [bool(f[1]) for f in flags]
    mine_ll, mine_ps, counts, seen = [], [], [0, 0, 0, 0], 0
    if all(f[0] and f[1] for f in flags):
        def gather(out_t, inp_t):
            if backend == "nccl":
                dist.all_gather_into_tensor(out_t, inp_t)
            else:
                host = [torch.empty(inp_t.numel(), dtype=inp_t.dtype) for _ in range(world)]
                dist.all_gather(host, inp_t.cpu())
                out_t.copy_(torch.cat(host))
        try:
            # which ranks does the collective really reach?  every rank contributes its number
            mark_in = torch.full((n,), float(rank), dtype=torch.float64, device=dev)
            mark_out = torch.full((N,), -1.0, dtype=torch.float64, device=dev)
            gather(mark_out, mark_in)
            torch.cuda.synchronize()
            seen = int(torch.unique(mark_out[mark_out >= 0]).numel())
            pstep = rdist.PeerShardedStep(sensor, n, 2 * n, device=dev, min_share=2, stream=stream.cuda_stream, all_gather=gather,
                                          temperature=temperature, fused=True)
            for k in range(steps):
                sensor.set_observation(frames[k])
                d_poses = torch.from_numpy(poses[k][rank * n:(rank + 1) * n].copy()).to(dev)
                ps = pstep.step(d_poses, uniforms[k].to(dev))
                torch.cuda.synchronize()
                mine_ll.append(pstep.d_all.cpu().numpy().copy())
                mine_ps.append(ps.cpu().numpy().copy())
            counts = [int(c) for c in pstep.counts.cpu().tolist()]
        except Exception as e:   # noqa: BLE001
            errs.append(f"rank {rank} step: {e!r}")
        torch.cuda.synchronize()
        dist.barrier()                 # nobody unmaps while a peer may still be reading
    if sensor is not None:
        sensor.close()
    everyone = [None] * world
    dist.all_gather_object(everyone, {"ll": mine_ll, "ps": mine_ps, "counts": counts, "seen": seen, "errs": errs})
    if rank != 0:
        return {}
    res["rccl_ranks_seen"] = [e["seen"] for e in everyone]
    res["multi_gpu_check_remote_children"] = [e["counts"][0] for e in everyone]
    res["multi_gpu_check_planes_staged"] = [e["counts"][2] for e in everyone]
    all_errs = [m for e in everyone for m in e["errs"]]
    if all_errs or not all(len(e["ll"]) == steps for e in everyone):
        res["multi_gpu_equals_single"] = False
        res["peer_read_ok"] = [False] * world
        res["multi_gpu_check_diagnosis"] = "the multi-rank step did not complete: " + ("; ".join(all_errs) or "a rank recorded fewer steps")
        return res
    try:
        ref_ll, ref_ps = [], []
        with RbSensor(om, cam, P, max_particles=N, device_id=dev.index, precision=a.precision, state_layout=a.layout) as one:
            one.reset()
            idx = np.zeros(N, np.int32)
            for k in range(steps):
                one.set_observation(frames[k])
                ll = one.loglikes_poses(poses[k], idx, update=True)
                ps = rdist.global_resample(torch.from_numpy(ll), uniforms[k], temperature).numpy()
                ref_ll.append(ll.copy()); ref_ps.append(ps.copy())
                idx = ps.astype(np.int32)
        worst, bad_parents, read_ok = 0.0, 0, []
        for r_, e in enumerate(everyone):
            ok_r = True
            for k in range(steps):
                d = np.abs(e["ll"][k] - ref_ll[k])
                # (not bit for bit: how a rectangle is cut into work items -- hence the order a particle's partial sums are
                # added in -- depends on the number of particles in the call, n here and world * n there)
                same = bool((d <= 1e-12 * np.maximum(1.0, np.abs(ref_ll[k]))).all())
                worst = max(worst, float(np.nanmax(d)) if d.size else 0.0)
                wrong = int((e["ps"][k] != ref_ps[k][r_ * n:(r_ + 1) * n]).sum())
                bad_parents += wrong
                ok_r = ok_r and same and wrong == 0
            read_ok.append(bool(ok_r))
        res["multi_gpu_equals_single"] = bool(all(read_ok))
        res["peer_read_ok"] = read_ok
        res["multi_gpu_check_max_abs_loglik_diff"] = worst
        res["multi_gpu_check_parent_mismatches"] = bad_parents
        if not all(read_ok):
            res["multi_gpu_check_diagnosis"] = (f"ranks {[r_ for r_, o in enumerate(read_ok) if not o]} disagree with the single handle: max |d loglik| "
                                                f"{worst:.3e}, {bad_parents} parents differ; remote children per rank {res['multi_gpu_check_remote_children']} "
                                                "(a rank whose children never had a remote parent did not exercise the peer reads)")
    except Exception as e:   # noqa: BLE001
        res["multi_gpu_equals_single"] = False
        res["multi_gpu_check_diagnosis"] = f"the single-handle replay failed: {e!r}"
    return res


def peer_configs_leg(a, dev, stream, dist, backend, world, rank, names=("c3_slice", "c4_slice")):
    """BASELINE C3 / C4 at their real per-GPU sizes (25 000 / 6 250 particles per rank) through the same multi-rank
    step: whole-job particle-likelihoods/s (MAX over ranks of the elapsed time) and where the parents were."""
    import copy
    res = {}
    for name in names:
        b = copy.copy(a)
        for k, v in PRESETS[name].items():
            setattr(b, k, v)
        b.steps = max(b.steps, 10)
        om, cam, P, n_tri, nb = build_scene(b)
        W = Workload(b, om, cam, P, nb, dev, rank)
        s, run = setup_peer_run(b, om, cam, P, W, dev, stream, dist, backend, world)
        el = run.timed(b.steps, 3, barrier=dist.barrier)
        t = torch.tensor([el], dtype=torch.float64, device=dev if backend == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        el = float(t.item())
        ok = bool(torch.isfinite(run.step.d_all).all().item())
        st = run.stats()
        torch.cuda.synchronize()
        dist.barrier()                     # nobody frees planes a peer may still be reading
        s.close()
        if not ok:
            raise SystemExit(f"non-finite log-likelihoods in the {name} leg")
        key = name.replace("_slice", "")
        res[f"{key}_value"] = b.particles * world * b.steps / el
        res[f"{key}_ms_per_step"] = el / b.steps * 1e3
        res[f"{key}_particles_total"] = b.particles * world
        for k_, v_ in st.items():
            res[f"{key}_{k_}"] = v_
        del W, run
        torch.cuda.empty_cache()
    res["configs_note"] = (f"BASELINE C3 ({25000 * world} particles, M1, 640x480) and C4 ({6250 * world} particles, M4 = 50 880 triangles, "
                           f"1280x960) over {world} ranks: the same step as the headline (global resampling every step), whole-job rates")
    return res


def make_sensor(a, om, cam, P, device, precision=None, layout=None, n=None, occlusion=None):
    from dbot_ros_amd import RbSensor
    lay = layout or a.layout
    prec = precision or a.precision
    occ = occlusion or getattr(a, "occlusion", None)
    if occ == "reference" and (lay != "window" or prec != "f64"):
        occ = "device"   # (stamped planes: binary64 likelihood on windowed planes only)
    return RbSensor(om, cam, P, device_id=device.index, max_particles=n or a.particles,
                    precision=prec, state_layout=lay, slab_px=a.slab_px if lay == "window" else 0, occlusion=occ)


def prime(sensor, a, W):
    sensor.reset()
    if os.environ.get("RBS_BENCH_PRINT_PTRS") == "1":     # (tools/dbg/bimodal.sh: does a run's speed follow where its planes lie?)
        sys.stderr.write("# planes at 0x%x / 0x%x\n" % (sensor.occlusion_device_ptr(0), sensor.occlusion_device_ptr(0, next_buffer=True)))
    if a.fill_planes is not None:
        fill_planes(sensor, a)
    sensor.set_observation(W.frames[0])
    sensor.synchronize()


def configs_leg(a, dev, stream, names=("c1_readonly", "c2", "c3_slice", "c4_slice", "default_res")):
    """The other BASELINE configurations on this GPU, same clock as the headline (inputs resident
    in HBM, the 30-frame sequence): flat `<config>_value` / `_ms_per_step` / `_raster_kernel_ms` keys."""
    import copy
    res = {}
    for name in names:
        b = copy.copy(a)
        for k, v in PRESETS[name].items():
            setattr(b, k, v)
        b.steps = max(b.steps, 20) if name != "c1_readonly" and name != "default_res" else 300
        om, cam, P, n_tri, nb = build_scene(b)
        W = Workload(b, om, cam, P, nb, dev, 0)
        d_out = torch.empty(b.particles, dtype=torch.float64, device=dev)
        s = make_sensor(b, om, cam, P, dev)
        prime(s, b, W)
        run = ResidentRun(b, W, s, stream, d_out)
        el = run.timed(b.steps, max(3, min(b.warmup, 10)))
        if not np.isfinite(d_out.cpu().numpy()).all():
            raise SystemExit(f"non-finite log-likelihoods in the {name} leg")
        raster_ms, copy_ms, _, _ = run.kernel_times(64)
        s.close()
        res[f"{name}_value"] = b.particles * b.steps / el
        res[f"{name}_ms_per_step"] = el / b.steps * 1e3
        res[f"{name}_raster_kernel_ms"] = raster_ms
        if b.update:
            res[f"{name}_copy_kernel_ms"] = copy_ms
        del W, d_out
        torch.cuda.empty_cache()
    res["configs_note"] = ("the same timed loop on BASELINE's other configurations, one GPU, precision " + a.precision + ": c1_readonly = "
                           "loglikes(update=false); c2 = 6 666 particles x (M1, M2, M3), particle-likelihoods/s (x3 = body renders/s); "
                           "c3_slice = 25 000 particles (1/8 of C3); c4_slice = 6 250 particles, mesh M4 (50 880 triangles), 1280x960 "
                           "(1/8 of C4); default_res = C1 at 80x60 (downsampling_factor 8)")
    return res


def sweep_truths(n_frames):
    """The travelling object of the sweep legs: along the diagonal of the visible volume at 0.7 m and back, 2 mm per frame."""
    from dbot_ros_amd import synth
    p0, p1 = np.array([-0.30, -0.21, 0.7]), np.array([0.30, 0.21, 0.7])
    length = float(np.linalg.norm(p1 - p0))
    truths = []
    for k in range(n_frames):
        s_ = (0.002 * k) % (2.0 * length)
        s_ = s_ if s_ <= length else 2.0 * length - s_           # there and back
        t = synth.truth_pose(1, frame=k % 360).copy()
        t[0, 9:12] = p0 + (p1 - p0) * (s_ / length)
        truths.append(t)
    return truths


def sweep_tracker_run(make, om, frames, truths, n, tail, shared_trail):
    """The device tracker (its own KL-triggered resampling) following the sweep's object, frame by frame from host memory: rate over the
    last `tail` frames, stored window fraction at the end.  make() -> the sensor (a context manager); shared_trail: RBS_SHARED_TRAIL."""
    from dbot_ros_amd import pose
    from dbot_ros_amd.tracker import DeviceParticleTracker, ObjectTransitionBuilder, ParticleTrackerBuilder
    n_frames = len(frames)
    init = np.zeros(12)
    Rt = truths[0][0]
    init[3:6] = pose.matrix_to_rotvec(Rt[:9].reshape(3, 3))
    init[0:3] = Rt[9:] - Rt[:9].reshape(3, 3) @ om.centers[0]
    old_env = os.environ.get("RBS_SHARED_TRAIL")
    os.environ["RBS_SHARED_TRAIL"] = "1" if shared_trail else "0"
    try:
        with make() as s:
            trans = ObjectTransitionBuilder(ObjectTransitionBuilder.Parameters(part_count=1)).build()
            tr = DeviceParticleTracker(trans, s, om, ParticleTrackerBuilder.Parameters(evaluation_count=n), device_rng=True, seed=3)
            tr.initialize([init])
            errs = []
            for k in range(1, n_frames - tail):
                tr.track(frames[k])
            t0 = time.perf_counter()
            for k in range(n_frames - tail, n_frames):
                est = tr.track(frames[k])
                errs.append(float(np.linalg.norm(est[0:3] - (truths[k][0, 9:12] - truths[k][0, :9].reshape(3, 3) @ om.centers[0]))))
            el = time.perf_counter() - t0
            w = np.array([s.get_window(q) for q in range(0, n, max(1, n // 64))])
            fr = float(np.mean(np.maximum(0, w[:, 2] - w[:, 0]) * np.maximum(0, w[:, 3] - w[:, 1]))) / (s.rows * s.cols)
            active, rebases = s.shared_trail_state()
            tr.close()
    finally:
        if old_env is None:
            os.environ.pop("RBS_SHARED_TRAIL", None)
        else:
            os.environ["RBS_SHARED_TRAIL"] = old_env
    return {"fps": tail / el, "value": n * tail / el, "window_fraction": fr, "position_error_max_m": max(errs), "rebasings": rebases}


def sweep_leg(a, dev, stream, n_frames=1000, tail=200, table=(0.03, 0.10, 0.25, 0.50)):
    """What the windowed state layout sustains when the object MOVES ACROSS THE IMAGE: a pixel stays in a
    particle's window until its occlusion value has relaxed to within 2^-18 of the background, ~730 frames (24 s) after the
    object left it, and a window is ONE bounding box of everything an ancestor touched in that time.  C1 (2 000 particles, M1,
    640x480, update=true, permutation parents) with the object travelling along the image diagonal and back at 2 mm per frame
    for n_frames frames; `sweep_value` = the rate over the LAST `tail` frames (every window then holds a 24 s trail),
    `sweep_window_fraction` = the mean stored fraction of a plane at the end.  And a table: the same C1 step with every plane's
    window pre-filled to a given fraction of the frame (window_fraction_table: fraction -> particle-likelihoods/s)."""
    import copy
    from dbot_ros_amd import RbSensor, synth
    b = copy.copy(a)
    for k, v in PRESETS["c1"].items():
        setattr(b, k, v)
    om, cam, P, n_tri, nb = build_scene(b)
    n = b.particles
    res = {}
    rng = np.random.default_rng(7)
    prng = np.random.default_rng(8)
    truths = sweep_truths(n_frames)
    with RbSensor(om, cam, P, device_id=dev.index, max_particles=1) as r:
        frames = np.stack([synth.make_frame(r.render_depth(t), b.rows, b.cols, rng) for t in truths]).astype(np.float32)
    # the particles of a tracker that follows the object: a cloud around the truth, one fixed set of offsets (the transition's spread)
    base = synth.particle_poses(truths[0], n, prng).reshape(n, -1)
    off = base[:, 9:12] - truths[0][0, 9:12]
    d_frames = torch.from_numpy(frames).to(dev)
    poses = np.repeat(base[None], 2, axis=0)         # two staging copies, rewritten on the device per frame
    d_base = torch.from_numpy(base).to(dev)
    d_pose = d_base.clone()
    d_off = torch.from_numpy(off).to(dev)
    d_t = torch.from_numpy(np.stack([t[0, 9:12] for t in truths])).to(dev)
    d_idx = torch.from_numpy(synth.resample_like_indices(n, prng)).to(dev)
    d_out = torch.empty(n, dtype=torch.float64, device=dev)
    del poses
    frame_bytes = d_frames[0].numel() * 4
    with make_sensor(b, om, cam, P, dev) as s:
        s.reset()
        s.set_observation(frames[0])
        s.synchronize()

        def step(k):
            d_pose[:, 9:12] = d_t[k] + d_off         # (two tiny torch kernels on the same stream: inside the clock)
            s.set_observation_device(d_frames.data_ptr() + k * frame_bytes, stream.cuda_stream)
            s.loglikes_device(d_pose.data_ptr(), d_idx.data_ptr(), n, True, d_out.data_ptr(), stream.cuda_stream)

        marks = {}
        for k in range(n_frames - tail):
            step(k)
            if k in (30, 100, 300):
                torch.cuda.synchronize()
                w = np.array([s.get_window(q) for q in range(0, n, max(1, n // 32))])
                marks[k] = float(np.mean(np.maximum(0, w[:, 2] - w[:, 0]) * np.maximum(0, w[:, 3] - w[:, 1]))) / (b.rows * b.cols)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(n_frames - tail, n_frames):
            step(k)
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        ok = bool(np.isfinite(d_out.cpu().numpy()).all())
        w = np.array([s.get_window(q) for q in range(0, n, max(1, n // 64))])
        frac = float(np.mean(np.maximum(0, w[:, 2] - w[:, 0]) * np.maximum(0, w[:, 3] - w[:, 1]))) / (b.rows * b.cols)
    res.update({"sweep_value": n * tail / el if ok else None, "sweep_ms_per_step": el / tail * 1e3, "sweep_window_fraction": frac,
                "sweep_window_fraction_after_frames": {str(k): v for k, v in marks.items()},
                "sweep_note": (f"C1 with the object travelling along the image diagonal and back at 2 mm/frame, {n_frames} frames, particles following it; "
                               f"rate over the last {tail} frames (windows hold the ~730-frame trail the 2^-18 snap leaves), stored fraction of a plane "
                               "at the end; inputs resident in HBM.  The headline's object oscillates over 6 cm (window 3 % of the plane)")})
    # ---- the same sweep under the DEVICE TRACKER (rbs_tracker_*: transition, KL-triggered multinomial resampling, mean): the
    # filter's own genealogy -- children share parents, so the trail is common to the particles -- with the shared background
    # plane (the library's default once windows have grown) and without it (RBS_SHARED_TRAIL=0)
    try:
        for tag, env in (("sweep_tracker", True), ("sweep_tracker_scalar_background", False)):
            r_ = sweep_tracker_run(lambda: make_sensor(b, om, cam, P, dev), om, frames, truths, n, tail, env)
            res.update({tag + "_" + k_: v_ for k_, v_ in r_.items()})
        res["sweep_tracker_note"] = ("the same travelling object followed by the device tracker (%d particles, frame by frame from host memory, "
                                     "its own KL-triggered resampling): frames/s and particle-likelihoods/s over the last %d of %d frames, stored window "
                                     "fraction at the end; sweep_tracker_*: planes stored against the shared background plane once windows have grown "
                                     "(the default), sweep_tracker_scalar_background_*: RBS_SHARED_TRAIL=0" % (n, tail, n_frames))
    except Exception as e:   # noqa: BLE001
        res["sweep_tracker_note"] = f"tracker sweep failed: {e!r}"
    del d_frames
    torch.cuda.empty_cache()
    # ---- window fraction -> rate: the headline's own step with every plane's window pre-filled
    tab = {}
    old_env = os.environ.get("RBS_SHARED_TRAIL")
    os.environ["RBS_SHARED_TRAIL"] = "0"      # (identical pre-filled blocks are a trail every particle shares: the shared plane would store them once)
    for f in table:
        c = copy.copy(b)
        c.fill_planes, c.fill_fraction = 0.9, f
        W = Workload(c, om, cam, P, nb, dev, 0)
        s = make_sensor(c, om, cam, P, dev)
        prime(s, c, W)
        run = ResidentRun(c, W, s, stream, d_out)
        run.timed(48, 0)                      # the handle samples the stored area every 8th call and picks its launch shape from it
        el = run.timed(100, 0)
        w = np.array([s.get_window(q) for q in range(0, n, max(1, n // 64))])
        got = float(np.mean(np.maximum(0, w[:, 2] - w[:, 0]) * np.maximum(0, w[:, 3] - w[:, 1]))) / (b.rows * b.cols)
        s.close()
        tab[f"{f:.2f}"] = {"value": n * 100 / el, "ms_per_step": el / 100 * 1e3, "stored_fraction_measured": got}
        del W
        torch.cuda.empty_cache()
    if old_env is None:
        os.environ.pop("RBS_SHARED_TRAIL", None)
    else:
        os.environ["RBS_SHARED_TRAIL"] = old_env
    res["window_fraction_table"] = tab
    res["window_fraction_table_note"] = ("what a stored window of that size COSTS (scalar background, RBS_SHARED_TRAIL=0): C1's step with every plane's window "
                                         "pre-filled to that fraction of the frame (a centred block of values that differ from the background): above 15 % "
                                         "the raster kernel runs two blocks per CU, above 50 % the call takes the whole-plane machinery.  With the shared "
                                         "background plane (the default) identical blocks are stored once and every row of this table is the headline's rate")
    return res


# --------------------------------------------------------------------------------- PMC child passes
def pmc_pass(a, counters, layout, timeout=150):
    """One rocprofv3 --pmc pass over a short child run of this same command (same workload
    flags).  Returns {kernel short name: {counter: mean value per dispatch}} or None."""
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        return None
    out = tempfile.mkdtemp(prefix="rbs_pmc_", dir="/tmp")
    flags = []
    for f in WORKLOAD_FLAGS:
        v = layout if f == "layout" else getattr(a, f)
        flags += ["--" + f.replace("_", "-"), str(v)]
    cmd = [exe, "--pmc", *counters, "--kernel-trace", "--output-format", "csv", "-d", out, "-o", "pmc", "--",
           sys.executable, os.path.abspath(__file__), "--pmc-child", "--steps", "12", "--warmup", "3", *flags]
    env = dict(os.environ, TMPDIR="/tmp")
    try:
        subprocess.run(cmd, cwd="/tmp", env=env, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=timeout, check=True)
        files = glob.glob(os.path.join(out, "**", "*counter_collection.csv"), recursive=True)
        acc = {}
        for f in files:
            for row in csv.DictReader(open(f)):
                name = row["Kernel_Name"]
                short = next((k for k in ("rbs_raster_kernel", "rbs_copy_window_kernel", "rbs_copy_rows_kernel",
                                          "rbs_frame_prep_kernel", "rbs_prep_kernel", "rbs_wide_window_kernel") if k in name), None)
                if short is None:
                    continue
                d = acc.setdefault(short, {}).setdefault(row["Counter_Name"], {})
                d[row["Dispatch_Id"]] = d.get(row["Dispatch_Id"], 0.0) + float(row["Counter_Value"])
        res = {}
        for k, cs in acc.items():
            res[k] = {}
            for c, per in cs.items():
                v = [per[d] for d in sorted(per, key=int)]
                v = v[len(v) // 4:]            # drop the warm-up dispatches
                res[k][c] = float(np.mean(v))
        return res or None
    except Exception as e:                     # noqa: BLE001 -- the bench must survive a box without counters
        print(f"# pmc pass {counters} failed: {e}", file=sys.stderr)
        return None
    finally:
        shutil.rmtree(out, ignore_errors=True)


def hbm_bytes(fetch, write, kernel):
    """FETCH_SIZE / WRITE_SIZE are KiB; gfx950's FETCH_SIZE reports half the bytes of wide
    coalesced reads (MI355X_MICROARCH.md, HBM section; calibrated on a float4 stream copy in
    profiles/r01_pmc_hbm.json: x1.99995 and x0.99996)."""
    if not fetch or not write or kernel not in fetch or kernel not in write:
        return None
    return fetch[kernel].get("FETCH_SIZE", 0.0) * 1024.0 * 2.0 + write[kernel].get("WRITE_SIZE", 0.0) * 1024.0


def roofline_for(a, n, raster_ms, copy_ms, alg_bytes, copy_dominant, live):
    """The `roofline` object of the dominant kernel of one device's launch of n particles: live
    rocprofv3 counter passes of this same command (child processes), the committed summary as a
    fall-back.  Windowed planes: the raster kernel, bound by VALU issue -- priced against the
    MEASURED issue ceiling of its own instruction mix (binary64 / binary64 transcendental / other:
    VALU_PEAK_* above), with the busy fraction of the SIMDs and the instruction count per unit of
    work beside it, so that neither padding nor a cheaper mix can pass for progress.  Whole planes:
    the copy kernel, bound by HBM."""
    sq = mix = fetch = write = None
    if live:
        sq = pmc_pass(a, ["SQ_INSTS_VALU", "SQ_ACTIVE_INST_VALU", "SQ_WAVE_CYCLES", "SQ_WAIT_ANY", "SQ_INSTS_SALU", "SQ_WAVES"], a.layout)
        mix = pmc_pass(a, ["SQ_INSTS_VALU_FMA_F64", "SQ_INSTS_VALU_MUL_F64", "SQ_INSTS_VALU_ADD_F64", "SQ_INSTS_VALU_TRANS_F64"], a.layout)
        fetch = pmc_pass(a, ["FETCH_SIZE"], a.layout)
        write = pmc_pass(a, ["WRITE_SIZE"], a.layout)
    pmc_live = sq is not None and "rbs_raster_kernel" in sq
    if not pmc_live:               # a box without counters: the committed summary of this command
        try:
            j = json.load(open(os.path.join(ROOT, "profiles", "r04_raster_sq.json")))
            if j.get("precision") == a.precision and j.get("state_layout") == a.layout:
                sq = {"rbs_raster_kernel": j["per_dispatch"]}
                mix = sq
        except Exception:           # noqa: BLE001
            sq = None
    rsq = (sq or {}).get("rbs_raster_kernel", {})
    rmix = (mix or {}).get("rbs_raster_kernel", {})
    valu = rsq.get("SQ_INSTS_VALU")
    raster_traffic = hbm_bytes(fetch, write, "rbs_raster_kernel")
    copy_kernel = "rbs_copy_window_kernel" if a.layout == "window" else "rbs_copy_rows_kernel"
    copy_traffic = hbm_bytes(fetch, write, copy_kernel)
    if copy_dominant:
        achieved = alg_bytes / (copy_ms * 1e-3) / 1e9
        roof = {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBPS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBPS,
                "traffic": copy_traffic, "kernel": copy_kernel, "kernel_ms": copy_ms}
    else:
        ginst = (valu / (raster_ms * 1e-3) / 1e9) if valu else None
        peak = frac = f64_share = peak_guide = n64 = ntr = None
        if valu and "SQ_INSTS_VALU_FMA_F64" in rmix:
            n64 = rmix["SQ_INSTS_VALU_FMA_F64"] + rmix.get("SQ_INSTS_VALU_MUL_F64", 0.0) + rmix.get("SQ_INSTS_VALU_ADD_F64", 0.0)
            ntr = rmix.get("SQ_INSTS_VALU_TRANS_F64", 0.0)
            rest = max(0.0, valu - n64 - ntr)
            t_min = (n64 / VALU_PEAK_F64_GINST + ntr / VALU_PEAK_TRANS_F64_GINST + rest / VALU_PEAK_F32_GINST) / 1e9   # s: nothing but issue
            peak = valu / t_min / 1e9
            frac = ginst / peak
            t_guide = (n64 / GUIDE_PEAK_F64_GINST + ntr / GUIDE_PEAK_TRANS_F64_GINST + rest / GUIDE_PEAK_F32_GINST) / 1e9
            peak_guide = valu / t_guide / 1e9
            f64_share = (n64 + ntr) / valu
        frac_guide = (ginst / peak_guide) if (ginst and peak_guide) else None
        roof = {"bound": "valu_issue", "achieved": ginst, "peak": peak_guide, "unit": "G wave-instructions/s", "frac": frac_guide,
                "peak_note": "issue ceiling of THIS kernel's instruction mix at the GUIDE's issue costs: 2 cycles float32 / integer, 4 binary64, "
                             "16 binary64 transcendental, wave64 at 2.4 GHz x 1 024 SIMDs (MI355X_MICROARCH.md)",
                "peak_measured_ceiling": peak, "frac_vs_measured_ceiling": frac,
                "peak_measured_ceiling_note": "the same mix at the MEASURED saturated per-class rates (binary64 590, binary64 transcendental 151, other "
                                              "1 020 G wave-instructions/s: profiles/r04_valu_issue_microbench.txt)",
                "frac_vs_guide_peak": frac_guide,
                "algorithmic_bytes_note": "SURVEY 8(d)'s HBM figure does not bound this kernel: algorithmic bytes (2 x 4 x W x H per particle-likelihood) / "
                                          "kernel time is several times the 8 TB/s peak (algorithmic_equiv_GBps) because a plane is stored as a WINDOW -- the "
                                          "call moves ~5 % of those bytes (traffic) and is bound by VALU issue; where the bytes really move the copy kernel "
                                          "is priced against HBM: dense_hbm_frac (whole planes) and sweep_hbm_frac (windows grown to most of the frame)",
                "valu_instr_f64": (n64 if valu and "SQ_INSTS_VALU_FMA_F64" in rmix else None),
                "valu_instr_trans_f64": (ntr if valu and "SQ_INSTS_VALU_FMA_F64" in rmix else None),
                "traffic": raster_traffic, "kernel": "rbs_raster_kernel", "kernel_ms": raster_ms,
                "f64_share_of_valu_instructions": f64_share,
                "valu_wave_instructions_per_launch": valu,
                "valu_instr_per_particle_likelihood": (valu / n) if valu else None,
                "valu_busy_frac": (rsq["SQ_ACTIVE_INST_VALU"] * 4.0 / 1024.0 / (raster_ms * 1e-3 * 2.4e9)) if rsq.get("SQ_ACTIVE_INST_VALU") else None,
                "valu_busy_note": "SQ_ACTIVE_INST_VALU quad-cycles x 4 / (1 024 SIMDs x kernel time x 2.4 GHz): share of SIMD time with a VALU instruction in flight",
                "wave_time_waiting_frac": (rsq["SQ_WAIT_ANY"] / rsq["SQ_WAVE_CYCLES"]) if rsq.get("SQ_WAVE_CYCLES") else None,
                "hbm_actual_GBps": (raster_traffic / (raster_ms * 1e-3) / 1e9) if raster_traffic else None,
                "hbm_actual_frac": (raster_traffic / (raster_ms * 1e-3) / 1e9 / HBM_PEAK_GBPS) if raster_traffic else None,
                "algorithmic_equiv_GBps": alg_bytes / (raster_ms * 1e-3) / 1e9}
    return roof, pmc_live, copy_traffic


# --------------------------------------------------------------------------------- CPU baseline
def usable_cores():
    """CPUs this process may actually use: the affinity mask, capped by the cgroup's CPU quota
    (cpu.max).  On the GPU boxes of this pool the host reports 256 hardware threads but the
    container's quota is 16 CPUs: a thread team sized by os.cpu_count() spends its time being
    throttled (round 1's 'all cores' figure was slower than one thread for that reason)."""
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    quota = None
    for path in ("/sys/fs/cgroup/cpu.max",):
        try:
            q, period = open(path).read().split()[:2]
            if q != "max":
                quota = float(q) / float(period)
        except (OSError, ValueError):
            pass
    if quota is None:
        try:
            q = float(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            period = float(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0:
                quota = q / period
        except (OSError, ValueError):
            pass
    if quota is not None:
        n = max(1, min(n, int(quota)))
    return n, quota


def cpu_baseline(om, cam, P, truth, frame, seconds):
    """The oracle in reference-CPU-semantics mode (LAZY) on a bounded sample of the same
    workload.  Headline = single thread, config C0's 200 particles per call, as dbot's CPU model
    runs; all_cores = C1's 2 000 particles per call with OpenMP over particles on every host core
    (persistent thread team, per-thread scratch kept, every slot first touched by the thread that
    evaluates it)."""
    os.environ.setdefault("OMP_PROC_BIND", "false")    # a quota-limited container: let the scheduler place the team
    os.environ.setdefault("OMP_WAIT_POLICY", "passive")
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_binding as ob
    from dbot_ros_amd import synth
    tris = sum(len(t) for t in om.triangles)

    def run(n, threads, budget):
        orc = ob.Oracle(om, cam, P, max_particles=n, mode=ob.LAZY)
        rng = np.random.default_rng(1)
        poses = synth.particle_poses(truth, n, rng)
        idx = np.zeros(n, dtype=np.int32)
        orc.reset(threads=threads)
        if threads > 1:                      # thread team + scratch: set-up, not the baseline
            orc.set_observation(frame)
            orc.loglikes_poses(poses, idx, update=True, threads=threads)
        done, t0 = 0, time.perf_counter()
        while True:
            orc.set_observation(frame)
            orc.loglikes_poses(poses, idx, update=True, threads=threads)
            done += n
            idx = rng.permutation(n).astype(np.int32)
            el = time.perf_counter() - t0
            if el >= budget:
                break
        orc.close()
        return done, el

    n1 = 200
    done, el = run(n1, 1, seconds)
    cores = os.cpu_count() or 1
    usable, quota = usable_cores()
    model = "unknown CPU"
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                model = line.split(":", 1)[1].strip()
                break
    except OSError:
        pass
    out = {"value": done / el, "unit": "particle-likelihoods/s", "cores": 1, "kind": "port", "host_cpu": model, "host_cores": cores,
           "sample": f"{done} particle-likelihoods = {done // n1} loglikes(update=true) calls x {n1} "
                     f"particles, {cam.cols}x{cam.rows}, {tris} triangles, {el:.1f} s on 1 of {cores} host cores"}
    out["usable_cores"] = usable
    out["cgroup_cpu_quota"] = quota
    if usable > 1:
        nm = 2000
        threads = min(usable, nm)
        done_mt, el_mt = run(nm, threads, max(3.0, seconds / 3))
        out["all_cores_value"] = done_mt / el_mt
        out["all_cores_threads"] = threads
        out["all_cores_speedup"] = (done_mt / el_mt) / (done / el)
        out["all_cores_sample"] = (f"{done_mt} particle-likelihoods = {done_mt // nm} calls x {nm} particles in {el_mt:.1f} s, "
                                   f"OpenMP over particles, {threads} threads = every CPU this container may use "
                                   f"({cores} hardware threads on the host" + (f", cgroup quota {quota:g} CPUs)" if quota else ")"))
        if out["all_cores_speedup"] < 0.5 * threads and out["all_cores_speedup"] < 10.0:
            out["all_cores_note"] = "below half-linear scaling: the host is shared with other tenants (see /proc/loadavg)"
    return out


# --------------------------------------------------------------------------------- host API from C++
def write_host_workload(f, om, cam, P, frames, poses, parents, update, init=None):
    """The binary workload tests/cpp/host_bench.cpp reads (layout in its header comment)."""
    import struct
    frames = np.ascontiguousarray(frames, dtype=np.float32)
    poses = np.ascontiguousarray(poses, dtype=np.float64)
    n, F = poses.shape[1], frames.shape[0]
    f.write(struct.pack("6i", cam.rows, cam.cols, om.count_parts, n, F, int(update)))
    f.write(np.ascontiguousarray(cam.camera_matrix, dtype=np.float64).tobytes())
    f.write(struct.pack("7d", P.occlusion.p_occluded_visible, P.occlusion.p_occluded_occluded,
                        P.occlusion.initial_occlusion_prob, P.kinect.tail_weight, P.kinect.model_sigma,
                        P.kinect.sigma_factor, P.delta_time))
    for v, t in zip(om.vertices, om.triangles):
        v = np.ascontiguousarray(v, dtype=np.float64)
        t = np.ascontiguousarray(t, dtype=np.int32)
        f.write(struct.pack("2i", len(v), len(t)))
        f.write(v.tobytes())
        f.write(t.tobytes())
    f.write(frames.tobytes())
    f.write(poses.tobytes())
    f.write(np.ascontiguousarray(parents, dtype=np.int32).tobytes())
    if init is not None:
        f.write(np.ascontiguousarray(init, dtype=np.float64).tobytes())


def native_host_leg(a, om, cam, P, W, steps):
    """Write the workload where tests/cpp/host_bench can read it and run that binary (built by
    __graft_entry__.build()).  Returns {} when the binary is missing."""
    import subprocess
    import tempfile
    exe = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tests", "cpp", "host_bench")
    if not os.path.exists(exe):
        return {}
    with tempfile.NamedTemporaryFile(suffix=".bin", delete=False) as f:
        path = f.name
        write_host_workload(f, om, cam, P, W.frames, W.poses, W.parents, bool(a.update))
    try:
        env = dict(os.environ, RBS_PRECISION=a.precision, RBS_STATE=a.layout)
        r = subprocess.run([exe, path, str(steps), "10"], capture_output=True, text=True, timeout=300, env=env)
        line = next((l for l in r.stdout.splitlines() if l.startswith("host_bench ")), None)
        if not line:
            return {"host_api_native_note": "host_bench did not run: " + (r.stdout + r.stderr)[-200:]}
        tok = line.split()
        res = {"host_api_native_value": float(tok[2]), "host_api_native_ms_per_step": float(tok[4]),
               "host_api_native_note": "the host-pointer step (rbs_set_observation_f32 + rbs_loglikes, synchronous) called from C++ "
                                       "(tests/cpp/host_bench.cpp), frames cycling forwards through the sequence"}
        rb = subprocess.run([exe, "--borrowed", path, str(steps), "10"], capture_output=True, text=True, timeout=300, env=env)
        lineb = next((l for l in rb.stdout.splitlines() if l.startswith("host_bench ")), None)
        if lineb:
            tb = lineb.split()
            res.update({"host_api_native_borrowed_value": float(tb[2]), "host_api_native_borrowed_ms_per_step": float(tb[4]),
                        "host_api_native_borrowed_checksum_equal": tb[6] == tok[6] if len(tb) > 6 and len(tok) > 6 else None,
                        "host_api_native_borrowed_note": "the same synchronous step with the frame BORROWED until rbs_loglikes returns (rbs_set_observation_borrowed_f32): "
                                                         "staged behind the geometry kernel of the two-kernel launch"})
        rl = subprocess.run([exe, "--loglikes-only", path, str(steps), "10"], capture_output=True, text=True, timeout=300, env=env)
        linel = next((l for l in rl.stdout.splitlines() if l.startswith("host_bench ")), None)
        if linel:
            tl_ = linel.split()
            res.update({"host_api_native_loglikes_only_value": float(tl_[2]), "host_api_native_loglikes_only_ms_per_step": float(tl_[4]),
                        "host_api_native_loglikes_only_note": "SURVEY 8(d)'s metric to the letter from C++: rbs_loglikes alone, synchronous -- poses and parent slots from host "
                                                              "memory, log-likelihoods back to host memory, the frame resident (host_api_loglikes_only_value: the same through ctypes)"})
        r2 = subprocess.run([exe, "--prefetch", path, str(steps), "10"], capture_output=True, text=True, timeout=300, env=env)
        line2 = next((l for l in r2.stdout.splitlines() if l.startswith("host_bench ")), None)
        if line2:
            t2 = line2.split()
            res.update({"host_api_native_prefetch_value": float(t2[2]), "host_api_native_prefetch_ms_per_step": float(t2[4]),
                        "host_api_native_prefetch_checksum_equal": t2[6] == tok[6] if len(t2) > 6 and len(tok) > 6 else None})
        # ... and THROUGH THE PLUGIN SURFACE the reference drives: dbot_amd::RbSensor::set_observation(image of
        # DOUBLES) + loglikes(state deltas, one heap vector per particle; indices; update), synchronous, no look-ahead
        for tag, mode in (("plugin_api", "--plugin-copy"), ("plugin_api_borrowed", "--plugin")):
            r3 = subprocess.run([exe, mode, path, str(steps), "10"], capture_output=True, text=True, timeout=300, env=env)
            line3 = next((l for l in r3.stdout.splitlines() if l.startswith("host_bench ")), None)
            if line3:
                t3 = line3.split()
                res.update({tag + "_value": float(t3[2]), tag + "_ms_per_step": float(t3[4])})
                if len(t3) > 6 and len(tok) > 6:
                    res[tag + "_checksum_rel_diff"] = abs(float(t3[6]) - float(tok[6])) / max(1.0, abs(float(tok[6])))
            else:
                res[tag + "_note"] = "host_bench --plugin did not run: " + (r3.stdout + r3.stderr)[-200:]
        res["plugin_api_note"] = ("through the plugin surface, from C++ (tests/cpp/host_bench.cpp --plugin): dbot_amd::RbSensorBuilder(...).build(), then per step "
                                  "set_observation(rows*cols doubles) + loglikes(deltas: one State per particle, indices, update) -- the frame's double -> float "
                                  "staging, the gather of the deltas and the pose composition (on the device: rbs_loglikes_deltas) inside the clock; synchronous, "
                                  "no look-ahead.  plugin_api_*: set_observation copies at once, as dbot's own sensors do (the mirror's and the dbot binding's "
                                  "DEFAULT, one-kernel launch).  plugin_api_borrowed_*: Options::borrow_frames -- the image is BORROWED until loglikes returns "
                                  "(safe when it outlives the pair inside tracker_->track(image)): loglikes stages it while its geometry kernel runs "
                                  "(rbs_set_observation_borrowed, two-kernel launch)")
        return res
    except Exception as e:   # noqa: BLE001 -- a benchmark leg must not take the headline down
        return {"host_api_native_note": "host_bench failed: %r" % (e,)}
    finally:
        os.unlink(path)


def native_tracker_leg(om, cam, P, frames, init, counts, precision):
    """The device tracker driven from C++ (tests/cpp/host_bench --tracker): what the reference's own
    node, which is C++, would see -- no interpreter between the frames.  {} when the binary is missing."""
    import subprocess
    import tempfile
    exe = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tests", "cpp", "host_bench")
    if not os.path.exists(exe):
        return {}
    nb = om.count_parts
    with tempfile.NamedTemporaryFile(suffix=".bin", delete=False) as f:
        path = f.name
        write_host_workload(f, om, cam, P, np.stack(frames), np.zeros((len(frames), 1, 12 * nb)), np.zeros(1, np.int32), True, init=init)
    out = {}
    try:
        env = dict(os.environ, RBS_PRECISION=precision)
        for n in counts:      # ... and through the mirror of the reference's builders, the images as doubles (plugin_tracker_fps_*)
            rp = subprocess.run([exe, "--tracker-plugin", path, str(n)], capture_output=True, text=True, timeout=300, env=env)
            lp = next((l for l in rp.stdout.splitlines() if l.startswith("tracker_bench ")), None)
            if lp:
                tk = lp.split()
                out[f"plugin_tracker_fps_{n}"] = float(tk[4])
                out[f"plugin_tracker_fps_pipelined_{n}"] = float(tk[6])
        out["plugin_tracker_fps_note"] = ("the device tracker through dbot_amd::ParticleTrackerBuilder(...).build(): tracker->track(image of rows*cols DOUBLES) frame by "
                                          "frame / submit + result with one frame of look-ahead (tests/cpp/host_bench.cpp --tracker-plugin)")
        for n in counts:
            r = subprocess.run([exe, "--tracker", path, str(n)], capture_output=True, text=True, timeout=300, env=env)
            line = next((l for l in r.stdout.splitlines() if l.startswith("tracker_bench ")), None)
            if not line:
                out["tracker_fps_native_note"] = "host_bench --tracker did not run: " + (r.stdout + r.stderr)[-200:]
                break
            tok = line.split()
            out[f"tracker_fps_native_{n}"] = float(tok[4])
            out[f"tracker_fps_native_pipelined_{n}"] = float(tok[6])
        else:
            out["tracker_fps_native_note"] = ("the same device tracker and frames driven from C++ through the C-ABI (tests/cpp/host_bench.cpp --tracker): "
                                              "rbs_tracker_track frame by frame / rbs_tracker_submit + rbs_tracker_result with one frame of look-ahead")
    except Exception as e:   # noqa: BLE001 -- a benchmark leg must not take the headline down
        out["tracker_fps_native_note"] = "host_bench --tracker failed: %r" % (e,)
    finally:
        os.unlink(path)
    return out


# --------------------------------------------------------------------------------- tracker FPS
def tracker_fps(om, cam, device, counts=(200, 2000, 20000), n_frames=30, precision=None, device_ids=None, occlusion=None):
    """Frames/s of the device tracker (rbs_tracker_*: transition, weights, KL, resampling and mean
    on the GPU, device RNG, one host sync per frame; the frame is uploaded from host memory every
    frame) on the 30-frame sequence.  Second half of BASELINE.json's metric."""
    from dbot_ros_amd import RbSensor, RbSensorBuilder, pose, synth
    from dbot_ros_amd.tracker import DeviceParticleTracker, ObjectTransitionBuilder, ParticleTrackerBuilder
    nb = om.count_parts
    out = {}
    frames = None
    for n in counts:
        P = RbSensorBuilder.Parameters(sample_count=n)
        # device_ids: the tracker SHARDED over several devices inside one handle (all states on every device, the sensor
        # call split, one RCCL all-gather of the log-likelihoods per sampling block)
        with RbSensor(om, cam, P, device_id=device.index, max_particles=max(1, n // nb), precision=precision, device_ids=device_ids,
                      occlusion=occlusion) as s:
            if frames is None:
                rng = np.random.default_rng(0)
                frames = [synth.make_frame(s.render_depth(synth.truth_pose(nb, frame=k)), cam.rows, cam.cols, rng,
                                           occluder=False).astype(np.float32) for k in range(n_frames + 1)]
            trans = ObjectTransitionBuilder(ObjectTransitionBuilder.Parameters(part_count=nb)).build()
            tr = DeviceParticleTracker(trans, s, om, ParticleTrackerBuilder.Parameters(evaluation_count=n), device_rng=True, seed=1)
            init = np.zeros(12 * nb)
            for b in range(nb):
                Rt = synth.truth_pose(nb, frame=0)[b]
                init[12 * b + 3:12 * b + 6] = pose.matrix_to_rotvec(Rt[:9].reshape(3, 3))
                init[12 * b:12 * b + 3] = Rt[9:] - Rt[:9].reshape(3, 3) @ om.centers[b]
            out["_native"] = (frames, init.copy())
            # the median of three passes over the sequence (a pass is 6 ms at 200 particles: one pass alone
            # moved by 25 % with whatever else the host was doing)
            dts = []
            for _rep in range(3):
                tr.initialize([init])
                tr.track(frames[0])  # warm-up
                t0 = time.perf_counter()
                for k in range(1, n_frames + 1):
                    est = tr.track(frames[k])
                dts.append(time.perf_counter() - t0)
            dt = float(np.median(dts))
            Rt = synth.truth_pose(nb, frame=n_frames)[0]
            err = float(np.linalg.norm(est[0:3] - (Rt[9:] - Rt[:9].reshape(3, 3) @ om.centers[0])))
            out[n] = {"fps": n_frames / dt, "ms_per_frame": dt / n_frames * 1e3, "resamplings": tr.n_resamplings,
                      "final_position_error_m": err}
            # the same sequence with one frame of look-ahead (rbs_tracker_submit / _result): frame k+1's
            # host copy and upload run beside frame k's kernels -- dataset replay, or a camera
            # ahead of its consumer
            dts = []
            for _rep in range(3):
                tr.initialize([init])
                tr.track(frames[0])
                t0 = time.perf_counter()
                tr.submit(frames[1])
                for k in range(2, n_frames + 1):
                    tr.submit(frames[k])
                    tr.result()
                est2 = tr.result()
                dts.append(time.perf_counter() - t0)
            dt = float(np.median(dts))
            out[n]["fps_pipelined"] = n_frames / dt
            out[n]["pipelined_equals_synchronous"] = bool(np.array_equal(est, est2))
            tr.close()
    return out


# --------------------------------------------------------------------------------- one process, several devices
def in_process_multi_device(a):
    """One handle over a.gpus devices (rbs_config.n_devices): the form a single-process
    particle_tracker node uses.  Weak scaling: a.particles per device."""
    from dbot_ros_amd import RbSensor, pose, synth
    from dbot_ros_amd.tracker import DeviceParticleTracker, ObjectTransitionBuilder, ParticleTrackerBuilder
    ids = [int(x) for x in a.device_ids.split(",")] if a.device_ids else list(range(a.gpus))
    if len(ids) != a.gpus:
        raise SystemExit("--device-ids must list --gpus ordinals")
    om, cam, P, n_tri, nb = build_scene(a)
    n = a.particles * a.gpus
    dev = torch.device("cuda", ids[0])
    torch.cuda.set_device(dev)
    a_one = argparse.Namespace(**vars(a))
    W = Workload(a_one, om, cam, P, nb, dev, 0)
    rng = np.random.default_rng(5)
    poses = np.stack([synth.particle_poses(t, n, rng).reshape(n, -1) for t in W.truths])
    parents = synth.resample_like_indices(n, rng)
    with RbSensor(om, cam, P, max_particles=n, precision=a.precision, state_layout=a.layout,
                  device_ids=ids if a.gpus > 1 else None, device_id=ids[0]) as g:
        g.reset()

        def step(i):
            k = W.order[i % len(W.order)]
            g.set_observation(W.frames[k])
            return g.loglikes_poses(poses[k], parents.copy(), update=bool(a.update))

        for i in range(max(a.warmup, MIN_WARMUP_STEPS)):
            step(i)
        region_ms = []
        for k_steps in region_steps(a.steps):
            t0 = time.perf_counter()
            for i in range(k_steps):
                ll = step(i)
            region_ms.append((time.perf_counter() - t0) / k_steps * 1e3)
        ms = float(np.median(region_ms))
        if not np.isfinite(ll).all():
            raise SystemExit("non-finite log-likelihoods in the timed run")
        if a.dump_outputs:             # the last timed step's log-likelihoods
            dump_outputs(a.dump_outputs, {"loglikes": ll})
        if a.full:
            # the dominant kernel on the handle's first device (every device runs the same launch on its shard)
            g.set_timing_every(2)
            for i in range(64):
                step(i)
            g.synchronize()
            call_ms, copy_ms, n_used = g.timing_summary(64)
            raster_ms = g.raster_kernel_ms(64)
            g.set_timing_every(8)
            # the sharded device tracker on the same handle
            trans = ObjectTransitionBuilder(ObjectTransitionBuilder.Parameters(part_count=nb)).build()
            tr = DeviceParticleTracker(trans, g, om, ParticleTrackerBuilder.Parameters(evaluation_count=n * nb), device_rng=True, seed=1)
            init = np.zeros(12 * nb)
            for b in range(nb):
                Rt = W.truths[0][b]
                init[12 * b + 3:12 * b + 6] = pose.matrix_to_rotvec(Rt[:9].reshape(3, 3))
                init[12 * b:12 * b + 3] = Rt[9:] - Rt[:9].reshape(3, 3) @ om.centers[b]
            tr.initialize([init])
            tr.track(W.frames[0])
            nf = min(30, len(W.frames) - 1) or 1
            t0 = time.perf_counter()
            for k in range(1, nf + 1):
                tr.track(W.frames[k % len(W.frames)])
            fps = nf / (time.perf_counter() - t0)
            tr.close()
    line = {
        "metric": "particle-likelihoods/sec @640x480" if (a.cols, a.rows) == (640, 480) else f"particle-likelihoods/sec @{a.cols}x{a.rows}",
        "value": n / (ms * 1e-3), "unit": "particle-likelihoods/s", "n_gpus": a.gpus, "steps": a.steps, "warmup": a.warmup,
        "warmup_steps_run": max(a.warmup, MIN_WARMUP_STEPS), "ms_per_step": ms, "timed_regions": len(region_ms), "timed_regions_ms_per_step": region_ms,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "f64 geometry + f32 likelihood (precision F32, opt-in)" if a.precision == "f32" else "f64", "data": "synthetic",
        "config": {"workload": f"C1 x {a.gpus}: ONE process, one handle over devices {ids} (rbs_config.n_devices), {a.particles} particles per "
                               f"device, host-pointer API (frame + poses uploaded, log-likelihoods downloaded every step), "
                               f"{a.cols}x{a.rows}, mesh {a.mesh} ({n_tri} triangles), precision {a.precision}",
                   "particles_per_gpu": a.particles, "resolution": [a.cols, a.rows], "triangles": int(n_tri),
                   "sharding": f"particles/{a.gpus} inside the handle: peer reads of remote parents, RCCL all-gather in the tracker"},
    }
    if a.full:
        alg_bytes = (2.0 if a.update else 1.0) * 4.0 * a.rows * a.cols * a.particles     # per device launch, SURVEY 8d
        # whole planes: the copy kernel is the dominant one and HBM bound.  Windowed planes: the raster kernel
        # (the windowed copy kernel runs BESIDE it and moves ~1 % of the algorithmic bytes: pricing it with
        # them would report several times the HBM peak)
        copy_dominant = bool(a.update) and a.layout == "dense" and copy_ms > raster_ms
        roof, pmc_live, copy_traffic = roofline_for(a, a.particles, raster_ms, copy_ms, alg_bytes, copy_dominant, not a.no_pmc and not a.quick)
        roof.update({"counters_live": bool(pmc_live), "counters_note": "instruction counts from a single-device pass of the same per-device launch",
                     "kernel_launches_averaged": n_used, "raster_kernel_ms": raster_ms, "copy_kernel_ms": copy_ms,
                     "call_ms_launch_stream": call_ms, "per_device": True, "algorithmic_bytes_per_launch": alg_bytes})
        line.update({"tracker_fps_sharded": fps, "tracker_particles": n, "roofline": roof})
    if a.gpus == 1 and not a.no_cpu_baseline and not a.quick:
        line["cpu_baseline"] = cpu_baseline(om, cam, P, W.truths[0], W.frames[0], a.cpu_seconds)
    print(json.dumps(line), flush=True)


# --------------------------------------------------------------------------------- main
def sharded_tracker_child(a):
    """A process of its own (bench.py --gpus N under torch.distributed.run starts it from rank 0 with a time limit:
    a leg that hangs must not take the headline down): the device tracker over ONE handle on --device-ids."""
    om, cam, P, n_tri, nb = build_scene(a)
    ids = [int(x) for x in a.device_ids.split(",")]
    dev = torch.device("cuda", ids[0])
    torch.cuda.set_device(dev)
    # first the equality test of the in-handle form (one handle over the devices: peer reads between its shards, ncclCommInitAll
    # communicators for the tracker): 256 particles per device, three resampled steps, against a handle on the first device alone
    try:
        from dbot_ros_amd import RbSensor, synth
        n = 256 * len(ids)
        with RbSensor(om, cam, P, max_particles=1, device_id=ids[0], precision=a.precision) as r1:
            rng = np.random.default_rng(3)
            truths = [synth.truth_pose(nb, frame=k) for k in range(3)]
            frames = [synth.make_frame(r1.render_depth(t), cam.rows, cam.cols, rng) for t in truths]
        poses = [synth.particle_poses(t, n, rng, scale=2.0) for t in truths]
        parents = [np.sort(rng.integers(0, n, n)).astype(np.int32) for _ in truths]
        got = []
        for kw in ({"device_ids": ids}, {"device_id": ids[0]}):
            with RbSensor(om, cam, P, max_particles=n, precision=a.precision, **kw) as g:
                g.reset()
                idx, lls = np.zeros(n, np.int32), []
                for k in range(3):
                    g.set_observation(frames[k])
                    lls.append(g.loglikes_poses(poses[k], idx, update=True).copy())
                    idx = parents[k].copy()
                got.append(np.stack(lls))
        d = float(np.abs(got[0] - got[1]).max())
        print("IN_HANDLE_CHECK " + json.dumps({"in_handle_equals_single": bool(d <= 1e-12 * max(1.0, float(np.abs(got[1]).max()))),
                                               "in_handle_max_abs_loglik_diff": d, "in_handle_devices": ids}), flush=True)
    except Exception as e:   # noqa: BLE001
        print("IN_HANDLE_CHECK " + json.dumps({"in_handle_equals_single": False, "in_handle_check_diagnosis": repr(e)}), flush=True)
    fps = tracker_fps(om, cam, dev, precision=a.precision, device_ids=ids)
    fps.pop("_native", None)
    print("SHARDED_TRACKER " + json.dumps({str(k): {"fps": v["fps"], "fps_pipelined": v["fps_pipelined"]} for k, v in fps.items()}), flush=True)
    # the travelling object under the tracker sharded over the job's devices: the shared trail on a handle over several devices
    # (one decision per call for all shards, every device its own copy of the shared plane -- round 6)
    try:
        from dbot_ros_amd import RbSensor, RbSensorBuilder, synth
        n, n_frames, tail = 2000 * len(ids), 600, 150
        truths = sweep_truths(n_frames)
        rng = np.random.default_rng(7)
        Pn = RbSensorBuilder.Parameters(sample_count=n)
        with RbSensor(om, cam, Pn, device_id=ids[0], max_particles=1) as r:
            frames = np.stack([synth.make_frame(r.render_depth(t), cam.rows, cam.cols, rng) for t in truths]).astype(np.float32)
        out = {}
        for tag, env in (("sweep_tracker_sharded", True), ("sweep_tracker_sharded_scalar_background", False)):
            r_ = sweep_tracker_run(lambda: RbSensor(om, cam, Pn, max_particles=n, precision=a.precision, device_ids=ids), om, frames, truths, n, tail, env)
            out.update({tag + "_" + k_: v_ for k_, v_ in r_.items()})
        out["sweep_tracker_sharded_note"] = (f"the sweep legs' travelling object followed by the device tracker over ONE handle on devices {ids}, {n} particles, "
                                             f"rate over the last {tail} of {n_frames} frames; *_scalar_background_*: RBS_SHARED_TRAIL=0")
        print("SHARDED_SWEEP " + json.dumps(out), flush=True)
    except Exception as e:   # noqa: BLE001
        print("SHARDED_SWEEP " + json.dumps({"sweep_tracker_sharded_note": f"failed: {e!r}"}), flush=True)


def sharded_tracker_leg(a, ids, timeout=600):
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE", "GROUP_RANK", "ROLE_RANK", "MASTER_ADDR", "MASTER_PORT",
                        "TORCHELASTIC_RUN_ID", "TORCHELASTIC_RESTART_COUNT", "TORCHELASTIC_MAX_RESTARTS", "TORCHELASTIC_USE_AGENT_STORE")}
    cmd = [sys.executable, os.path.abspath(__file__), "--sharded-tracker-child", "--gpus", str(len(ids)), "--device-ids", ",".join(map(str, ids)),
           "--precision", a.precision]
    try:
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired:
        return {"in_handle_rccl_ok": False, "tracker_fps_sharded_note": f"sharded tracker leg did not finish within {timeout} s (stopped)"}
    chk = {}
    for line in r.stdout.splitlines():
        if line.startswith("IN_HANDLE_CHECK "):
            chk = json.loads(line[len("IN_HANDLE_CHECK "):])
    for line in r.stdout.splitlines():
        if line.startswith("SHARDED_TRACKER "):
            d = json.loads(line[len("SHARDED_TRACKER "):])
            out = dict(chk)
            out["in_handle_rccl_ok"] = True      # (the tracker's per-block all-gather ran on the handle's own communicators)
            for k_, v_ in d.items():
                out[f"tracker_fps_sharded_{k_}"] = v_["fps"]
                out[f"tracker_fps_sharded_pipelined_{k_}"] = v_["fps_pipelined"]
            out["tracker_fps_sharded_note"] = (f"rbs_tracker_* over one handle on devices {ids} (rbs_config.n_devices): every device holds all "
                                               "particle states, the sensor call is sharded, RCCL all-gather of the log-likelihoods per sampling "
                                               "block; frame uploaded from host memory every frame; a process of its own started by rank 0 while "
                                               "the ranks wait")
            for line2 in r.stdout.splitlines():
                if line2.startswith("SHARDED_SWEEP "):
                    out.update(json.loads(line2[len("SHARDED_SWEEP "):]))
            return out
    return dict(chk, in_handle_rccl_ok=False, tracker_fps_sharded_note="sharded tracker leg failed (rc %d): %s" % (r.returncode, (r.stderr or r.stdout)[-300:]))


class LineGuard:
    """--gpus N prints its ONE line whatever the first contact with a multi-GPU node does: the step with LOCAL
    parents + the all-gather is measured first and kept; everything that maps other processes' memory (rbs_ipc_attach has been
    seen never to return for some buffer sizes), the self-check and the legs run under a timer THREAD -- ctypes and the
    collectives release the interpreter lock while they block -- which on expiry prints the best complete line so far (rank 0)
    and ends the process with status 0 on every rank."""

    def __init__(self, rank):
        import threading
        self.rank, self.best, self.timer, self.why, self._threading = rank, None, None, "", threading

    def arm(self, seconds, why):
        self.disarm()
        self.why = why
        self.timer = self._threading.Timer(float(seconds), self._fire)
        self.timer.daemon = True
        self.timer.start()

    def disarm(self):
        if self.timer is not None:
            self.timer.cancel()
            self.timer = None

    def _fire(self):
        if self.rank == 0:
            line = dict(self.best) if self.best else {"metric": "particle-likelihoods/sec @640x480", "value": None, "unit": "particle-likelihoods/s"}
            line["peer_step"] = (f"attach_timeout: {self.why} did not finish in time; this line is what had been measured before it"
                                 + ("" if self.best else " (nothing: the first collective never returned)"))
            sys.stdout.write(json.dumps(line) + "\n")
            sys.stdout.flush()
        sys.stderr.write(f"# bench.py rank {self.rank}: watchdog -- {self.why} did not finish; leaving with the line measured before\n")
        sys.stderr.flush()
        os._exit(0)


def region_steps(steps):
    """--steps split into the headline's timed regions: as many as REPEATS allows with MIN_REGION_STEPS each, sizes within one."""
    r = max(1, min(REPEATS, steps // MIN_REGION_STEPS))
    return [steps // r + (1 if i < steps % r else 0) for i in range(r)]


def dump_outputs(path, arrays):
    """--dump-outputs: each array as path/<name>.npy (float64 stays float64, anything else float32); an array beyond its share of
    DUMP_BYTES is replaced by a fixed, seeded sample of its elements (same indices for the same size, run after run)."""
    os.makedirs(path, exist_ok=True)
    share = DUMP_BYTES // max(1, len(arrays))
    for name, x in arrays.items():
        x = np.asarray(x)
        x = np.ascontiguousarray(x, dtype=np.float64 if x.dtype == np.float64 else np.float32).ravel()
        if x.nbytes > share:
            keep = share // x.itemsize
            x = x[np.sort(np.random.default_rng(12345).choice(x.size, keep, replace=False))]
        np.save(os.path.join(path, name + ".npy"), x)


def headline(a, world, n, n_tri, region_ms, peer):
    """The contract's keys of the line; region_ms: ms per step of each timed region, the median of which is the line's ms_per_step
    (peer: 'ipc' = global parents over attached handles, 'local' = shards with local parents + the all-gather, None = one rank)."""
    ms = float(np.median(region_ms))
    out = {
        "metric": "particle-likelihoods/sec @640x480" if (a.cols, a.rows) == (640, 480)
                  else f"particle-likelihoods/sec @{a.cols}x{a.rows}",
        "value": n * world / (ms * 1e-3),
        "unit": "particle-likelihoods/s",
        "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
        "warmup_steps_run": max(a.warmup, MIN_WARMUP_STEPS), "ms_per_step": ms,
        "timed_regions": len(region_ms), "timed_regions_ms_per_step": list(region_ms),
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "f64 geometry + f32 likelihood (precision F32, opt-in)" if a.precision == "f32" else "f64",
        "data": "synthetic",
        "config": {"workload": f"C1: {n} particles/GPU x loglikes(update={'true' if a.update else 'false'}), {a.cols}x{a.rows} "
                               f"synthetic depth frame, mesh {a.mesh} ({n_tri} triangles), "
                               f"parents={a.parents}, " + (f"{max(1, a.sequence)}-frame moving-object sequence" if a.sequence > 0 else "one static frame")
                               + f", likelihood precision {a.precision}, {a.layout} planes"
                               + (f" in slabs of {a.slab_px} px" if a.slab_px else "") + ", inputs resident in HBM",
                   "particles_per_gpu": n, "resolution": [a.cols, a.rows], "triangles": int(n_tri),
                   "sharding": f"particles/{world}" + (" + RCCL all-gather of log-likelihoods" if world > 1 else "")},
    }
    if peer == "ipc":
        out["config"]["workload"] = (f"C1 per GPU: {n} particles/GPU ({n * world} in all) x [loglikes(update=true) with GLOBAL parents + RCCL all-gather of "
                                     f"the log-likelihoods + multinomial resampling over all ranks' particles (weights exp((ll - max) / {a.resample_temperature:g}))], "
                                     f"{a.cols}x{a.rows} synthetic depth frame, mesh {a.mesh} ({n_tri} triangles), {max(1, a.sequence)}-frame moving-object "
                                     f"sequence, likelihood precision {a.precision}, {a.layout} planes, inputs resident in HBM")
        out["config"]["sharding"] = (f"particles/{world}: one process per GPU, handles attached over HIP IPC (parents on other ranks read in place over "
                                     "xGMI, shared ones pulled once), one RCCL all-gather per step, resampling + plan in one library call "
                                     "(rbs_peer_resample), no plane migration, no host synchronisation")
    elif peer == "local":
        out["config"]["workload"] = (f"C1 per GPU: {n} particles/GPU ({n * world} in all) x [loglikes(update=true), parents on the rank's own GPU + "
                                     f"RCCL all-gather of the log-likelihoods]")
        out["config"]["sharding"] = f"particles/{world}: one process per GPU, local parents, one RCCL all-gather per step"
    return out


def main():
    t_main = time.perf_counter()
    if os.environ.get("RBS_BENCH_WATCHDOG"):    # diagnostics: dump every thread's stack and exit after that many seconds
        import faulthandler
        faulthandler.dump_traceback_later(int(os.environ["RBS_BENCH_WATCHDOG"]), exit=True)
    a = parse()
    if a.sharded_tracker_child:
        return sharded_tracker_child(a)
    if (a.gpus > 1 or a.in_process) and "WORLD_SIZE" not in os.environ and not a.pmc_child:
        if not torch.cuda.is_available():
            raise SystemExit("bench.py needs an MI355X: the HIP path is the only path (no CPU fallback)")
        return in_process_multi_device(a)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != a.gpus and world > 1:
        raise SystemExit(f"--gpus {a.gpus} but WORLD_SIZE={world}")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the HIP path is the only path (no CPU fallback)")
    # RBS_BENCH_BACKEND=gloo: functional test of the multi-rank path on a box with fewer GPUs than
    # ranks (ranks share devices, the all-gather goes through host tensors); never used for numbers
    backend = os.environ.get("RBS_BENCH_BACKEND", "nccl")
    if backend != "nccl":
        local = local % torch.cuda.device_count()
    torch.cuda.set_device(local)
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend)

    om, cam, P, n_tri, nb = build_scene(a)
    n = a.particles
    dev = torch.device("cuda", local)
    W = Workload(a, om, cam, P, nb, dev, rank)
    if rank == 0 and not a.pmc_child:
        print(f"# parents={a.parents}: {len(np.unique(W.parents))} distinct of {n}", file=sys.stderr)
    # a non-default torch stream: the kernels, the timing events and the RCCL all-gather all live
    # on it (a NULL stream would select the handle's private stream instead)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(stream)
    d_out = torch.empty(n, dtype=torch.float64, device=dev)
    d_all = torch.empty(n * world, dtype=torch.float64, device=dev) if world > 1 else None
    d_out.zero_()                  # first submission creates the stream's hardware queue: setup, not a step
    torch.cuda.synchronize()

    if a.sweep_only:
        print(json.dumps(sweep_leg(a, dev, stream), indent=1), flush=True)
        return
    peer_ok, peer_msg = world > 1, None
    selfcheck = {}
    guard = LineGuard(rank)
    if world > 1 and not a.pmc_child:
        # FIRST the step that needs nothing but each rank's own handle and the collective: shards with local parents + the
        # all-gather.  Its line is kept; it is printed only if what follows (mapping the other ranks' planes) never returns.
        guard.arm(float(os.environ.get("RBS_BENCH_FIRST_TIMEOUT", "300")), "the first step with local parents + the all-gather")
        fb_sensor = make_sensor(a, om, cam, P, dev)
        prime(fb_sensor, a, W)

        def fb_gather(out_t, inp_t):
            if backend == "nccl":
                dist.all_gather_into_tensor(out_t, inp_t)
            else:
                host = [torch.empty(n, dtype=torch.float64) for _ in range(world)]
                dist.all_gather(host, inp_t.cpu())
                out_t.copy_(torch.cat(host))

        fb_run = LocalShardRun(a, W, fb_sensor, stream, d_out, d_all, fb_gather)
        fb_region_ms = []
        for rep, k_steps in enumerate(region_steps(a.steps)):
            el = fb_run.timed(k_steps, max(a.warmup, MIN_WARMUP_STEPS) if rep == 0 else 0, barrier=dist.barrier)
            t = torch.tensor([el], dtype=torch.float64, device=dev if backend == "nccl" else "cpu")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            fb_region_ms.append(float(t.item()) / k_steps * 1e3)
        torch.cuda.synchronize()
        dist.barrier()
        fb_sensor.close()
        del fb_run
        fb_line = headline(a, world, n, n_tri, fb_region_ms, "local")
        guard.best = fb_line
        guard.arm(float(os.environ.get("RBS_BENCH_ATTACH_TIMEOUT", "240")), "rbs_ipc_attach / the multi-GPU self-check / the attached step")
    if world > 1:
        if a.full:
            try:
                selfcheck = multi_gpu_selfcheck(a, dev, stream, dist, backend, world, rank)
            except Exception as e:   # noqa: BLE001 -- the check must not take the headline down
                selfcheck = {"multi_gpu_equals_single": False, "multi_gpu_check_diagnosis": f"self-check raised {e!r}"} if rank == 0 else {}
        try:
            sensor, run = setup_peer_run(a, om, cam, P, W, dev, stream, dist, backend, world)
            d_out, d_all = run.step.d_out, run.step.d_all
        except RuntimeError as e:          # (dist.attach_peers raises on EVERY rank when any rank could not attach)
            peer_ok, peer_msg = False, str(e)
            if rank == 0:
                print("# bench.py: " + peer_msg + " -- falling back to shards with local parents + all-gather", file=sys.stderr)
            sensor = make_sensor(a, om, cam, P, dev)
            prime(sensor, a, W)

            def gather(out_t, inp_t):
                if backend == "nccl":
                    dist.all_gather_into_tensor(out_t, inp_t)
                else:
                    host = [torch.empty(n, dtype=torch.float64) for _ in range(world)]
                    dist.all_gather(host, inp_t.cpu())
                    out_t.copy_(torch.cat(host))

            run = LocalShardRun(a, W, sensor, stream, d_out, d_all, gather)
    else:
        sensor = make_sensor(a, om, cam, P, dev)
        prime(sensor, a, W)
        run = ResidentRun(a, W, sensor, stream, d_out)

    if a.pmc_child:                # wrapped by rocprofv3: a few steps, no output
        run.timed(a.steps, a.warmup)
        sensor.close()
        return

    # --steps timed steps in all, in up to REPEATS regions (every one bracketed by barrier +
    # synchronize on both sides, the MAX over ranks taken per region); the headline is the MEDIAN
    # region's ms per step -- a 20-step region is 4 ms, and one region alone moved by 7 % between runs
    region_ms = []
    for rep, k_steps in enumerate(region_steps(a.steps)):
        el = run.timed(k_steps, max(a.warmup, MIN_WARMUP_STEPS) if rep == 0 else 0, barrier=dist.barrier if world > 1 else None)
        if world > 1:
            t = torch.tensor([el], dtype=torch.float64, device=dev if backend == "nccl" else "cpu")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            el = float(t.item())
        region_ms.append(el / k_steps * 1e3)
    if world > 1:
        # every rank must hold every rank's log-likelihoods after the exchange
        ref = d_all.view(world, n)[rank].cpu().numpy()
        if not np.array_equal(ref, d_out.cpu().numpy()):
            raise SystemExit("all-gather returned the wrong shard")
    ll = d_out.cpu().numpy()
    if not np.isfinite(ll).all():
        raise SystemExit("non-finite log-likelihoods in the timed run")
    if a.dump_outputs and rank == 0:   # the last timed step's log-likelihoods (several ranks: every rank's, gathered)
        dump_outputs(a.dump_outputs, {"loglikes": d_all.cpu().numpy() if world > 1 else ll})
    if a.full:
        # dominant-kernel durations: a separate pass of 512 launches, 256 of them bracketed by events
        raster_ms, copy_ms, call_ms, n_used = run.kernel_times(512)
        windows = np.array([sensor.get_window(s_) for s_ in range(0, n, max(1, n // 64))])
        win_frac = float(np.mean(np.maximum(0, windows[:, 2] - windows[:, 0]) * np.maximum(0, windows[:, 3] - windows[:, 1]))) / (a.rows * a.cols)
    peer_stats, peer_legs = None, {}
    if world > 1:
        # the headline is measured: from here on the watchdog would print IT (without the legs that follow)
        best = headline(a, world, n, n_tri, region_ms, "ipc" if peer_ok else "local")
        best.update(selfcheck)
        best["peer_step"] = "ok" if peer_ok else "FAILED, local parents only: " + (peer_msg or "")
        guard.best = best
        guard.arm(float(os.environ.get("RBS_BENCH_LEGS_TIMEOUT", "1500")), "the legs behind the headline (flattened weights, C3 / C4 per-GPU sizes, sharded tracker)")
    if world > 1 and not peer_ok:
        peer_stats = {"peer_step": "FAILED, local parents only: " + (peer_msg or "")}
        torch.cuda.synchronize()
        dist.barrier()
        sensor.close()
    if world > 1 and peer_ok:
        peer_stats = run.stats()
        peer_stats["peer_step"] = "ok"
        if a.full:
            # the same step with FLATTENED weights (temperature = the spread of the log-likelihoods): many distinct parents,
            # a large share of them on other ranks and unshared -- the case that exercises the in-place reads over xGMI
            # (the filter's own weights on these synthetic poses leave one or two survivors per step)
            run.reset_stats()
            run.step.temperature = max(1.0, float(d_all.std().item()))
            run.timed(a.warmup + 3, 0, barrier=dist.barrier)
            run.reset_stats()
            el2 = run.timed(a.steps, 0, barrier=dist.barrier)
            t2 = torch.tensor([el2], dtype=torch.float64, device=dev if backend == "nccl" else "cpu")
            dist.all_reduce(t2, op=dist.ReduceOp.MAX)
            peer_stats.update({"spread_parents_" + k_: v_ for k_, v_ in run.stats().items()})
            peer_stats["spread_parents_value"] = n * world * a.steps / float(t2.item())
            peer_stats["spread_parents_temperature"] = run.step.temperature
        torch.cuda.synchronize()
        dist.barrier()                     # every rank is done reading its peers' planes: handles may go
        sensor.close()
        if not a.no_configs_leg and a.config in (None, "c1"):
            try:
                peer_legs = peer_configs_leg(a, dev, stream, dist, backend, world, rank)
            except RuntimeError as e:      # (attach_peers: raised on every rank alike)
                peer_legs = {"configs_note": "C3 / C4 legs failed: " + str(e)}
        # tracker FPS over the job's GPUs: the device tracker sharded inside ONE handle (rank 0 drives every device; the
        # other ranks wait) -- the reference's node is one process (R:source/dbot_ros/tracker/particle_tracker_node.cpp:277-284)
        if not a.no_tracker_fps and os.environ.get("RBS_BENCH_SHARDED_TRACKER", "1") != "0":
            # (the other ranks wait on the rendezvous STORE, on the host: a collective barrier would park a spinning RCCL
            # kernel on every GPU rank 0 is about to time)
            store = dist.distributed_c10d._get_default_store()
            if rank == 0:
                ids = [0] * world if backend != "nccl" else list(range(world))
                peer_legs.update(sharded_tracker_leg(a, ids))
                store.set("rbs_sharded_tracker_done", "1")
            else:
                store.wait(["rbs_sharded_tracker_done"])

    if rank != 0:
        if world > 1:
            dist.destroy_process_group()
        else:
            sensor.close()
        return

    alg_bytes = (2.0 if a.update else 1.0) * 4.0 * a.rows * a.cols * n  # per launch, SURVEY 8d
    out = headline(a, world, n, n_tri, region_ms, None if world == 1 else ("ipc" if peer_ok else "local"))
    if world > 1:
        if not peer_ok:
            out["config"]["workload"] += " -- the ranks' handles could not be attached to each other, see peer_step"
        out.update(selfcheck)
        out.update(peer_stats)
        out.update(peer_legs)
    single = world == 1
    if a.full:
        # whole planes: the copy kernel is the dominant one and HBM bound.  Windowed planes: the raster kernel
        # (the windowed copy kernel runs BESIDE it and moves ~1 % of the algorithmic bytes: pricing it with
        # them would report several times the HBM peak)
        copy_dominant = bool(a.update) and a.layout == "dense" and copy_ms > raster_ms
        # (several ranks: rank 0's device; live counter passes only on request -- the other ranks would
        # wait minutes at the next collective -- otherwise the committed counters of the same launch)
        roof, pmc_live, copy_traffic = roofline_for(a, n, raster_ms, copy_ms, alg_bytes, copy_dominant,
                                                    not a.no_pmc and (single or os.environ.get("RBS_BENCH_PMC_MULTI") == "1"))
        roof.update({"counters_live": bool(pmc_live), "kernel_launches_averaged": n_used,
                     "raster_kernel_ms": raster_ms, "copy_kernel_ms": copy_ms, "call_ms_launch_stream": call_ms,
                     "copy_kernel_hbm_bytes_per_launch": copy_traffic,
                     "state_layout": a.layout, "stored_window_fraction_of_plane": win_frac,
                     "algorithmic_bytes_per_launch": alg_bytes})
        out["roofline"] = roof
    if world == 1:
        sensor.close()

    # ---- the same steps on whole planes: the copy kernel is dominant there and HBM bound
    if single and a.update and a.layout == "window" and not a.no_dense_leg:
        dense = make_sensor(a, om, cam, P, dev, layout="dense")
        prime(dense, a, W)
        drun = ResidentRun(a, W, dense, stream, d_out)
        dsteps = 200                      # the legs run a fixed number of steps, whatever --steps says
        td = drun.timed(dsteps, a.warmup)
        d_raster_ms, d_copy_ms, _, d_used = drun.kernel_times(400)
        dense.close()
        dfetch = dwrite = None
        if not a.no_pmc:
            dfetch = pmc_pass(a, ["FETCH_SIZE"], "dense")
            dwrite = pmc_pass(a, ["WRITE_SIZE"], "dense")
        dtraffic = hbm_bytes(dfetch, dwrite, "rbs_copy_rows_kernel")
        dach = alg_bytes / (d_copy_ms * 1e-3) / 1e9
        out["dense_value"] = n * dsteps / td
        out["dense_ms_per_step"] = td / dsteps * 1e3
        out["roofline"].update({"dense_bound": "hbm", "dense_kernel": "rbs_copy_rows_kernel", "dense_kernel_ms": d_copy_ms,
                                "dense_achieved_GBps": dach, "dense_frac": dach / HBM_PEAK_GBPS,
                                "dense_frac_of_measured_copy": dach / HBM_COPY_MEASURED_GBPS,   # (what a float4 copy reaches on this part: the guide)
                                "dense_traffic": dtraffic,
                                "dense_traffic_over_algorithmic": (dtraffic / alg_bytes) if dtraffic else None,
                                "dense_kernel_launches_averaged": d_used, "dense_raster_kernel_ms": d_raster_ms})
    # ---- the other likelihood precision, same steps (F32 is opt-in: float32-level agreement only)
    other = "f32" if a.precision == "f64" else "f64"
    if single and not a.no_f32_leg:
        so = make_sensor(a, om, cam, P, dev, precision=other)
        prime(so, a, W)
        ro = ResidentRun(a, W, so, stream, d_out)
        s_ = 300
        to = ro.timed(s_, a.warmup)
        ko = ro.kernel_times(400)
        so.close()
        out[f"{other}_value"] = n * s_ / to
        out[f"{other}_ms_per_step"] = to / s_ * 1e3
        out[f"{other}_raster_kernel_ms"] = ko[0]
        if other == "f32":
            out["f32_note"] = ("opt-in rbs_config.likelihood_precision = F32: float32 likelihood over binary64 geometry; within 1e-5 of the "
                               "reference semantics only for well-conditioned sums, parent indices not reproduced at large particle counts")
    # ---- the reference's own occlusion bookkeeping on the device (rbs_config.occlusion_mode = REFERENCE, opt-in): what it costs
    if single and not a.no_f32_leg and a.precision == "f64" and a.layout == "window" and a.update and getattr(a, "occlusion", None) != "reference":
        sx = make_sensor(a, om, cam, P, dev, occlusion="reference")
        prime(sx, a, W)
        rx = ResidentRun(a, W, sx, stream, d_out)
        s_ = 300
        tx = rx.timed(s_, a.warmup)
        kx = rx.kernel_times(400)
        sx.close()
        out["exact_occlusion_value"] = n * s_ / tx
        out["exact_occlusion_ms_per_step"] = tx / s_ * 1e3
        out["exact_occlusion_raster_kernel_ms"] = kx[0]
        out["exact_occlusion_copy_kernel_ms"] = kx[1]
        out["exact_occlusion_note"] = ("the headline's steps with rbs_config.occlusion_mode = REFERENCE (opt-in): per-pixel posterior + 16-bit age, the prior "
                                       "propagated in binary64 at use with the oracle's operations -- bit-identical priors, log-likelihoods within 1e-11 of "
                                       "the reference-semantics (LAZY) oracle, not one resampled child of 600 000 with another parent "
                                       "(tests/test_gpu_reference_semantics.py); the cost is the ages' memory traffic in the pixel pass "
                                       "(profiles/r06_exact_occlusion_cost.txt)")
    if single and not a.no_configs_leg and a.config in (None, "c1"):
        out.update(configs_leg(a, dev, stream))
    if single and not a.no_sweep_leg and a.config in (None, "c1") and a.layout == "window":
        try:
            out.update(sweep_leg(a, dev, stream))
            if out.get("sweep_value") and out.get("sweep_window_fraction"):
                # the bytes the sweep's calls really move: the stored fraction of SURVEY 8(d)'s 2 x 4 x W x H per particle-likelihood
                out["sweep_hbm_frac"] = out["sweep_value"] * 8.0 * a.rows * a.cols * out["sweep_window_fraction"] / (HBM_PEAK_GBPS * 1e9)
        except Exception as e:   # noqa: BLE001 -- a leg must not take the headline down
            out["sweep_note"] = f"sweep leg failed: {e!r}"
    # ---- the step `--gpus N` times, on this one rank: the like-for-like reference of the multi-rank values
    if single and not a.no_configs_leg and a.config in (None, "c1") and a.layout == "window" and a.update:
        try:
            out.update(single_rank_filter_step_leg(a, om, cam, P, W, dev, stream))
        except Exception as e:   # noqa: BLE001 -- a leg must not take the headline down
            out["filter_step_note"] = f"single-rank filter-step leg failed: {e!r}"
    # ---- host-pointer API: frame upload + pose upload + log-likelihood download inside the clock
    if single and not a.no_host_leg:
        hs = make_sensor(a, om, cam, P, dev)
        prime(hs, a, W)
        hsteps = 300

        def host_step(i, with_frame=True):
            k = W.order[i % len(W.order)]
            if with_frame:
                hs.set_observation(W.frames[k])
            idx = W.parents.copy()
            return hs.loglikes_poses(W.poses[k], idx, update=bool(a.update))

        for i in range(10):
            host_step(i)
        t0 = time.perf_counter()
        for i in range(hsteps):
            host_step(i)
        th = time.perf_counter() - t0
        t0 = time.perf_counter()
        for i in range(hsteps):
            host_step(i, with_frame=False)
        tl = time.perf_counter() - t0
        # the same with the frame written straight into the handle's pinned staging buffer
        # (rbs_acquire_frame_buffer / rbs_commit_frame_buffer): what a driver callback that converts
        # its message into that buffer pays -- no 1.2 MB host copy inside the API
        def staged_step(i):
            k = W.order[i % len(W.order)]
            hs.frame_buffer()           # the producer's buffer: left as it is (its content is one of the two last frames)
            hs.commit_frame()
            return hs.loglikes_poses(W.poses[k], W.parents.copy(), update=bool(a.update))

        for i in range(10):
            staged_step(i)
        t0 = time.perf_counter()
        for i in range(hsteps):
            staged_step(i)
        ts = time.perf_counter() - t0
        # the same with the NEXT frame handed over with each call (rbs_loglikes_prefetch): its staging copy and transfer
        # pass behind the call's kernels; rbs_set_observation_prefetched then costs nothing.  Still every frame from
        # host memory, every pose up and every log-likelihood down inside the clock.
        def ahead_step(i):
            k, k1 = W.order[i % len(W.order)], W.order[(i + 1) % len(W.order)]
            ll_ = hs.loglikes_poses_prefetch(W.poses[k], W.parents.copy(), W.frames[k1], update=bool(a.update))
            hs.set_observation_prefetched()
            return ll_

        hs.set_observation(W.frames[W.order[0]])
        for i in range(10):
            ahead_step(i)
        t0 = time.perf_counter()
        for i in range(10, 10 + hsteps):
            ahead_step(i)
        tp = time.perf_counter() - t0
        hs.close()
        out["host_api_prefetch_value"] = n * hsteps / tp
        out["host_api_prefetch_ms_per_step"] = tp / hsteps * 1e3
        out["host_api_staged_frame_value"] = n * hsteps / ts
        out["host_api_value"] = n * hsteps / th
        out["host_api_ms_per_step"] = th / hsteps * 1e3
        out["host_api_loglikes_only_value"] = n * hsteps / tl
        out["host_api_note"] = ("rbs_set_observation_f32 (1.2 MB frame from host memory) + rbs_loglikes (poses + parent indices "
                                "from host memory, log-likelihoods back to host memory, synchronous), called through ctypes; "
                                "host_api_prefetch_*: the same frames, poses and results through rbs_loglikes_prefetch + "
                                "rbs_set_observation_prefetched (frame k+1 handed over with call k: a recorded dataset, or a driver one frame ahead); "
                                "host_api_loglikes_only_value = SURVEY 8(d)'s definition of the metric to the letter (pose upload and "
                                "log-likelihood download inside the clock, no frame)")
        # the same step driven from C++ through the C-ABI (tests/cpp/host_bench.cpp): what the
        # reference's own filter, which is C++, would pay -- no interpreter between the calls
        nat = native_host_leg(a, om, cam, P, W, hsteps)
        if nat:
            out.update(nat)
    # ---- tracker FPS, the second half of the metric
    if single and not a.no_tracker_fps:
        fps = tracker_fps(om, cam, dev, precision=a.precision)
        # BASELINE config C2 as a tracker: 20 000 evaluations per frame = 6 666 particles x 3 sampling
        # blocks (meshes M1, M2, M3), two read-only blocks and one updating block per frame
        from dbot_ros_amd import ObjectModel, synth
        meshes = [synth.mesh_m1(), synth.mesh_m2(), synth.mesh_m3()]
        om_c2 = ObjectModel([v for v, _ in meshes], [t for _, t in meshes], center=True)
        nat_frames, nat_init = fps.pop("_native")
        out.update(native_tracker_leg(om, cam, P, nat_frames, nat_init, (200, 2000, 20000), a.precision))
        c2 = tracker_fps(om_c2, cam, dev, counts=(20000,), precision=a.precision)[20000]
        out["tracker_fps_c2"] = c2["fps"]
        out["tracker_fps_pipelined_c2"] = c2["fps_pipelined"]
        out["tracker_c2_note"] = ("C2: 6 666 particles x 3 bodies (M1, M2, M3) = 20 000 particle-likelihoods per frame, 640x480; "
                                  f"{c2['resamplings']} resamplings, final position error {c2['final_position_error_m']:.4f} m")
        for k, v in fps.items():
            out[f"tracker_fps_{k}"] = v["fps"]
            out[f"tracker_fps_pipelined_{k}"] = v["fps_pipelined"]
            out[f"tracker_ms_per_frame_{k}"] = v["ms_per_frame"]
        out["tracker_fps_note"] = ("device tracker (rbs_tracker_*), one object (M1), 640x480, 30-frame sequence, frame uploaded "
                                   "from host memory every frame, precision " + a.precision.upper() + "; resamplings " +
                                   "/".join(str(v["resamplings"]) for v in fps.values()))
    if single and not a.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline(om, cam, P, W.truths[0], W.frames[0], a.cpu_seconds)
    guard.disarm()
    # ---- SURVEY 8(d)'s own figures first: `value` stays the bench contract's (inputs resident in HBM when the clock
    # starts); the metric as SURVEY 8(d) words it -- pose upload and log-likelihood download inside the clock -- is host_pointer_value,
    # and through the plugin surface the reference would call (the double image inside the clock as well) plugin_api_value
    if single and a.full:
        lead = {"resident_value": out["value"],
                "host_pointer_value": out.get("host_api_native_loglikes_only_value", out.get("host_api_loglikes_only_value")),
                "plugin_api_value": out.get("plugin_api_value"), "plugin_api_borrowed_value": out.get("plugin_api_borrowed_value"),
                "exact_occlusion_value": out.get("exact_occlusion_value"),
                "dense_hbm_frac": out["roofline"].get("dense_frac"), "sweep_value": out.get("sweep_value"), "sweep_hbm_frac": out.get("sweep_hbm_frac"),
                "roofline_frac": out["roofline"].get("frac"),
                "note": "particle-likelihoods/s on C1, one GPU.  resident_value = `value` (device-pointer API, inputs in HBM: the bench contract's clock); "
                        "host_pointer_value = SURVEY 8(d)'s metric to the letter (rbs_loglikes from host memory: poses up, log-likelihoods down, synchronous; called from "
                        "C++ as the reference's filter would -- host_api_loglikes_only_value is the same through ctypes); "
                        "plugin_api_value = the reference's own call sequence from C++ (set_observation of a double image, copied, + loglikes(deltas, indices, "
                        "update)); exact_occlusion_value = resident_value with rbs_config.occlusion_mode = REFERENCE; dense / sweep: where SURVEY 8(d)'s "
                        "bytes really move, as fractions of 8 TB/s; roofline_frac: the dominant kernel against the guide's VALU issue peak"}
        out = {**{k: out[k] for k in ("metric", "value", "unit")}, "survey_8d": lead, **{k: v for k, v in out.items() if k not in ("metric", "value", "unit")}}
    out["bench_wall_s"] = round(time.perf_counter() - t_main, 1)   # the whole run, every leg (the timed region is ms_per_step x steps)
    print(json.dumps(out), flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
