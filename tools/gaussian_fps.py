"""Frames per second of the robust Gaussian tracker (rbs_gauss_*), frame by frame, and its CPU twin
(tests/gauss_twin.py, numpy + the oracle's renderer, one core) beside it.  Prints ONE JSON line:

    {"tool": "gaussian_fps", "cases": [{"case", "size", "bodies", "sigma_poses", "fps", "ms_per_frame",
      "device_ms": {"render", "moments", "reduce"}, "submit_fps", "lookahead_fps", "twin_fps"}, ...]}

Cases: M1 and [M1, M2, M3] at 640x480, M4 at 1280x960; synthetic frames of scenarios.make_frames
(occluding slab, 5 % NaN).  device_ms: the library's HIP events around its three kernels, averaged
over the timed frames.  fps: rbs_gauss_track frame by frame (the D x D algebra on the host); submit_fps:
rbs_gauss_submit + rbs_gauss_result frame by frame (the whole step on the device); lookahead_fps: submit k + 1
before result k (two frames in flight).  Usage: python tools/gaussian_fps.py [--frames N] [--warmup W] [--twin-frames T]
"""
import os

for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):   # the twin: one core
    os.environ[_v] = "1"

import argparse  # noqa: E402
import json  # noqa: E402
import sys  # noqa: E402
import time  # noqa: E402

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import gauss_twin as gt  # noqa: E402
import oracle_binding as ob  # noqa: E402
import scenarios as sc  # noqa: E402
from dbot_ros_amd import RbSensor, RbSensorBuilder  # noqa: E402
from dbot_ros_amd.gaussian import GaussianTracker, GaussianTrackerBuilder  # noqa: E402

CASES = (("M1", ("m1",), 640, 480), ("M1+M2+M3", ("m1", "m2", "m3"), 640, 480), ("M4", ("m4",), 1280, 960))


def run_case(name, meshes, cols, rows, n_frames, warmup, twin_frames):
    om, cam, P = sc.make_scene(meshes, cols, rows, max_particles=1)
    orc = ob.Oracle(om, cam, P, max_particles=1)
    total = warmup + n_frames
    frames = sc.make_frames(orc, len(meshes), min(total, 30), seed=0)
    frames = [frames[k % len(frames)] for k in range(total)]
    sensor = RbSensor(om, cam, RbSensorBuilder.Parameters(sample_count=1), max_particles=1)
    params = GaussianTrackerBuilder.Parameters()
    params.object_transition.part_count = len(meshes)
    tracker = GaussianTracker(sensor, om, params)
    try:
        tracker.initialize([tracker._from_model(gt.truth_state(frames[0][0]))])
        for _, y in frames[:warmup]:
            tracker.track(y)
        ms = np.zeros(3)
        t0 = time.perf_counter()
        for _, y in frames[warmup:]:
            tracker.track(y)
            ms += tracker.kernel_ms()
        wall = time.perf_counter() - t0
        n_sigma = len(tracker.sigma_poses())
        walls = {}
        for mode in ("submit", "lookahead"):
            tracker.initialize([tracker._from_model(gt.truth_state(frames[0][0]))])
            for _, y in frames[:warmup]:
                tracker.submit(y)
                tracker.result()
            ys = [y for _, y in frames[warmup:]]
            t0 = time.perf_counter()
            if mode == "submit":
                for y in ys:
                    tracker.submit(y)
                    tracker.result()
            else:
                tracker.submit(ys[0])
                for k in range(len(ys)):
                    if k + 1 < len(ys):
                        tracker.submit(ys[k + 1])
                    tracker.result()
            walls[mode] = time.perf_counter() - t0
    finally:
        tracker.close()
        sensor.close()
    tw = gt.GaussTwin(gt.Params.from_builder(params), len(meshes), orc.render_depth)
    tw.initialize(gt.truth_state(frames[0][0]))
    t0 = time.perf_counter()
    for _, y in frames[:twin_frames]:
        tw.track(y)
    twin_wall = time.perf_counter() - t0
    return {"case": name, "size": f"{cols}x{rows}", "bodies": len(meshes), "sigma_poses": n_sigma,
            "fps": round(n_frames / wall, 1), "ms_per_frame": round(1e3 * wall / n_frames, 4),
            "device_ms": {k: round(float(v) / n_frames, 4) for k, v in zip(("render", "moments", "reduce"), ms)},
            "submit_fps": round(n_frames / walls["submit"], 1), "lookahead_fps": round(n_frames / walls["lookahead"], 1),
            "twin_fps": round(twin_frames / twin_wall, 3)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--twin-frames", type=int, default=3)
    a = ap.parse_args()
    cases = [run_case(n, m, c, r, a.frames, a.warmup, a.twin_frames) for n, m, c, r in CASES]
    print(json.dumps({"tool": "gaussian_fps", "cases": cases}))


if __name__ == "__main__":
    main()
