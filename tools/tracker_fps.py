#!/usr/bin/env python3
"""Tracker FPS (the second half of BASELINE.json's metric): frames/s of the full per-frame step
-- set_observation + transition + loglikes(update) + weights + KL + resample + mean -- on a
30-frame synthetic sequence (object translating 2 mm and rotating 1 degree per frame), for
{200, 2 000, 20 000} particles on one MI355X.  Two variants per count: filter='device' (rbs_tracker_*: transition, weights, KL,
resampling, mean on the GPU, one host sync per frame) and filter='host' (numpy mirror).  Prints one JSON line per particle count.

    tracker_fps.py [COUNTS [MESHES]] --posterior [--repeats R]
the device tracker's posterior report (rbs_tracker_set_posterior) off and on, alternating in ONE process after a warm-up, frame
by frame and with look-ahead (two frames in flight): frames/s of each (median and range over the repeats -- the range is the
run-to-run spread a difference has to exceed) and the report's kernels' device time from events.  One JSON line per count.

    tracker_fps.py [COUNTS [MESHES]] --occlusion-map [--never-resample] [--repeats R]
the same measurement for the device tracker's occlusion map (rbs_tracker_set_occlusion_map); MESHES m1,m2,m3 is the
three-body scene; --never-resample sets max_kl_divergence so large that nothing resamples and every slot stays live.

    tracker_fps.py [COUNTS [MESHES]] --object-map [--never-resample] [--repeats R]
the same for the device tracker's object map (rbs_tracker_set_object_map), with the sensor's raster kernel time of the
frame's likelihood call beside the map's (rbs_raster_kernel_ms: the kernel that draws the same poses).

    tracker_fps.py [COUNTS [MESHES]] --modes [--never-resample] [--repeats R]
the same for the device tracker's posterior modes (rbs_tracker_set_modes, the default parameters); with the number of modes of
the last frame's first body."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dbot_ros_amd import CameraData, ObjectModel, RbSensor, RbSensorBuilder, pose, synth  # noqa: E402
from dbot_ros_amd.tracker import (DeviceParticleTracker, ObjectTransitionBuilder, ParticleTracker,  # noqa: E402
                                  ParticleTrackerBuilder)


def posterior_main(argv, product="posterior"):
    """--posterior, --occlusion-map, --object-map, --modes: see the module's docstring."""
    repeats = 5
    never = product != "posterior" and "--never-resample" in argv
    argv = [a for a in argv if a != "--never-resample"]
    if "--repeats" in argv:
        k = argv.index("--repeats")
        repeats = int(argv[k + 1])
        del argv[k:k + 2]
    counts = [int(x) for x in argv[0].split(",")] if len(argv) > 0 else [200, 2000, 20000]
    names = argv[1].split(",") if len(argv) > 1 else ["m1"]
    cols, rows, n_frames = 640, 480, 30
    fns = {"m1": synth.mesh_m1, "m2": synth.mesh_m2, "m3": synth.mesh_m3, "m4": synth.mesh_m4}
    meshes = [fns[k]() for k in names]
    nb = len(meshes)
    om = ObjectModel([v for v, _ in meshes], [t for _, t in meshes], center=True)
    cam = CameraData(synth.camera_matrix(cols, rows), rows, cols)
    init = np.zeros(12 * nb)
    for b in range(nb):
        Rt = synth.truth_pose(nb, frame=0)[b]
        init[12 * b + 3:12 * b + 6] = pose.matrix_to_rotvec(Rt[:9].reshape(3, 3))
        init[12 * b:12 * b + 3] = Rt[9:] - Rt[:9].reshape(3, 3) @ om.centers[b]
    for n in counts:
        P = RbSensorBuilder.Parameters(sample_count=n)
        with RbSensor(om, cam, P, max_particles=max(1, n // nb)) as s:
            rng = np.random.default_rng(0)
            frames = [synth.make_frame(s.render_depth(synth.truth_pose(nb, frame=k)), rows, cols, rng, occluder=False)
                      for k in range(n_frames + 1)]
            trans = ObjectTransitionBuilder(ObjectTransitionBuilder.Parameters(part_count=nb)).build()
            tp = ParticleTrackerBuilder.Parameters(evaluation_count=n)
            if never:
                tp.max_kl_divergence = 1e30
            tr = DeviceParticleTracker(trans, s, om, tp, device_rng=True, seed=1)
            switch, ms_of, last = {"posterior": (tr.set_posterior, tr.posterior_ms, tr.posterior),
                                   "occlusion_map": (tr.set_occlusion_map, tr.occlusion_map_ms, tr.occlusion_map),
                                   "object_map": (tr.set_object_map, tr.object_map_ms, tr.object_map),
                                   "modes": (lambda on: tr.set_modes(True if on else None), tr.modes_ms, tr.modes)}[product]

            def block(on, look_ahead, collect_ms=None):
                """The 30 frames from a fresh initialize -> frames/s (the same sequence every time: device RNG, same seed)."""
                tr.initialize([init])
                switch(on)
                tr.track(frames[0])
                t0 = time.perf_counter()
                if look_ahead:
                    tr.submit(frames[1])
                    for k in range(2, n_frames + 1):
                        tr.submit(frames[k])
                        tr.result()
                    tr.result()
                else:
                    for k in range(1, n_frames + 1):
                        tr.track(frames[k])
                        if collect_ms is not None:
                            collect_ms.append(ms_of())
                dt = time.perf_counter() - t0
                if on:
                    assert last().frame == n_frames + 1
                return n_frames / dt

            for on in (False, True):      # warm-up: every kernel of both settings has run
                block(on, False), block(on, True)
            ms = []
            block(True, False, collect_ms=ms)                 # (a pass of its own: the query is not inside the timed loops)
            fps = {(on, la): [] for on in (False, True) for la in (False, True)}
            for _ in range(repeats):
                for la in (False, True):
                    for on in (False, True):                  # alternating
                        fps[(on, la)].append(block(on, la))
            what = {"posterior": "posterior report", "occlusion_map": "occlusion map", "object_map": "object map",
                    "modes": "posterior modes"}[product]
            out = {"metric": "tracker FPS, %s off / on" % what, "evaluation_count": n, "objects": nb, "particles": max(1, n // nb),
                   "repeats": repeats, "unit": "frames/s", "resolution": [cols, rows],
                   product + "_kernels_device_ms": {"median": float(np.median(ms)), "min": float(np.min(ms)), "max": float(np.max(ms))}}
            if product != "posterior":
                out["resamplings"] = tr.n_resamplings
            if product == "modes":
                out["modes_of_body_0_last_frame"] = len(last().bodies[0])
            if product == "object_map":
                out["raster_kernel_ms_last_call"] = float(s.raster_kernel_ms())
            for (on, la), v in fps.items():
                out[("on" if on else "off") + ("_look_ahead" if la else "_frame_by_frame")] = {
                    "median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}
            for la, name in ((False, "frame_by_frame"), (True, "look_ahead")):
                out["on_over_off_" + name] = float(np.median(fps[(True, la)]) / np.median(fps[(False, la)]))
            tr.close()
            print(json.dumps(out), flush=True)


def main():
    if "--posterior" in sys.argv:
        argv = [a for a in sys.argv[1:] if a != "--posterior"]
        return posterior_main(argv)
    if "--occlusion-map" in sys.argv:
        argv = [a for a in sys.argv[1:] if a != "--occlusion-map"]
        return posterior_main(argv, product="occlusion_map")
    if "--object-map" in sys.argv:
        argv = [a for a in sys.argv[1:] if a != "--object-map"]
        return posterior_main(argv, product="object_map")
    if "--modes" in sys.argv:
        argv = [a for a in sys.argv[1:] if a != "--modes"]
        return posterior_main(argv, product="modes")
    counts = [int(x) for x in sys.argv[1].split(",")] if len(sys.argv) > 1 else [200, 2000, 20000]
    names = sys.argv[2].split(",") if len(sys.argv) > 2 else ["m1"]     # e.g. m1,m2,m3 = BASELINE config C2
    cols, rows, n_frames = 640, 480, 30
    fns = {"m1": synth.mesh_m1, "m2": synth.mesh_m2, "m3": synth.mesh_m3, "m4": synth.mesh_m4}
    meshes = [fns[k]() for k in names]
    nb = len(meshes)
    f = np.concatenate([t for _, t in meshes])
    om = ObjectModel([v for v, _ in meshes], [t for _, t in meshes], center=True)
    cam = CameraData(synth.camera_matrix(cols, rows), rows, cols)
    for n, mode in [(n, m) for n in counts for m in ("device", "host")]:
        P = RbSensorBuilder.Parameters(sample_count=n)
        with RbSensor(om, cam, P, max_particles=max(1, n // nb)) as s:
            rng = np.random.default_rng(0)
            frames = [synth.make_frame(s.render_depth(synth.truth_pose(nb, frame=k)), rows, cols, rng,
                                       occluder=False) for k in range(n_frames + 1)]
            trans = ObjectTransitionBuilder(ObjectTransitionBuilder.Parameters(part_count=nb)).build()
            tp = ParticleTrackerBuilder.Parameters(evaluation_count=n)
            if mode == "device":   # transition + filter step + mean on the GPU, device RNG
                tr = DeviceParticleTracker(trans, s, om, tp, device_rng=True, seed=1)
            else:                  # host mirror (numpy)
                tr = ParticleTracker(trans, s, om, tp, np.random.default_rng(1))
            init = np.zeros(12 * nb)
            for b in range(nb):
                Rt = synth.truth_pose(nb, frame=0)[b]
                init[12 * b + 3:12 * b + 6] = pose.matrix_to_rotvec(Rt[:9].reshape(3, 3))
                init[12 * b:12 * b + 3] = Rt[9:] - Rt[:9].reshape(3, 3) @ om.centers[b]
            tr.initialize([init])
            tr.track(frames[0])  # warm-up
            t0 = time.perf_counter()
            sensor_ms = 0.0
            for k in range(1, n_frames + 1):
                est = tr.track(frames[k])
            dt = time.perf_counter() - t0
            sensor_ms = s.timing_summary(n_frames * nb)[0] * n_frames * nb   # sampled kernel timing, outside the loop
            Rt = synth.truth_pose(nb, frame=n_frames)[0]
            err = np.linalg.norm(est[0:3] - (Rt[9:] - Rt[:9].reshape(3, 3) @ om.centers[0]))
            print(json.dumps({"metric": "tracker FPS", "filter": mode, "evaluation_count": n, "objects": nb, "particles": max(1, n // nb), "value": n_frames / dt, "unit": "frames/s",
                              "ms_per_frame": dt / n_frames * 1e3, "sensor_device_ms_per_frame": sensor_ms / n_frames,
                              "resamplings": tr.n_resamplings, "final_position_error_m": float(err),
                              "resolution": [cols, rows], "triangles": int(len(f)), "n_gpus": 1}), flush=True)


if __name__ == "__main__":
    main()
