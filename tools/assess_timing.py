"""Time per call of the pose assessor (rbs_assess_poses) on one device beside one tracker frame, and what its verdicts
say about the object finder's finds.  Prints ONE JSON line:

    {"tool": "assess_timing",
     "timing": {"size", "assess": [{"n", "host_ms", "render_ms", "count_ms"}, ...],
                "tracker_frame": {"particles", "host_ms"}},
     "finds": [{"case", "scene_seed", "truth": {"rendered", "support", "u", "fraction", "verdict"},
                "found": {"dt_mm", "rendered", "support", "u", "fraction", "verdict"}, "confirmed"}, ...]}

timing: M1 at 640x480, the truth pose and n - 1 perturbed copies against one synth.make_frame frame; host_ms: host
clock around rbs_assess_poses (frame given: staging, upload, both kernels, the copy back and the synchronisation),
averaged over --calls calls after a warm-up call; render_ms / count_ms: the library's HIP events of the last call.
tracker_frame: one rbs_tracker_track frame of a DeviceParticleTracker at --particles particles over the same sensor
size, host clock, averaged over --frames frames after a warm-up frame, in the same run.
finds: the object finder's default search on tools/find_object_timing.py's scenes (--cases x --scene-seeds: the six
of DESIGN.md Appendix F are m1,m2,m3 x 101,102), the truth pose and the best found pose assessed against the frame with
the assessor's default parameters; fraction = support / u, u = support + behind; confirmed: FindResult.confirmed.
--no-finds skips that part.
--contour: the assessor with the contour rule on at its defaults (rbs_contour_poses): "assess" rows gain "contour_ms" (the
third kernel), every record of "finds" gains "contour": {"rim", "valid", "flush", "in_front", "beyond", "verdict"}, "found"
rows gain "supported_by_plain_rule" and "confirmed" is Assessment.confirmed_mask()'s first pose.
Usage: python tools/assess_timing.py [--calls N] [--frames F] [--particles P] [--cases m1,m2,m3] [--scene-seeds 101,102] [--no-finds]
                                     [--contour]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import scenarios as sc  # noqa: E402
from dbot_ros_amd import RbSensor, RbSensorBuilder, synth  # noqa: E402
from dbot_ros_amd.assess import CONTOUR_COUNTS, CONTOUR_VERDICTS, SUPPORTED, VERDICTS, PoseAssessor  # noqa: E402
from dbot_ros_amd.finder import ObjectFinder  # noqa: E402
from dbot_ros_amd.pose import matrix_to_rotvec  # noqa: E402
from dbot_ros_amd.tracker import DeviceParticleTracker, ObjectTransitionBuilder, ParticleTrackerBuilder  # noqa: E402


def timing(calls, frames, particles, contour=None):
    cols, rows = 640, 480
    om, cam, _ = sc.make_scene(("m1",), cols, rows, max_particles=particles)
    P = RbSensorBuilder.Parameters(sample_count=particles)
    rng = np.random.default_rng(2)
    truths = [synth.truth_pose(1, z=0.7, frame=k) for k in range(frames + 1)]
    out = {"size": [cols, rows], "assess": []}
    with RbSensor(om, cam, P, max_particles=particles) as sensor:
        seq = [synth.make_frame(np.where(np.isfinite(d), d, np.inf), rows, cols, rng)
               for d in (sensor.render_depth(t) for t in truths)]
        a = PoseAssessor(sensor, contour=contour)
        for n in (1, 32):
            poses = np.concatenate([truths[0][None], synth.particle_poses(truths[0], n - 1, rng, scale=2.0)]) if n > 1 else truths[0][None]
            a.assess(poses, seq[0])                               # warm-up (and the buffers' allocation)
            t0 = time.perf_counter()
            for _ in range(calls):
                a.assess(poses, seq[0])
            host = (time.perf_counter() - t0) / calls * 1e3
            ms = a.kernel_ms()
            out["assess"].append({"n": n, "host_ms": round(host, 3), "render_ms": round(ms[0], 3), "count_ms": round(ms[1], 3)})
            if contour is not None:
                out["assess"][-1]["contour_ms"] = round(ms[2], 3)
        tr = DeviceParticleTracker(ObjectTransitionBuilder(ObjectTransitionBuilder.Parameters()).build(), sensor, om,
                                   ParticleTrackerBuilder.Parameters(evaluation_count=particles), device_rng=True, seed=1)
        s0 = np.zeros(12)
        R = truths[0][0, :9].reshape(3, 3)
        s0[:3], s0[3:6] = truths[0][0, 9:] - R @ om.centers[0], matrix_to_rotvec(R)
        tr.initialize([s0])
        tr.track(seq[0])                                          # warm-up
        t0 = time.perf_counter()
        for fr in seq[1:]:
            tr.track(fr)
        out["tracker_frame"] = {"particles": tr.n, "host_ms": round((time.perf_counter() - t0) / frames * 1e3, 3)}
        tr.close()
    return out


def record(c, v, cc=None, cv=None):
    rendered, support, behind = int(c[0]), int(c[2]), int(c[4])
    u = support + behind
    out = {"rendered": rendered, "support": support, "u": u, "fraction": round(support / u, 3) if u else None, "verdict": VERDICTS[int(v)]}
    if cc is not None:
        out["contour"] = dict({k: int(x) for k, x in zip(CONTOUR_COUNTS, cc)}, verdict=CONTOUR_VERDICTS[int(cv)])
    return out


def contour_of(a, k):
    return (a.contour_counts[k, 0], a.contour_verdicts[k, 0]) if a.contour_counts is not None else (None, None)


def finds(cases, seeds, contour=None):
    import find_object_timing as fot
    out = []
    for name in cases:
        mesh, cols, rows = fot.CASES[name]
        om, cam, P = sc.make_scene((mesh,), cols, rows, max_particles=1)
        for seed in seeds:
            with RbSensor(om, cam, P, max_particles=1) as sensor:
                truth, frame, _ = fot.scene(sensor, cam, seed)
                a = PoseAssessor(sensor, contour=contour)
                with ObjectFinder(sensor, om, ObjectFinder.Parameters()) as fnd:
                    r = fnd.find(frame, assess=a)
                t = a.assess(truth, frame)
                row = {"case": name, "scene_seed": seed, "truth": record(t.counts[0, 0], t.verdicts[0, 0], *contour_of(t, 0)), "found": None,
                       "confirmed": r.confirmed}
                if len(r.poses):
                    row["found"] = dict(dt_mm=round(float(np.linalg.norm(r.poses[0, 9:] - truth[9:])) * 1e3, 1),
                                        **record(r.assessment.counts[0, 0], r.assessment.verdicts[0, 0], *contour_of(r.assessment, 0)))
                    if contour is not None:
                        hits = np.nonzero(r.assessment.verdicts[:, 0] == SUPPORTED)[0]
                        row["found"]["supported_by_plain_rule"] = int(hits[0]) if hits.size else -1
                out.append(row)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--particles", type=int, default=2000)
    ap.add_argument("--cases", default="m1,m2,m3")
    ap.add_argument("--scene-seeds", default="101,102")
    ap.add_argument("--no-finds", action="store_true")
    ap.add_argument("--contour", action="store_true")
    a = ap.parse_args()
    contour = PoseAssessor.ContourParameters() if a.contour else None
    res = {"tool": "assess_timing", "timing": timing(a.calls, a.frames, a.particles, contour)}
    if not a.no_finds:
        res["finds"] = finds(a.cases.split(","), [int(s) for s in a.scene_seeds.split(",")], contour)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
