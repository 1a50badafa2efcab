"""Time and effect of the pose refiner (rbs_refine_*) on one device.  Prints ONE JSON line:

    {"tool": "refine_timing",
     "timing": [{"n", "iters", "ms_per_call", "stage_ms": {"render", "accumulate", "solve"}, "statuses", "iterations", "counts"}, ...],
     "finder": [{"case", "scene_seed", "rounds", "ms_per_find", "ms_per_find_refined", "refine_kernel_ms",
                 "found": {"dt_mm", "deg", "iou", "score"}, "refined": {"dt_mm", "deg", "iou", "score"}, "truth_score",
                 "status", "iterations", "counts"}, ...]}

timing: M1 at 640 x 480 (tools/find_object_timing.py's scene 101), n = 1 and n = 32 poses 5 mm and 5 degrees beside the
truth (the 32: further turned by up to 2 degrees each, seeded), the library's default parameters with --iters iterations:
ms_per_call is the host clock around rbs_refine_poses (median of --calls calls after a warm-up; upload, every launch, the
copy and the synchronisation included), stage_ms the library's HIP events summed over the iterations (median likewise).
finder: the accuracy bar's six scenes (m1, m2, m3 x scene seeds 101, 102: find_object_timing.py --foreground --refinement)
at --rounds rounds each, the finder alone and with the refiner behind it (ObjectFinder.find(refine=...)): pose 0's error
against the truth, IoU of its silhouette with the truth's and its log-likelihood at the sensor's resolution, and the host
clock per find (median of --finds after a warm-up).
Usage: python tools/refine_timing.py [--calls N] [--finds N] [--iters I] [--rounds 4,8,16] [--skip-finder]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import scenarios as sc  # noqa: E402
from dbot_ros_amd import RbSensor  # noqa: E402
from dbot_ros_amd.finder import ObjectFinder  # noqa: E402
from dbot_ros_amd.pose import rotvec_to_matrix  # noqa: E402
from dbot_ros_amd.refine import STATUSES, PoseRefiner  # noqa: E402
from find_object_timing import CASES, scene  # noqa: E402


def moved(pose, dt, rv):
    """pose [12] turned by the rotation vector rv about its own origin and moved by dt."""
    R = rotvec_to_matrix(np.asarray(rv, dtype=np.float64)) @ pose[:9].reshape(3, 3)
    return np.concatenate([R.ravel(), pose[9:] + np.asarray(dt)])


def errors(pose, truth):
    c = (np.trace(pose[:9].reshape(3, 3) @ truth[:9].reshape(3, 3).T) - 1.0) / 2.0
    return float(np.linalg.norm(pose[9:] - truth[9:])) * 1e3, math.degrees(math.acos(max(-1.0, min(1.0, c))))


def timing(calls, iters):
    mesh, cols, rows = CASES["m1"]
    om, cam, P = sc.make_scene((mesh,), cols, rows, max_particles=1)
    out = []
    with RbSensor(om, cam, P, max_particles=1) as sensor:
        truth, frame, _ = scene(sensor, cam, 101)
        rng = np.random.default_rng(5)
        axis = np.ones(3) / math.sqrt(3.0)
        start = moved(truth, (0.005, -0.005, 0.005), axis * math.radians(5.0))
        ref = PoseRefiner(sensor, PoseRefiner.Parameters(iters=iters))
        for n in (1, 32):
            poses = np.stack([start] + [moved(start, (0.0, 0.0, 0.0), rng.normal(size=3) * math.radians(2.0) / math.sqrt(3.0)) for _ in range(n - 1)])
            ref.refine(poses[:, None], frame)                      # warm-up: the buffers are allocated here
            wall, stages = [], []
            for _ in range(calls):
                t0 = time.perf_counter()
                _, rec = ref.refine(poses[:, None], frame)
                wall.append((time.perf_counter() - t0) * 1e3)
                stages.append(ref.kernel_ms())
            st = np.median(np.array(stages), axis=0)
            out.append({"n": n, "iters": iters, "ms_per_call": round(float(np.median(wall)), 3),
                        "ms_per_call_min_max": [round(float(min(wall)), 3), round(float(max(wall)), 3)],
                        "stage_ms": dict(zip(("render", "accumulate", "solve"), (round(float(x), 4) for x in st))),
                        "statuses": {STATUSES[k]: int((rec.status == k).sum()) for k in range(4)},
                        "iterations": [int(rec.iterations.min()), int(rec.iterations.max())],
                        "counts": [int(rec.counts[..., 1].min()), int(rec.counts[..., 1].max())]})
    return out


def finder(finds, rounds_list, iters):
    out = []
    for name in ("m1", "m2", "m3"):
        mesh, cols, rows = CASES[name]
        om, cam, P = sc.make_scene((mesh,), cols, rows, max_particles=1)
        for seed in (101, 102):
            with RbSensor(om, cam, P, max_particles=1) as sensor, RbSensor(om, cam, P, max_particles=1024) as scorer:
                truth, frame, _ = scene(sensor, cam, seed)
                scorer.reset()
                scorer.set_observation(frame)

                def score(pose):
                    return float(scorer.loglikes_poses(np.repeat(pose[None], 1024, 0), np.zeros(1024, dtype=np.int32))[0])

                def report(pose):
                    a, b = np.isfinite(sensor.render_depth(pose)), np.isfinite(sensor.render_depth(truth))
                    dt, deg = errors(pose, truth)
                    return {"dt_mm": round(dt, 3), "deg": round(deg, 2), "iou": round(float((a & b).sum() / max((a | b).sum(), 1)), 3),
                            "score": round(score(pose), 1)}
                truth_score = round(score(truth), 1)
                ref = PoseRefiner(sensor, PoseRefiner.Parameters(iters=iters))
                for rounds in rounds_list:
                    p = ObjectFinder.Parameters()
                    p.rounds = rounds
                    with ObjectFinder(sensor, om, p, foreground=ObjectFinder.Foreground(), refinement=ObjectFinder.Refinement()) as fnd:
                        fnd.find(frame, refine=ref)                # warm-up of both
                        plain, refined = [], []
                        for _ in range(finds):
                            t0 = time.perf_counter()
                            r0 = fnd.find(frame)
                            plain.append((time.perf_counter() - t0) * 1e3)
                            t0 = time.perf_counter()
                            r = fnd.find(frame, refine=ref)
                            refined.append((time.perf_counter() - t0) * 1e3)
                        case = {"case": name, "scene_seed": seed, "rounds": rounds, "ms_per_find": round(float(np.median(plain)), 3),
                                "ms_per_find_refined": round(float(np.median(refined)), 3), "truth_score": truth_score,
                                "n_refined": 0 if r.refined is None else len(r.refined)}
                        if len(r.poses):
                            case.update(found=report(r0.poses[0]), refined=report(r.refined[0]),
                                        refine_kernel_ms=[round(x, 4) for x in ref.kernel_ms()],
                                        status=STATUSES[int(r.refinement.status[0, 0])], iterations=int(r.refinement.iterations[0, 0]),
                                        counts=r.refinement.counts[0, 0].tolist())
                        out.append(case)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--finds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", default="4,8,16")
    ap.add_argument("--skip-finder", action="store_true")
    a = ap.parse_args()
    res = {"tool": "refine_timing", "timing": timing(a.calls, a.iters)}
    if not a.skip_finder:
        res["finder"] = finder(a.finds, [int(r) for r in a.rounds.split(",")], a.iters)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
