"""Time per find of the object finder (rbs_find_*) on one device, per stage, beside the CPU oracle's cost of the same
scoring.  Prints ONE JSON line:

    {"tool": "find_object_timing", "cases": [{"case", "size", "coarse", "hypotheses", "children", "ms_per_find",
      "stage_ms": {"frame_seeds", "coarse", "selection", "refinement"}, "hypotheses_per_s", "oracle_s",
      "found": {"dt_mm", "iou", "score", "truth_score"}, "nearest_candidate": {"dt_mm", "deg"},
      "nearest_survivor": {"dt_mm", "deg"}, "scene_seed", "seed_stride", "foreground", "plane": {...} | null,
      "refinement", "rounds", "sigma_angle_deg", "sigma_translation",
      "seeds_by_label": {"plane", "object", "occluder"}, "meets_bar"}, ...]}

Cases: M1, M2, M3 at 640x480 and M4 at 1280x960, the header's default parameters; one synth.make_frame frame per case
(background plane, occluder, noise, 5 % NaN) with the object at a seeded random rotation, z in 0.55-0.9 m.
ms_per_find: host clock around rbs_find_run, averaged over the timed finds (after a warm-up find); stage_ms: the
library's HIP events of the last find.  oracle_s: the CPU oracle's (EAGER, one core) time per pose at the coarse
resolution, measured on --oracle-poses poses, times the hypothesis count, plus the same at full resolution times the
refinement's children.  nearest_candidate / nearest_survivor: the coarse stage's closest pose to the truth (translation,
then rotation angle of that pose) -- whether the search had the object in hand before the refinement.
--foreground switches step 1b on (the library's default setting) and --seed-stride sets seed_stride; --scene-seeds lists the
scenes' seeds (the accuracy bar's six scenes: --cases m1,m2,m3 --scene-seeds 101,102).  plane: the dominant plane the find
took away (rbs_find_get_plane); seeds_by_label: the find's seeds on the background plane, the object and the occluder (labels
from the noise-free scene); meets_bar: translation < 1 cm, IoU >= 0.85, score >= 0.98 x the truth's.  --oracle-poses 0 skips
the oracle's timing.  --refinement switches step 6b on (the library's default setting); --sigma-angle (degrees),
--sigma-translation (metres) and --rounds set the search's start and length for either refinement.
--gate switches the silhouette gate on (the library's default setting; --require-confirmed: found needs a confirmed pose 0);
a case then carries "gate": the confirmed hypotheses / candidates / finals and the evidence kernel's two times (step 4b's lie
inside stage_ms "coarse", step 7's inside "refinement"); per body for a scene, with the body's nearest candidate.
Usage: python tools/find_object_timing.py [--finds N] [--oracle-poses P] [--cases m1,m2,m3,m4] [--foreground] [--seed-stride S]
                                          [--scene-seeds 101,102] [--refinement] [--sigma-angle DEG] [--sigma-translation M]
                                          [--rounds R] [--gate [--require-confirmed]]
--objects m1,m2,m3 times the SCENE finder (rbs_find_scene_*) instead: one scene of those meshes placed apart at 640x480 per
scene seed (tests/scene_find_scenes.py), the same switches for every body's find, --explain-radius / --polish-sweeps for the
scene finder's own parameters.  Its cases: {"case", "size", "ms_per_scene_find", "stage_ms": {"per_body", "render",
"residual", "polish", "whole"}, "order", "found", "bodies": [{"dt_mm", "iou", "score"}], "joint_score", "truth_joint_score",
"meets_bar", ...}.
"""
import os

for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):   # the oracle: one core
    os.environ[_v] = "1"

import argparse  # noqa: E402
import json  # noqa: E402
import math  # noqa: E402
import sys  # noqa: E402
import time  # noqa: E402

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import oracle_binding as ob  # noqa: E402
import scenarios as sc  # noqa: E402
from dbot_ros_amd import CameraData, RbSensor, synth  # noqa: E402
from dbot_ros_amd.finder import ObjectFinder  # noqa: E402
from dbot_ros_amd.pose import quat_to_matrix  # noqa: E402

CASES = {"m1": ("m1", 640, 480), "m2": ("m2", 640, 480), "m3": ("m3", 640, 480), "m4": ("m4", 1280, 960)}


def scene(sensor, cam, seed):
    rng = np.random.default_rng(seed)
    q = rng.normal(size=4)
    R = quat_to_matrix(q / np.linalg.norm(q))
    z = rng.uniform(0.55, 0.9)
    K = cam.camera_matrix
    u, v = rng.uniform(0.3, 0.7) * cam.cols, rng.uniform(0.3, 0.7) * cam.rows
    truth = np.concatenate([R.ravel(), [(u - K[0, 2]) / K[0, 0] * z, (v - K[1, 2]) / K[1, 1] * z, z]])
    d = sensor.render_depth(truth)
    d = np.where(np.isfinite(d), d, np.inf)
    return truth, synth.make_frame(d, cam.rows, cam.cols, rng), scene_labels(d, cam.rows, cam.cols)


def scene_labels(d, rows, cols):
    """0 background plane, 1 object, 2 occluder, from the noise-free scene."""
    clean = synth.make_frame(d, rows, cols, None, noise=False, nan_frac=0).reshape(rows, cols)
    bare = synth.make_frame(d, rows, cols, None, noise=False, nan_frac=0, occluder=False).reshape(rows, cols)
    lab = np.zeros((rows, cols), dtype=np.int8)
    lab[np.isfinite(d.reshape(rows, cols))] = 1
    lab[clean != bare] = 2
    return lab


def nearest(poses, truth):
    if len(poses) == 0:
        return None
    dt = np.linalg.norm(poses[:, 9:] - truth[9:], axis=1)
    i = int(np.argmin(dt))
    c = (np.trace(poses[i, :9].reshape(3, 3).T @ truth[:9].reshape(3, 3)) - 1.0) / 2.0
    return {"dt_mm": round(float(dt[i]) * 1e3, 2), "deg": round(math.degrees(math.acos(max(-1.0, min(1.0, c)))), 1)}


def oracle_s_per_pose(om, K, rows, cols, P, frame, poses):
    o = ob.Oracle(om, CameraData(K, rows, cols), P, max_particles=len(poses), mode=ob.EAGER)
    o.reset()
    o.set_observation(np.asarray(frame, dtype=np.float64))
    t0 = time.perf_counter()
    o.loglikes_poses(poses.reshape(len(poses), 1, 12), np.zeros(len(poses), dtype=np.int32), update=False)
    s = (time.perf_counter() - t0) / len(poses)
    o.close()
    return s


def gate_of(gate, require_confirmed):
    return ObjectFinder.Gate(require_confirmed=bool(require_confirmed)) if gate else None


def gate_report(fnd):
    """The gate's figures of fnd's last find: confirmed hypotheses / candidates / finals and the evidence kernel's two times."""
    ms = fnd.gate_ms()
    return {"confirmed": {st: int((fnd.evidence(st)[1] == 0).sum()) for st in ("coarse", "candidates", "result")},
            "evidence_ms": {"step_4b": round(ms[0], 3), "step_7": round(ms[1], 3)}}


def run_case(name, finds, oracle_poses, seed=101, foreground=False, seed_stride=None, refinement=False, sigma_angle=None,
             sigma_translation=None, rounds=None, gate=False, require_confirmed=False):
    mesh, cols, rows = CASES[name]
    om, cam, P = sc.make_scene((mesh,), cols, rows, max_particles=1)
    with RbSensor(om, cam, P, max_particles=1) as sensor:
        truth, frame, labels = scene(sensor, cam, seed)
        p = ObjectFinder.Parameters()
        if seed_stride:
            p.seed_stride = seed_stride
        if sigma_angle is not None:
            p.sigma_angle = math.radians(sigma_angle)
        if sigma_translation is not None:
            p.sigma_translation = sigma_translation
        if rounds is not None:
            p.rounds = rounds
        with ObjectFinder(sensor, om, p, foreground=ObjectFinder.Foreground() if foreground else None,
                          refinement=ObjectFinder.Refinement() if refinement else None, gate=gate_of(gate, require_confirmed)) as fnd:
            fnd.find(frame)                                       # warm-up
            t0 = time.perf_counter()
            for _ in range(finds):
                r = fnd.find(frame)
            ms = (time.perf_counter() - t0) / finds * 1e3
            st = fnd.stage_ms()
            seeds, _, _, info = fnd.stage("seeds")
            plane = fnd.plane()._asdict() if foreground else None
            gated = gate_report(fnd) if gate else None
            cp, _, _, _ = fnd.stage("candidates")
            sp, _, _, _ = fnd.stage("survivors")
            kp, _, _, _ = fnd.stage("children", p.rounds - 1) if p.rounds else (np.zeros((0, 12)),) * 4
        crows, ccols, f, hyp = int(info[0]), int(info[1]), int(info[2]), int(info[3])
        best = r.poses[0] if len(r.poses) else None
        d_best, d_truth = sensor.render_depth(best) if best is not None else None, sensor.render_depth(truth)
    with RbSensor(om, cam, P, max_particles=1024) as ref:
        ref.reset()
        ref.set_observation(frame)
        truth_score = float(ref.loglikes_poses(np.repeat(truth[None], 1024, 0), np.zeros(1024, dtype=np.int32))[0])
    Kc = cam.camera_matrix.copy()
    Kc[:2] /= f
    coarse = frame.reshape(rows, cols)[: crows * f: f, : ccols * f: f].ravel()
    per_coarse = per_full = 0.0
    if oracle_poses > 0:
        sample = cp[:oracle_poses] if len(cp) else np.repeat(truth[None], oracle_poses, 0)
        per_coarse = oracle_s_per_pose(om, Kc, crows, ccols, P, coarse, sample)
        per_full = oracle_s_per_pose(om, cam.camera_matrix, rows, cols, P, frame, kp[: max(1, oracle_poses // 4)]) if len(kp) else 0.0
    seed_labels = labels[: crows * f: f, : ccols * f: f].ravel()[seeds[:, 3].astype(np.int64)] if len(seeds) else np.zeros(0, dtype=np.int8)
    children = p.n_survivors * p.children * p.rounds
    found = None
    if best is not None:
        a, b = np.isfinite(d_best), np.isfinite(d_truth)
        found = {"dt_mm": round(float(np.linalg.norm(best[9:] - truth[9:])) * 1e3, 2),
                 "iou": round(float((a & b).sum() / max((a | b).sum(), 1)), 3),
                 "score": round(float(r.scores[0]), 1), "truth_score": round(truth_score, 1)}
    meets = bool(found and found["dt_mm"] < 10.0 and found["iou"] >= 0.85 and r.scores[0] >= truth_score - 0.02 * abs(truth_score))
    return {"case": name, "size": [cols, rows], "coarse": [ccols, crows], "hypotheses": hyp, "children": children,
            "ms_per_find": round(ms, 2),
            "stage_ms": dict(zip(("frame_seeds", "coarse", "selection", "refinement"), (round(x, 3) for x in st[:4]))),
            "hypotheses_per_s": round(hyp / (st[1] * 1e-3)) if st[1] > 0 else None,
            "oracle_s": round(per_coarse * hyp + per_full * children, 1),
            "found": found, "nearest_candidate": nearest(cp, truth), "nearest_survivor": nearest(sp, truth),
            "scene_seed": seed, "seed_stride": p.seed_stride, "foreground": bool(foreground), "plane": plane,
            "refinement": bool(refinement), "rounds": p.rounds, "sigma_angle_deg": round(math.degrees(p.sigma_angle), 3),
            "sigma_translation": p.sigma_translation, "gate": gated, "require_confirmed": bool(gate and require_confirmed),
            "found_flag": bool(r.found),
            "seeds_by_label": dict(zip(("plane", "object", "occluder"), (int((seed_labels == k).sum()) for k in range(3)))),
            "meets_bar": meets}


def run_scene(names, finds, seed=101, foreground=False, seed_stride=None, refinement=False, sigma_angle=None, sigma_translation=None,
              rounds=None, explain_radius=None, polish_sweeps=None, gate=False, require_confirmed=False):
    import scene_find_scenes as ss
    from dbot_ros_amd.assess import PoseAssessor
    from dbot_ros_amd.finder import SceneFinder
    s = ss.Scene(names, 640, 480, seed)
    p = ObjectFinder.Parameters()
    if seed_stride:
        p.seed_stride = seed_stride
    if sigma_angle is not None:
        p.sigma_angle = math.radians(sigma_angle)
    if sigma_translation is not None:
        p.sigma_translation = sigma_translation
    if rounds is not None:
        p.rounds = rounds
    sp = SceneFinder.Parameters()
    if explain_radius is not None:
        sp.explain_radius = explain_radius
    if polish_sweeps is not None:
        sp.polish_sweeps = polish_sweeps
    with RbSensor(s.om, s.cam, s.P, max_particles=1) as sensor:
        with SceneFinder(sensor, s.om, p, sp, foreground=ObjectFinder.Foreground() if foreground else None,
                         refinement=ObjectFinder.Refinement() if refinement else None, gate=gate_of(gate, require_confirmed)) as fnd:
            fnd.find(s.frame)                                     # warm-up
            t0 = time.perf_counter()
            for _ in range(finds):
                r = fnd.find(s.frame)
            ms = (time.perf_counter() - t0) / finds * 1e3
            per_body, render, residual, polish, whole = fnd.stage_ms()
            order, _ = fnd.order()
            gated = None
            if gate:   # per searched body: the gate's figures, the coarse stage's time beside them, the nearest candidate
                gated = []
                for b in range(s.B):
                    body = fnd.body_finder(b)
                    gated.append(dict(gate_report(body), coarse_ms=round(body.stage_ms()[1], 3),
                                      nearest_candidate=nearest(body.stage("candidates")[0], s.truth[b])))
        a = PoseAssessor(sensor)

        def planes(poses):
            a.assess(np.asarray(poses)[None])
            return [np.isfinite(a.plane(0, b)) for b in range(s.B)]
        posed = np.isfinite(r.poses).all()
        got, want = planes(np.where(np.isfinite(r.poses), r.poses, s.truth)), planes(s.truth)
    with RbSensor(s.om, s.cam, s.P, max_particles=1024) as ref:
        ref.reset()
        ref.set_observation(s.frame)
        truth_score = float(ref.loglikes_poses(np.repeat(s.truth[None], 1024, 0), np.zeros(1024, dtype=np.int32))[0])
    bodies = [{"dt_mm": round(float(np.linalg.norm(r.poses[b, 9:] - s.truth[b, 9:])) * 1e3, 2),
               "iou": round(float((got[b] & want[b]).sum() / max((got[b] | want[b]).sum(), 1)), 3),
               "score": round(float(r.scores[b]), 1)} for b in range(s.B)]
    meets = bool(posed and all(b["dt_mm"] < 10.0 and b["iou"] >= 0.85 for b in bodies) and
                 r.joint_score >= truth_score - 0.02 * abs(truth_score))
    return {"case": "+".join(names), "size": [640, 480], "ms_per_scene_find": round(ms, 2),
            "stage_ms": {"per_body": [round(x, 3) for x in per_body], "render": round(render, 4), "residual": round(residual, 4),
                         "polish": round(polish, 3), "whole": round(whole, 3)},
            "order": order, "found": [bool(x) for x in r.found], "bodies": bodies,
            "joint_score": round(float(r.joint_score), 1), "truth_joint_score": round(truth_score, 1), "meets_bar": meets,
            "scene_seed": seed, "seed_stride": p.seed_stride, "foreground": bool(foreground), "refinement": bool(refinement),
            "rounds": p.rounds, "sigma_angle_deg": round(math.degrees(p.sigma_angle), 3), "sigma_translation": p.sigma_translation,
            "explain_radius": sp.explain_radius, "polish_sweeps": sp.polish_sweeps, "gate": gated,
            "require_confirmed": bool(gate and require_confirmed)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--finds", type=int, default=5)
    ap.add_argument("--oracle-poses", type=int, default=16)
    ap.add_argument("--cases", default="m1,m2,m3,m4")
    ap.add_argument("--foreground", action="store_true")
    ap.add_argument("--seed-stride", type=int, default=0)
    ap.add_argument("--scene-seeds", default="101")
    ap.add_argument("--refinement", action="store_true")
    ap.add_argument("--sigma-angle", type=float, default=None, help="degrees")
    ap.add_argument("--sigma-translation", type=float, default=None, help="metres")
    ap.add_argument("--rounds", type=int, default=None)
    ap.add_argument("--objects", default="", help="meshes of one scene, e.g. m1,m2,m3: time the scene finder")
    ap.add_argument("--explain-radius", type=int, default=None)
    ap.add_argument("--polish-sweeps", type=int, default=None)
    ap.add_argument("--gate", action="store_true", help="the silhouette gate at the library's defaults")
    ap.add_argument("--require-confirmed", action="store_true", help="with --gate: found needs a confirmed pose 0")
    a = ap.parse_args()
    if a.objects:
        cases = [run_scene(tuple(a.objects.split(",")), a.finds, int(s), a.foreground, a.seed_stride, a.refinement, a.sigma_angle,
                           a.sigma_translation, a.rounds, a.explain_radius, a.polish_sweeps, a.gate, a.require_confirmed) for s in a.scene_seeds.split(",")]
        print(json.dumps({"tool": "find_object_timing", "cases": cases}))
        return
    cases = [run_case(c, a.finds, a.oracle_poses, int(s), a.foreground, a.seed_stride, a.refinement, a.sigma_angle, a.sigma_translation,
                      a.rounds, a.gate, a.require_confirmed) for c in a.cases.split(",")
             for s in a.scene_seeds.split(",")]
    print(json.dumps({"tool": "find_object_timing", "cases": cases}))


if __name__ == "__main__":
    main()
