"""The scene of the silhouette gate's outcome tests (tests/test_find_gate_cpu.py, tests/test_gpu_find_gate.py): the two-body
scene of DESIGN.md Appendix K on which plain selection puts the visible body into synth.make_frame's slab, and the settings
of tests/test_gpu_scene_find.py's accuracy test."""
import math

import scene_find_scenes as ss

NAMES, COLS, ROWS, SEED, BODY = ("m1", "m2"), 640, 480, 101, 0
# the finder's parameters besides the defaults; with them: step 1b and step 6b at their defaults
FIND = dict(seed_stride=4, sigma_angle=math.radians(25.0), sigma_translation=0.015, rounds=16)


def scene():
    return ss.Scene(NAMES, COLS, ROWS, SEED)


# ---------------------------------------------------------------- the twin chain, every score the eager oracle's
# Body m1's find on the whole frame (it is the first body searched: its residual frame is the frame) with steps 1b and 6b at
# their defaults, once with plain selection and once with the gate at its defaults, as computed on the CPU by twin_find
# (tests/test_find_gate_cpu.py runs it again): pose 0's distance from the truth in metres, its score, its class (the gate
# only), the confirmed finals.
TWIN_PLAIN = dict(distance=0.42342224, score=26456.09)
TWIN_GATED = dict(distance=0.00014385, score=14594.593, cls=0, confirmed_finals=1, confirmed_hypotheses=20301, hypotheses=67584,
                  candidates_near=20)


def _crop_evidence(plane, frame, rows, cols, ms, sf, params):
    """gt.evidence on the covered pixels' bounding box grown by the radius (outside it nothing is covered and nothing has an
    anchor: the counts are those of the whole image)."""
    import numpy as np

    import find_gate_twin as gt
    img = np.asarray(plane, dtype=np.float32).reshape(rows, cols)
    ys, xs = np.nonzero(np.isfinite(img))
    if len(ys) == 0:
        return np.zeros(10, dtype=np.int32), 1
    r = params["radius"]
    y0, y1, x0, x1 = max(ys.min() - r, 0), min(ys.max() + r + 1, rows), max(xs.min() - r, 0), min(xs.max() + r + 1, cols)
    sub = np.ascontiguousarray(img[y0:y1, x0:x1])
    fr = np.ascontiguousarray(np.asarray(frame, dtype=np.float32).reshape(rows, cols)[y0:y1, x0:x1])
    return gt.evidence(sub.ravel(), fr.ravel(), y1 - y0, x1 - x0, ms, sf, **params)


def twin_find(s, gate, b=BODY, threads=None):
    """rbs_find_run's steps for body b of scene s on s.frame in the numpy twins (steps 1b and 6b at their defaults, FIND),
    gate: None (plain selection) or a dict of the gate's fields.  -> dict(poses, scores, classes, found, hypotheses,
    confirmed_hypotheses)."""
    import types
    from concurrent.futures import ThreadPoolExecutor

    import numpy as np

    import find_fg_twin as fg
    import find_gate_twin as gt
    import find_refine_twin as rf
    import find_twin as tw
    import scenarios as sc
    import scene_find_twin as st
    from dbot_ros_amd import CameraData
    threads = threads or sc.usable_threads()
    p = types.SimpleNamespace(coarse_downsampling=0, seed_stride=4, min_depth=0.2, max_depth=3.0, depth_offset=-1.0, max_seeds=1024,
                              n_rotations=1024, n_candidates=512, nms_translation=0.02, nms_angle=np.radians(30.0), n_survivors=32,
                              rounds=8, children=64, sigma_translation=0.01, sigma_angle=np.radians(10.0), decay=0.6, seed=0,
                              min_score=-np.inf)
    for k, v in FIND.items():
        setattr(p, k, v)
    frame, rows, cols = s.frame, s.rows, s.cols
    f = tw.coarse_factor(cols, p.coarse_downsampling)
    coarse, cr, cc = tw.subsample(frame, rows, cols, f)
    Kc = tw.coarse_K(s.K, f)
    _, seed_frame = fg.foreground(coarse.ravel(), cr, cc, p.min_depth, p.max_depth, s.ms, s.sf, p.seed, **ss.FOREGROUND)
    seeds, _ = tw.seeds(np.asarray(seed_frame).reshape(cr, cc), p.seed_stride, p.min_depth, p.max_depth, p.max_seeds)
    hyp = tw.hypotheses(seeds, p.n_rotations, Kc, st.mean_vertex_distance(s.om.vertices[b]))
    H = len(hyp)
    ccam = CameraData(Kc, cr, cc)
    hs = np.asarray(ss._scores(s.part_oracle(b, H, ccam), coarse.ravel(), hyp, threads))
    cls = np.ones(H, dtype=np.int64)
    params = dict(gt.DEFAULTS, **(gate or {}))
    params = {k: params[k] for k in gt.DEFAULTS}
    if gate is not None:
        def chunk(idx):
            o = s.part_oracle(b, 1, ccam)
            out = []
            for h in idx:
                d = o.render_depth(hyp[h])
                out.append(_crop_evidence(np.where(np.isfinite(d), d, np.inf), coarse, cr, cc, s.ms, s.sf, params)[1])
            o.close()
            return out
        with ThreadPoolExecutor(threads) as ex:
            cls = np.concatenate(list(ex.map(chunk, np.array_split(np.arange(H), threads * 8))))
        cand = gt.gated_topk(hs, cls, p.n_candidates)[1]
    else:
        cand = tw.select_order(hs)[: p.n_candidates]
    kept = tw.nms(hyp[cand], p.nms_translation, p.nms_angle, p.n_survivors)
    cur = hyp[cand][kept]
    full = s.part_oracle(b, p.n_survivors * p.children)
    cur, best, _ = rf.refine(cur, lambda q: ss._scores(full, frame, q, threads), p.rounds, p.children, p.seed, p.sigma_angle,
                             p.sigma_translation, **{k: v for k, v in rf.DEFAULTS.items()})
    fcls = np.ones(len(cur), dtype=np.int64)
    if gate is not None:
        fcls = np.array([_crop_evidence(s.plane(b, q), frame, rows, cols, s.ms, s.sf, params)[1] for q in cur])
        o = gt.result_order(best, fcls)
        found = gt.found(best, fcls, o, p.min_score, bool(gate.get("require_confirmed")))
    else:
        o = tw.result_order(best)
        found = bool(best[o[0]] >= p.min_score)
    near = np.linalg.norm(hyp[cand][:, 9:] - s.truth[b, 9:], axis=1) < 0.03
    return dict(poses=cur[o], scores=best[o], classes=fcls[o], found=found, hypotheses=H, confirmed_hypotheses=int((cls == 0).sum()),
                candidates_near=int(near.sum()))
