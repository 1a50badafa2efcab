"""Planted poses and the reference of the contour rule's GPU tests (tests/test_gpu_contour.py) over the assessor's
scenes (tests/assess_scenes.py): poses whose visible face lies in the synthetic frame's background plane, and counts and
verdicts from the numpy twin (tests/contour_twin.py) on the one-body oracle's planes.  Nothing here needs a device."""
import numpy as np

import assess_scenes as asc
import contour_twin as ct

PARAMS = dict(ct.DEFAULTS)                     # stated, not the library's defaults
OFFSETS_MM = (0, 10, 20, 30)


def wall_depth(s, x):
    """Depth of synth.make_frame's background plane at the image's middle row, at the column where a point (x, 0, ~1.5 m)
    projects."""
    K = s.cam.camera_matrix
    return 1.5 + 0.2 * ((K[0, 0] * x / 1.5 + K[0, 2]) / s.cols - 0.5)


def in_wall(s, off_mm):
    """[B, 12]: body b unrotated at (x_b, 0, wall_depth(x_b) + off), x_b = -0.3 + 0.15 b."""
    p = np.zeros((s.B, 12))
    for b in range(s.B):
        x = -0.3 + 0.15 * b
        p[b, 0] = p[b, 4] = p[b, 8] = 1.0
        p[b, 9:12] = (x, 0.0, wall_depth(s, x) + off_mm * 1e-3)
    return p


def planted(s):
    """name -> pose [B, 12]: the in-wall poses."""
    return {"in wall +%d mm" % off: in_wall(s, off) for off in OFFSETS_MM}


def poses(s):
    """Scene.poses() and the in-wall poses."""
    out = dict(s.poses())
    out.update(planted(s))
    return out


def expect(s, pose, frame=None, sigmas=asc.PARAMS["sigmas"], **params):
    """The twin's contour (counts [B, 5], verdicts [B]) of `pose` against `frame` (None: the scene's)."""
    return ct.contour(s.planes(pose), s.frame if frame is None else frame, s.rows, s.cols, s.ms, s.sf, sigmas=sigmas,
                      **dict(PARAMS, **params))
