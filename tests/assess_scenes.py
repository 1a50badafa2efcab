"""Scenes, poses and the reference of the pose assessor's GPU tests (tests/test_gpu_assess.py): per-body depth planes
from one-body oracles (oracle/rbsensor_oracle.c renders), counts and verdicts from the numpy twin (tests/assess_twin.py).
Nothing here needs a device."""
import numpy as np

import assess_twin as tw
import oracle_binding as ob
import scenarios as sc
from dbot_ros_amd import ObjectModel, synth

# the smallest sizes that still take each path: one tile; cols % 4 != 0 and several tiles; three bodies; full size
SCENES = {"m1_80": (("m1",), 80, 60), "m1m2_161": (("m1", "m2"), 161, 121), "m1m2m3_322": (("m1", "m2", "m3"), 322, 241),
          "m1_640": (("m1",), 640, 480)}
PARAMS = dict(sigmas=3.0, min_support_fraction=0.5, min_visible_fraction=0.25, min_pixels=16)   # stated, not the library's defaults


class Scene:
    def __init__(self, meshes, cols, rows):
        self.meshes, self.cols, self.rows = meshes, cols, rows
        self.om, self.cam, self.P = sc.make_scene(meshes, cols, rows, max_particles=1)
        self.B = len(meshes)
        self.orc = ob.Oracle(self.om, self.cam, self.P, max_particles=1, mode=ob.EAGER)
        self.parts = []      # the oracle of every part as a one-body model
        for b in range(self.B):
            om1 = ObjectModel([self.om.vertices[b]], [self.om.triangles[b]], center=False)
            self.parts.append(ob.Oracle(om1, self.cam, self.P, max_particles=1, mode=ob.EAGER))
        (truth, frame), = sc.make_frames(self.orc, self.B, 1, seed=3)
        self.truth = np.asarray(truth, dtype=np.float64).reshape(self.B, 12)
        self.frame = np.asarray(frame, dtype=np.float32)
        self.ms, self.sf = self.P.kinect.model_sigma, self.P.kinect.sigma_factor
        self._planes = {}

    def close(self):
        for o in [self.orc] + self.parts:
            o.close()

    def planes(self, pose):
        """[B, npx] float32: every body of `pose` [B, 12] rendered alone by its one-body oracle (cached)."""
        pose = np.ascontiguousarray(pose, dtype=np.float64).reshape(self.B, 12)
        key = pose.tobytes()
        if key not in self._planes:
            self._planes[key] = np.stack([self.parts[b].render_depth(pose[b]) for b in range(self.B)])
        return self._planes[key]

    def expect(self, pose, frame=None, **params):
        """The twin's (counts [B, 5], verdicts [B]) of `pose` against `frame` (None: the scene's)."""
        return tw.assess(self.planes(pose), self.frame if frame is None else frame, self.ms, self.sf, **dict(PARAMS, **params))

    def shifted(self, dx=0.0, dy=0.0, dz=0.0):
        p = self.truth.copy()
        p[:, 9] += dx
        p[:, 10] += dy
        p[:, 11] += dz
        return p

    def at(self, x, y, z):
        """Every body's centre at (x, y, z), rotations as at the truth."""
        p = self.truth.copy()
        p[:, 9:12] = (x, y, z)
        return p

    def poses(self):
        """name -> pose [B, 12]: the cases the counts are held to."""
        K = self.cam.camera_matrix
        z = 0.7
        left, right = (0 - K[0, 2]) / K[0, 0] * z, (self.cols - 1 - K[0, 2]) / K[0, 0] * z
        top, bottom = (0 - K[1, 2]) / K[1, 1] * z, (self.rows - 1 - K[1, 2]) / K[1, 1] * z
        out = {"truth": self.truth.copy(), "x+8cm": self.shifted(dx=0.08), "z+2cm": self.shifted(dz=0.02),
               "left border": self.at(left, 0.0, z), "right border": self.at(right, 0.0, z),
               "top border": self.at(0.0, top, z), "bottom border": self.at(0.0, bottom, z),
               "corner": self.at(left, top, z),
               "off screen": self.shifted(dx=5.0), "behind the camera": self.shifted(dz=-1.5),
               "fills the image": self.at(0.0, 0.0, 0.11)}
        if self.B > 1:   # body 1 half behind body 0
            p = self.truth.copy()
            p[1, 9:12] = p[0, 9:12] + np.array([0.035, 0.0, 0.06])
            out["half behind"] = p
        return out


def truth_state(om, Rt):
    """Absolute pose (R | t of the centred mesh frame) of a one-body scene -> tracker State in the caller's mesh frame."""
    from dbot_ros_amd.pose import matrix_to_rotvec
    Rt = np.asarray(Rt).reshape(12)
    R = Rt[:9].reshape(3, 3)
    s = np.zeros(12)
    s[0:3] = Rt[9:] - R @ om.centers[0]
    s[3:6] = matrix_to_rotvec(R)
    return s
