"""ctypes wrapper of rbs_test_prep, the rectangles kernel's probe in the TEST build of the library
(dbot_ros_amd/csrc/rbsensor_probes.hip, librbsensor_mi355x_hooks.so).  Every output array is `TAIL` elements (rows) longer than
the kernel may write and filled with a sentinel before the call; the wrapper hands back the whole arrays, so a test sees what
was written, what was left alone and whether the tail still holds the sentinel.  Test infrastructure."""
import ctypes as C

import numpy as np

from filter_probes import RBS_ERR_INVALID_ARGUMENT, RBS_OK, child_outcomes, hooks_path  # noqa: F401  (re-exported)
from prep_twin import MAX_GROUPS, MAX_STRIPS, PREP_PER_BLOCK

PREP_SYMBOLS = ("rbs_test_prep", "rbs_test_prep_layout", "rbs_test_prep_tiles_ub")
TAIL = 5
SENTINEL, ISENTINEL = 7.25, -7
ROUTE_DEVICE, ROUTE_HOST, ROUTE_DELTAS = 0, 1, 2
MAX_BODIES = 16
GROUPS_INTS = 4 + 4 * MAX_GROUPS + MAX_GROUPS + MAX_GROUPS                 # n + padding, rect, first, mask
STRIPS_INTS = 4 + (MAX_STRIPS + 1) + 2 * MAX_STRIPS                        # n + padding, first, box (four 16-bit values each)
assert (4 + MAX_STRIPS + 1) % 2 == 0                                       # (the boxes are 8-byte aligned without padding)

_IN = ("vtx_begin", "vtx")
_OUT = ("poses", "rects", "groups", "strips", "parents", "item_range", "item_particle", "ctr_this", "done", "win_used", "win_dst",
        "reg_dst", "err", "area_sum", "aux", "keep")


class PrepIO(C.Structure):
    _fields_ = ([(k, C.c_int32) for k in ("rows", "cols", "n_bodies", "n")] + [(k, C.c_double) for k in ("fx", "fy", "cx", "cy")] +
                [(k, C.c_void_p) for k in _IN] + [(k, C.c_int32) for k in ("rect_align", "tile_w", "tile_h", "tile_px", "windowed",
                                                                           "slab_px", "slots", "update")] +
                [("win_src", C.c_void_p), ("rebase_box", C.c_void_p), ("route", C.c_int32), ("pad0", C.c_int32),
                 ("poses_in", C.c_void_p), ("indices", C.c_void_p), ("frame", C.c_void_p)] +
                [(k, C.c_double) for k in ("tw", "ms", "sf", "lam")] + [("tail", C.c_int64)] + [(k, C.c_void_p) for k in _OUT])


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def sentinel(shape, dtype):
    return np.full(shape, SENTINEL if np.dtype(dtype).kind == "f" else ISENTINEL, dtype=dtype)


def untouched(a):
    return bool(np.all(a == (SENTINEL if a.dtype.kind == "f" else ISENTINEL)))


def pack_bodies(bodies):
    """list of [nv][3] vertex arrays -> (vtx_begin [B + 1] int32, vtx [sum nv][4] float32)."""
    begin = np.concatenate([[0], np.cumsum([len(b) for b in bodies])]).astype(np.int32)
    vtx = np.zeros((int(begin[-1]), 4), dtype=np.float32)
    vtx[:, :3] = np.concatenate([np.asarray(b, dtype=np.float32).reshape(-1, 3) for b in bodies])
    return begin, vtx


class PrepResult(dict):
    """The arrays of one call, whole (tails included), and views of the particles' records."""
    __getattr__ = dict.__getitem__

    def group_list(self, i):
        """[(rect, mask, first)] of particle i in stored order."""
        g = self["groups"][i]
        return [(tuple(int(k) for k in g[4 + 4 * k:8 + 4 * k]), int(np.uint32(g[4 + 4 * MAX_GROUPS + MAX_GROUPS + k])), int(g[4 + 4 * MAX_GROUPS + k]))
                for k in range(int(g[0]))]

    def strip_list(self, i):
        """(n, first [MAX_STRIPS + 1], box [MAX_STRIPS][4]) of particle i."""
        s = self["strips"][i]
        first = s[4:4 + MAX_STRIPS + 1]
        box = np.ascontiguousarray(s[4 + MAX_STRIPS + 1:]).view(np.uint16).reshape(MAX_STRIPS, 4).astype(np.int32)
        return int(s[0]), first, box


class PrepProbe:
    def __init__(self, path):
        self.lib = C.CDLL(path)
        for s in PREP_SYMBOLS:
            getattr(self.lib, s).restype = C.c_int32
        self.lib.rbs_test_prep_tiles_ub.restype = C.c_int64
        lay = np.zeros(6, dtype=np.int32)
        assert self.lib.rbs_test_prep_layout(_p(lay)) == RBS_OK
        assert lay.tolist() == [4 * GROUPS_INTS, 4 * STRIPS_INTS, MAX_GROUPS, MAX_STRIPS, PREP_PER_BLOCK, MAX_BODIES], lay

    def tiles_ub(self, cols, rows, tile_w, tile_h, tile_px):
        return int(self.lib.rbs_test_prep_tiles_ub(C.c_int32(cols), C.c_int32(rows), C.c_int32(tile_w), C.c_int32(tile_h), C.c_int32(tile_px)))

    def run(self, rows, cols, K, bodies, poses, indices=None, *, route=ROUTE_DEVICE, rect_align=4, tile_w=256, tile_h=4, tile_px=8192,
            windowed=1, slab_px=0, slots=0, win_src=None, rebase_box=None, update=1, groups=False, strips=False, frame=None,
            model=(0.01, 0.003, 0.0014, 0.69), want_aux=True, want_keep=False, area=False, ctr0=(0, 0), err0=(0, 0), expect=RBS_OK):
        """poses: [n][B][12] (routes DEVICE and HOST) or [n + 1][B][6] (DELTAS: the deltas, then the default poses).
        -> PrepResult; tiles_ub is the host's bound for these tile constants."""
        B = len(bodies)
        poses = np.ascontiguousarray(poses, dtype=np.float64)
        n = poses.shape[0] - (1 if route == ROUTE_DELTAS else 0)
        assert poses.shape == ((n + 1, B, 6) if route == ROUTE_DELTAS else (n, B, 12)), poses.shape
        indices = np.zeros(n, dtype=np.int32) if indices is None else np.ascontiguousarray(indices, dtype=np.int32)
        assert indices.shape == (n,)
        begin, vtx = pack_bodies(bodies)
        win_src = None if win_src is None else np.ascontiguousarray(win_src, dtype=np.int32).reshape(slots, 4)
        rebase_box = None if rebase_box is None else np.ascontiguousarray(rebase_box, dtype=np.int32).reshape(4)
        frame = None if frame is None else np.ascontiguousarray(frame, dtype=np.float32).reshape(rows * cols)
        ub = self.tiles_ub(cols, rows, tile_w, tile_h, tile_px)
        assert ub >= 1 or expect != RBS_OK, ub
        ub = max(ub, 1)
        out = PrepResult(
            poses=sentinel(n * B * 12 + TAIL, np.float64), rects=sentinel((n + TAIL, 4), np.int32),
            groups=sentinel((n + TAIL, GROUPS_INTS), np.int32) if groups else None,
            strips=sentinel((n + TAIL, STRIPS_INTS), np.int32) if strips else None,
            parents=sentinel(n + TAIL, np.int32), item_range=sentinel((n + TAIL, 2), np.int32),
            item_particle=sentinel(n * ub * (MAX_GROUPS if groups else 1) + TAIL, np.int32),
            ctr_this=sentinel(2 + TAIL, np.int32), done=sentinel(n + TAIL, np.int32), win_used=sentinel((n + TAIL, 4), np.int32),
            win_dst=sentinel((n + TAIL, 4), np.int32), reg_dst=sentinel((n + TAIL, 4), np.int32), err=sentinel(2 + TAIL, np.int32),
            area_sum=np.zeros(1, dtype=np.uint64) if area else None,
            aux=sentinel((rows * cols + TAIL, 4), np.float64) if frame is not None and want_aux else None,
            keep=sentinel(rows * cols + TAIL, np.float32) if frame is not None and want_keep else None)
        out["ctr_this"][:2] = ctr0
        out["err"][:2] = err0
        io = PrepIO(rows=rows, cols=cols, n_bodies=B, n=n, fx=K[0], fy=K[1], cx=K[2], cy=K[3], rect_align=rect_align, tile_w=tile_w,
                    tile_h=tile_h, tile_px=tile_px, windowed=windowed, slab_px=slab_px, slots=slots, update=update, route=route,
                    tw=model[0], ms=model[1], sf=model[2], lam=model[3], tail=TAIL)
        keepalive = dict(vtx_begin=begin, vtx=vtx, win_src=win_src, rebase_box=rebase_box, poses_in=poses, indices=indices, frame=frame)
        for k, a in list(keepalive.items()) + [(k, out[k]) for k in _OUT]:
            setattr(io, k, _p(a))
        rc = self.lib.rbs_test_prep(C.byref(io))
        assert rc == expect, rc
        out["tiles_ub"], out["n"], out["B"] = ub, n, B
        return out
