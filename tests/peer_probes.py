"""ctypes wrapper of rbs_test_peer_scratch, the probe of resampling across processes in the TEST build of the library
(dbot_ros_amd/csrc/rbsensor_probes.hip, librbsensor_mi355x_hooks.so): what the last rbs_peer_resample call on a handle left in its
scratch block -- the cumulative weights inside each tile, the tiles' maxima (large jobs) and totals, the rank's parents.  The probe
launches nothing.  Also the one way the device tests make a call: outputs filled with a sentinel, every array handed back.
Test infrastructure."""
import ctypes as C

import numpy as np
import torch

from filter_probes import child_outcomes, hooks_path  # noqa: F401

PEER_SYMBOLS = ("rbs_test_peer_scratch",)
RBS_OK, RBS_ERR_INVALID_ARGUMENT, RBS_ERR_HIP, RBS_ERR_UNSUPPORTED = 0, -1, -4, -5
TILE = 2048
SENTINEL, ISENTINEL = 7.25, -7


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class PeerProbe:
    def __init__(self, path):
        self.lib = C.CDLL(path)
        self.lib.rbs_test_peer_scratch.restype = C.c_int32

    def raw(self, handle, cdf, tile_max, tile_total, mine):
        return self.lib.rbs_test_peer_scratch(handle, cdf, tile_max, tile_total, mine)

    def scratch(self, sensor, N, n):
        """-> dict(cdf [N], tile_max [tiles] or None where the call did not write it, tile_total [tiles], mine [n])."""
        tiles = (N + TILE - 1) // TILE
        cdf, tmax, ttot = np.full(N, SENTINEL), np.full(tiles, SENTINEL), np.full(tiles, SENTINEL)
        mine = np.full(n, ISENTINEL, dtype=np.int32)
        rc = self.raw(C.c_void_p(sensor._h.value), _p(cdf), _p(tmax), _p(ttot), _p(mine))
        assert rc in (0, 1), rc
        assert rc == 1 or bool(np.all(tmax == SENTINEL))
        return dict(cdf=cdf, tile_max=tmax if rc == 1 else None, tile_total=ttot, mine=mine)


class PeerCall:
    """One job's device arrays, uploaded once; run(rank) makes the call `repeats` times into sentinel-filled outputs."""

    def __init__(self, sensor, ll, u_sorted, n, temperature=1.0, min_share=2):
        self.s, self.N, self.n, self.T, self.min_share = sensor, int(np.size(ll)), n, temperature, min_share
        self.d_ll = torch.from_numpy(np.ascontiguousarray(ll, dtype=np.float64)).cuda()
        self.d_u = torch.from_numpy(np.ascontiguousarray(u_sorted, dtype=np.float64)).cuda()

    def outputs(self):
        return [torch.full((self.n,), ISENTINEL, dtype=torch.int32, device="cuda") for _ in range(4)], \
            torch.zeros(4, dtype=torch.int64, device="cuda")

    def run(self, rank, repeats=1, min_share=None):
        """-> parent_idx, stage_src, stage_dst, parents_local [n] int32 and counts [4] int64, as numpy arrays."""
        out, counts = self.outputs()
        for _ in range(repeats):
            self.s.peer_resample(self.d_ll.data_ptr(), self.d_u.data_ptr(), self.N, self.n, rank, self.min_share if min_share is None else min_share,
                                 self.T, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), counts.data_ptr())
        self.s.synchronize()
        torch.cuda.synchronize()
        return [o.cpu().numpy() for o in out] + [counts.cpu().numpy()]
