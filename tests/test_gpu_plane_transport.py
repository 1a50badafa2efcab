"""The occlusion planes' entry points, one at a time and on every storage layout: rbs_get_occlusion / rbs_set_occlusion,
rbs_occlusion_device_ptr / rbs_occlusion_next_device_ptr, rbs_export_plane / rbs_import_plane, rbs_export_window /
rbs_import_window.  A plane that goes in comes out bit for bit by every route; slabs grow for a plane or a window handed in from
outside without disturbing the other slots; every refusal is a host-side argument check with its own message that leaves the
planes as they were.  Small frames (160 x 120, 16 slots): the long scenarios at 320 x 240 and above are in the layouts' own suites."""
import numpy as np
import pytest

import scenarios as sc
from dbot_ros_amd import RbSensor, RbSensorError, _capi, synth

pytestmark = pytest.mark.gpu

COLS, ROWS, N = 160, 120, 16
BOX = (44, 31, 92, 70)        # x0, y0, x1, y1: off-centre, x0 and x1 multiples of 4 (what a window may be)
ODD_BOX = (13, 7, 51, 40)     # x0, x1 not multiples of 4: whole-plane routes only

# name -> (constructor arguments, shared trail active)
LAYOUTS = {
    "dense": (dict(state_layout="dense"), False),
    "windowed": (dict(), False),
    "slabs": (dict(slab_px=4096), False),
    "reference": (dict(occlusion="reference"), False),
    "reference-slabs": (dict(occlusion="reference", slab_px=4096), False),
    "windowed-shared": (dict(), True),
    "slabs-shared": (dict(slab_px=4096), True),
    "reference-shared": (dict(occlusion="reference"), True),
}
EMPTY = (COLS, ROWS, 0, 0)
WHOLE = (0, 0, COLS, ROWS)


def _scene():
    return sc.make_scene(("m1_l2",), COLS, ROWS, max_particles=N)


def _open(monkeypatch, name, **more):
    """A handle in the named layout; `shared`: driven into the shared trail by a short updating sequence, as
    tests/test_gpu_exact_occlusion.py::test_plane_transport_against_a_shared_plane does."""
    kw, shared = LAYOUTS[name]
    kw = dict(kw, **more)
    monkeypatch.setenv("RBS_SHARED_TRAIL", "1" if shared else "0")
    if shared:
        monkeypatch.setenv("RBS_STP_ENTER", "0.0")
        monkeypatch.setenv("RBS_STP_EVERY", "3")
    om, cam, P = _scene()
    g = RbSensor(om, cam, P, max_particles=N, **kw)
    if shared:
        g.set_timing_every(1)
        g.reset()
        _advance(g, 8, update=True)
        assert g.shared_trail_state()[0]
    return g


def _advance(g, frames, update, seed=31):
    rng = np.random.default_rng(seed)
    idx = np.zeros(N, np.int32)
    for k in range(frames):
        t = synth.truth_pose(1, frame=k)
        t[:, 9] += -0.08 + 0.012 * k
        g.set_observation(synth.make_frame(g.render_depth(t), ROWS, COLS, rng))
        g.loglikes_poses(synth.particle_poses(t, N, rng, scale=1.0), idx, update=update)
        idx = np.sort(rng.choice(N, size=N)).astype(np.int32)


def _planted(g, box, seed=0):
    """The background level everywhere except `box`, which holds values in (0.2, 0.9) that differ from it."""
    bg = np.float32(g.get_background())
    x0, y0, x1, y1 = box
    plane = np.full((ROWS, COLS), bg, np.float32)
    v = np.random.default_rng(seed).uniform(0.2, 0.9, (y1 - y0, x1 - x0)).astype(np.float32)
    v[v == bg] = np.float32(0.5)
    plane[y0:y1, x0:x1] = v
    return plane.ravel()


def _sentinel(buf):
    """-1 everywhere, and there before the library's streams touch the buffer (torch fills on a stream of its own)."""
    import torch
    buf.fill_(-1.0)
    torch.cuda.synchronize()


def _cut(plane, rect):
    return plane.reshape(ROWS, COLS)[rect[1]:rect[3], rect[0]:rect[2]].ravel()


def _contains(rect, box):
    return rect[0] <= box[0] and rect[1] <= box[1] and rect[2] >= box[2] and rect[3] >= box[3]


def _refused(code, fragment, call, *args, **kw):
    with pytest.raises(RbSensorError) as e:
        call(*args, **kw)
    assert e.value.code == code, (e.value.code, str(e.value))
    assert fragment in str(e.value), str(e.value)
    return str(e.value)


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_round_trips(monkeypatch, name):
    import torch
    shared = LAYOUTS[name][1]
    reference = "reference" in name
    travels_whole = shared or name == "dense"      # no window of its own to send: the plane travels whole
    with _open(monkeypatch, name) as g:
        bg_plane = np.full(ROWS * COLS, np.float32(g.get_background()), np.float32)
        buf = torch.empty(COLS * ROWS, dtype=torch.float32, device="cuda:0")
        a, b, c, d, e = 1, 5, 9, 12, 14
        # host routes, both planted planes
        for seed, box in enumerate((BOX, ODD_BOX)):
            plane = _planted(g, box, seed)
            g.set_occlusion(a, plane)
            assert np.array_equal(g.get_occlusion(a), plane), box
            # whole planes, device to device
            _sentinel(buf)
            g.export_plane(a, buf.data_ptr())
            g.synchronize(); torch.cuda.synchronize()
            assert np.array_equal(buf.cpu().numpy(), plane), box
            g.import_plane(b, buf.data_ptr())
            g.synchronize()
            assert np.array_equal(g.get_occlusion(b), plane), box
        # the window-sized routes: the aligned box
        plane = _planted(g, BOX, 7)
        g.set_occlusion(a, plane)
        _sentinel(buf)
        rect = g.export_window(a, buf.data_ptr(), buf.numel())
        g.synchronize(); torch.cuda.synchronize()
        assert _contains(rect, BOX), rect
        if travels_whole:
            assert rect == WHOLE
        if name in ("slabs", "reference", "reference-slabs"):      # the stored window is the box of what differs
            assert rect == BOX
        w = (rect[2] - rect[0]) * (rect[3] - rect[1])
        got = buf.cpu().numpy()
        assert np.array_equal(got[:w], _cut(plane, rect))
        assert (got[w:] == -1.0).all()
        g.import_window(c, rect, buf.data_ptr())
        g.synchronize()
        assert np.array_equal(g.get_occlusion(c), plane)
        assert np.array_equal(g.get_occlusion(a), plane)
        # an empty window with no payload is the background plane; sent on, it is empty again and carries nothing
        g.import_window(d, EMPTY, None)
        g.synchronize()
        _sentinel(buf)
        rect = g.export_window(d, buf.data_ptr(), buf.numel())
        g.synchronize(); torch.cuda.synchronize()
        if travels_whole:
            assert rect == WHOLE and np.array_equal(buf.cpu().numpy(), bg_plane)
        else:
            assert rect == EMPTY and (buf.cpu().numpy() == -1.0).all()
        assert np.array_equal(g.get_occlusion(d), bg_plane)
        if name in ("slabs", "reference", "reference-slabs"):      # ... and so is an all-background plane handed in whole
            g.set_occlusion(e, bg_plane)
            assert g.export_window(e, buf.data_ptr(), buf.numel()) == EMPTY
            g.synchronize(); torch.cuda.synchronize()
            assert (buf.cpu().numpy() == -1.0).all()
            assert np.array_equal(g.get_occlusion(e), bg_plane)
        # float whole planes: the slot itself, read in place
        if name in ("dense", "windowed", "windowed-shared"):
            p = g.occlusion_device_ptr(a)
            assert p
            g.export_plane(a, buf.data_ptr())
            g.synchronize(); torch.cuda.synchronize()
            view = g.get_occlusion(a)
            assert np.array_equal(buf.cpu().numpy(), view) and np.array_equal(view, plane)
            own = torch.as_tensor(_DeviceFloats(p, COLS * ROWS), device="cuda:0")
            assert np.array_equal(own.cpu().numpy(), view)
            assert g.occlusion_device_ptr(a, next_buffer=True) not in (None, 0, p)
        elif reference:
            _refused(_capi.RBS_ERR_UNSUPPORTED, "not a float plane", g.occlusion_device_ptr, a)


class _DeviceFloats:
    """A raw device address as torch takes it in (the slot is the library's memory, not a tensor's)."""

    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<f4", "data": (int(ptr), False), "version": 2}


@pytest.mark.parametrize("name", ["slabs", "reference-slabs"])
def test_slabs_grow_for_a_plane_or_a_window_handed_in(monkeypatch, name):
    """A plane whose box exceeds the slab (rbs_set_occlusion), then a window larger than the grown slab (rbs_import_window): both
    are taken, and the other slots' planes move with the slabs -- values and, on stamped planes, ages."""
    import torch
    with _open(monkeypatch, name, slab_px=1024) as g:
        small = [_planted(g, (8 + 12 * k, 10 + 9 * k, 24 + 12 * k, 18 + 9 * k), 20 + k) for k in range(4)]     # 16 x 8 px each
        for k in range(4):
            g.set_occlusion(k, small[k])
        if "reference" in name:      # a frame passes and is looked at: what is stored is no longer "as of now"
            _advance(g, 1, update=False)
        before = [g.get_occlusion(k) for k in range(4)]
        if "reference" not in name:
            assert all(np.array_equal(x, y) for x, y in zip(before, small))
        big = _planted(g, (20, 20, 84, 60), 30)                 # 64 x 40 = 2 560 px > 1 024
        g.set_occlusion(4, big)
        assert np.array_equal(g.get_occlusion(4), big)
        for k in range(4):
            assert np.array_equal(g.get_occlusion(k), before[k]), k
        rect = (16, 10, 144, 110)                               # 128 x 100 = 12 800 px: beyond any slab the first growth chose
        bigger = _planted(g, rect, 31)
        payload = torch.from_numpy(_cut(bigger, rect).copy()).to("cuda:0")
        torch.cuda.synchronize()
        g.import_window(5, rect, payload.data_ptr())
        g.synchronize()
        assert np.array_equal(g.get_occlusion(5), bigger)
        assert np.array_equal(g.get_occlusion(4), big)
        for k in range(4):
            assert np.array_equal(g.get_occlusion(k), before[k]), k


ENTRY_POINTS = ("get_occlusion", "set_occlusion", "occlusion_device_ptr", "occlusion_next_device_ptr",
                "export_plane", "import_plane", "export_window", "import_window")


def _call(g, entry, slot, buf, plane):
    {"get_occlusion": lambda: g.get_occlusion(slot),
     "set_occlusion": lambda: g.set_occlusion(slot, plane),
     "occlusion_device_ptr": lambda: g.occlusion_device_ptr(slot),
     "occlusion_next_device_ptr": lambda: g.occlusion_device_ptr(slot, next_buffer=True),
     "export_plane": lambda: g.export_plane(slot, buf.data_ptr()),
     "import_plane": lambda: g.import_plane(slot, buf.data_ptr()),
     "export_window": lambda: g.export_window(slot, buf.data_ptr(), buf.numel()),
     "import_window": lambda: g.import_window(slot, BOX, buf.data_ptr())}[entry]()


@pytest.mark.parametrize("name", ["windowed", "slabs", "reference"])
def test_refusals_leave_the_planes_alone(monkeypatch, name):
    """Every refusal here is an argument check on the host that returns before anything is launched."""
    import torch
    with _open(monkeypatch, name) as g:
        plane = _planted(g, BOX, 3)
        g.set_occlusion(2, plane)
        buf = torch.zeros(COLS * ROWS, dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        inv, uns = _capi.RBS_ERR_INVALID_ARGUMENT, _capi.RBS_ERR_UNSUPPORTED
        for entry in ENTRY_POINTS:
            for slot in (-1, N):
                msg = _refused(inv, f"{entry}: bad slot", _call, g, entry, slot, buf, plane)
                assert f"bad slot {slot}" in msg
        _refused(inv, "bad rectangle", g.import_window, 3, (2, 8, 30, 20), buf.data_ptr())           # windows move whole float4s
        _refused(inv, "bad rectangle", g.import_window, 3, (8, 8, COLS + 4, 20), buf.data_ptr())
        rect = g.export_window(2, buf.data_ptr(), buf.numel())
        w = (rect[2] - rect[0]) * (rect[3] - rect[1])
        _refused(inv, "the buffer", g.export_window, 2, buf.data_ptr(), w - 1)
        if name == "reference":
            _refused(uns, "occlusion_device_ptr:", g.occlusion_device_ptr, 2)
            _refused(uns, "occlusion_next_device_ptr:", g.occlusion_device_ptr, 2, next_buffer=True)
        if name == "slabs":
            _refused(uns, "occlusion_next_device_ptr: slots are slabs", g.occlusion_device_ptr, 2, next_buffer=True)
            _refused(uns, "cannot be made dense", g.occlusion_device_ptr, 2)
        assert np.array_equal(g.get_occlusion(2), plane)


def test_a_group_routes_global_slots_to_its_shard(monkeypatch):
    """A one-shard group on one device (RBS_GROUP_SINGLE, as tests/test_gpu_multidevice.py): the same entry points through global
    slots; the group's own range check; a shard's refusal with the device in front."""
    import torch
    monkeypatch.setenv("RBS_GROUP_SINGLE", "1")
    monkeypatch.setenv("RBS_SHARED_TRAIL", "0")
    om, cam, P = _scene()
    with RbSensor(om, cam, P, max_particles=N, device_ids=[0]) as g:
        plane = _planted(g, BOX, 5)
        buf = torch.empty(COLS * ROWS, dtype=torch.float32, device="cuda:0")
        g.set_occlusion(3, plane)
        assert np.array_equal(g.get_occlusion(3), plane)
        g.export_plane(3, buf.data_ptr())
        g.import_plane(N - 1, buf.data_ptr())
        g.synchronize()
        assert np.array_equal(g.get_occlusion(N - 1), plane)
        rect = g.export_window(3, buf.data_ptr(), buf.numel())
        assert _contains(rect, BOX)
        g.import_window(7, rect, buf.data_ptr())
        g.synchronize()
        assert np.array_equal(g.get_occlusion(7), plane)
        inv = _capi.RBS_ERR_INVALID_ARGUMENT
        for entry in ENTRY_POINTS:
            for slot in (-1, N):
                msg = _refused(inv, f"bad slot {slot}", _call, g, entry, slot, buf, plane)
                assert entry not in msg and "device 0" not in msg
        msg = _refused(inv, "device 0: import_window: bad rectangle", g.import_window, 7, (8, 8, COLS + 4, 20), buf.data_ptr())
        w = (rect[2] - rect[0]) * (rect[3] - rect[1])
        _refused(inv, "device 0: export_window: the window of slot 3", g.export_window, 3, buf.data_ptr(), w - 1)
        assert np.array_equal(g.get_occlusion(3), plane) and np.array_equal(g.get_occlusion(7), plane)
