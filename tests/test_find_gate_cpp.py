"""The C++ mirror of the finder's silhouette gate (include/dbot_amd/object_finder.hpp: ObjectFinder::Gate, ::set_gate,
::evidence, SceneFinder::set_gate): the header compiles cleanly on its own, and a small program over it
(tests/cpp/find_gate_check.cpp) linked against the library gives Python's find bit for bit, or fails loudly where there is
no GPU."""
import os
import subprocess

import numpy as np

import test_find_object_cpu as drv
from dbot_ros_amd import _capi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
INC = os.path.join(ROOT, "include")
SMALL = dict(max_seeds=48, n_rotations=128, n_candidates=256, n_survivors=8, rounds=3, children=16, batch=4096)


def test_object_finder_header_compiles_on_its_own(tmp_path):
    tu = tmp_path / "only_the_header.cpp"
    tu.write_text("#include <dbot_amd/object_finder.hpp>\nstatic_assert(sizeof(dbot_amd::ObjectFinder::Gate) == sizeof(rbs_find_gate), \"\");\n")
    r = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I" + INC, str(tu)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr[-3000:]


def test_program_over_the_mirror_gives_pythons_find_or_fails_loudly(tmp_path):
    import scenarios as sc
    from dbot_ros_amd.finder import ObjectFinder
    exe = str(tmp_path / "find_gate_check")
    lib_dir = os.path.dirname(_capi.LIB_PATH)
    r = subprocess.run(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + INC, "-o", exe, os.path.join(HERE, "cpp", "find_gate_check.cpp"),
                        "-L" + lib_dir, "-lrbsensor_mi355x", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    p = ObjectFinder.Parameters()
    for k, v in SMALL.items():
        setattr(p, k, v)
    have_gpu = _capi.load().rbs_device_count() > 0
    om, cam, P = sc.make_scene(("m1",), 160, 120, max_particles=1)
    if have_gpu:
        from test_gpu_finder import _scene
        om, cam, P, sensor, truth, frame = _scene("m1", 160, 120, seed=3)
        with sensor, ObjectFinder(sensor, om, p, gate=ObjectFinder.Gate(require_confirmed=True)) as fnd:
            want = fnd.find(frame)
            want_rec, want_cls = fnd.evidence("result")
    else:
        frame = np.full(cam.rows * cam.cols, 1.0, dtype=np.float32)
    inp, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    drv.write_driver_input(inp, om.vertices[0], om.triangles[0], cam.camera_matrix, cam.cols, cam.rows, p, frame)
    run = subprocess.run([exe, inp, out], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout, run.stderr[-2000:])
    if not have_gpu:
        assert run.stdout.startswith("NO_DEVICE")
        return
    assert run.stdout.startswith("OK"), (run.stdout, run.stderr)
    raw = open(out, "rb").read()
    found, n = np.frombuffer(raw[:8], dtype=np.int32)
    assert bool(found) == want.found and n == len(want.poses)
    d = np.frombuffer(raw[8: 8 + 8 * 25 * n], dtype=np.float64)
    i = np.frombuffer(raw[8 + 8 * 25 * n:], dtype=np.int32)
    assert len(i) == 11 * n
    assert np.array_equal(d[: 12 * n].reshape(n, 12).view(np.uint64), want.poses.view(np.uint64))
    assert np.array_equal(d[12 * n: 13 * n].view(np.uint64), want.scores.view(np.uint64))
    assert np.array_equal(i[: 10 * n].reshape(n, 10), want_rec) and np.array_equal(i[10 * n:], want_cls) and np.array_equal(want_cls, want.classes)
