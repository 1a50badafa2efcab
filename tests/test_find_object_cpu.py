"""The object finder's C++ mirror (include/dbot_amd/object_finder.hpp) without a device: its driver
(tests/cpp/find_object_check.cpp) compiles against include/ with every warning an error and answers NO_DEVICE where
no device can be opened.  tests/test_gpu_finder_layers.py runs it against the Python finder."""
import os
import subprocess

import numpy as np

from dbot_ros_amd import _capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER_SRC = os.path.join(ROOT, "tests", "cpp", "find_object_check.cpp")


def build_driver(out_dir):
    """g++ the C++ mirror's driver into out_dir; returns the executable's path."""
    exe = os.path.join(str(out_dir), "find_object_check")
    lib_dir = os.path.dirname(_capi.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           DRIVER_SRC, "-L" + lib_dir, "-lrbsensor_mi355x", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def write_driver_input(path, vertices, triangles, K, cols, rows, params, frame):
    """The driver's input file (its header comment); vertices are used as they are (centre them first)."""
    p = params
    with open(path, "wb") as f:
        f.write(np.array([cols, rows, len(vertices), len(triangles), p.max_seeds, p.n_rotations, p.n_candidates,
                          p.n_survivors, p.rounds, p.children, p.batch], dtype=np.int32).tobytes())
        f.write(np.ascontiguousarray(K, dtype=np.float64).ravel().tobytes())
        f.write(np.ascontiguousarray(vertices, dtype=np.float64).ravel().tobytes())
        f.write(np.ascontiguousarray(triangles, dtype=np.int32).ravel().tobytes())
        f.write(np.ascontiguousarray(frame, dtype=np.float32).ravel().tobytes())


def read_driver_output(path):
    raw = open(path, "rb").read()
    found, n = np.frombuffer(raw[:8], dtype=np.int32)
    d = np.frombuffer(raw[8:], dtype=np.float64)
    return bool(found), d[: 12 * n].reshape(n, 12), d[12 * n: 13 * n], d[13 * n:].reshape(n, 12)


def test_driver_compiles_and_needs_a_device(tmp_path):
    from dbot_ros_amd.finder import ObjectFinder
    exe = build_driver(tmp_path)
    lib = _capi.load()
    if lib.rbs_device_count() > 0:
        return   # (a device is visible: tests/test_gpu_finder_layers.py runs the driver)
    v, t = synth.mesh_m1()
    inp = os.path.join(str(tmp_path), "in.bin")
    write_driver_input(inp, v - v.mean(0), t, synth.camera_matrix(80, 60), 80, 60, ObjectFinder.Parameters(),
                       np.full(80 * 60, np.nan, dtype=np.float32))
    r = subprocess.run([exe, inp, os.path.join(str(tmp_path), "out.bin")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.startswith("NO_DEVICE"), (r.returncode, r.stdout, r.stderr)
