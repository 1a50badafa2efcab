"""The Gaussian tracker's device pipeline (rbs_gauss_submit / rbs_gauss_result) without a device: the exported C-ABI,
the new kernels' register budget in the compiler's report, and the C++ mirror's submit / result compiling against
include/.  tests/test_gpu_gaussian_pipeline.py runs it all."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from dbot_ros_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIPELINE_SYMBOLS = ("rbs_gauss_submit", "rbs_gauss_submit_f64", "rbs_gauss_result")
NEW_KERNELS = ("rbs_gauss_predict_kernel", "rbs_gauss_reduce_update_kernel")
DRIVER_SRC = os.path.join(ROOT, "tests", "cpp", "gauss_pipeline_check.cpp")


def build_driver(out_dir):
    """g++ the C++ mirror's driver (tests/cpp/gauss_pipeline_check.cpp) into out_dir; returns the executable's path."""
    exe = os.path.join(str(out_dir), "gauss_pipeline_check")
    lib_dir = os.path.dirname(_capi.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           DRIVER_SRC, "-L" + lib_dir, "-lrbsensor_mi355x", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def write_driver_input(path, meshes, K, cols, rows, init_state, frames):
    """The driver's input file (its header comment): raw meshes (centred by the driver, as ObjectModel(center=True)),
    the camera, the initial state in the original mesh frame, float64 frames."""
    with open(path, "wb") as f:
        f.write(np.array([len(meshes), cols, rows, len(frames)], dtype=np.int32).tobytes())
        f.write(np.ascontiguousarray(K, dtype=np.float64).ravel().tobytes())
        f.write(np.array([[len(v), len(t)] for v, t in meshes], dtype=np.int32).ravel().tobytes())
        for v, t in meshes:
            f.write(np.ascontiguousarray(v, dtype=np.float64).ravel().tobytes())
            f.write(np.ascontiguousarray(t, dtype=np.int32).ravel().tobytes())
        f.write(np.ascontiguousarray(init_state, dtype=np.float64).ravel().tobytes())
        for y in frames:
            f.write(np.ascontiguousarray(y, dtype=np.float64).ravel().tobytes())


def _usage(txt, mangled_part):
    m = re.search(r"Function Name: (\S*" + re.escape(mangled_part) + r"\S*).*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+)"
                  r".*?Occupancy \[waves/SIMD\]: (\d+).*?VGPRs Spill: (\d+)", txt, re.S)
    assert m, mangled_part
    return {"vgprs": int(m.group(2)), "scratch": int(m.group(3)), "occupancy": int(m.group(4)), "spills": int(m.group(5))}


def test_pipeline_symbols_are_declared_and_exported():
    lib = C.CDLL(_capi.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "rbsensor_mi355x.h")).read()
    for s in PIPELINE_SYMBOLS:
        assert s in _capi.EXPORTS and hasattr(lib, s) and (s + "(") in header, s


def test_pipeline_calls_fail_loudly_without_a_tracker():
    lib = _capi.load()
    assert lib.rbs_gauss_submit(None, None) == _capi.RBS_ERR_INVALID_ARGUMENT
    assert lib.rbs_gauss_submit_f64(None, None) == _capi.RBS_ERR_INVALID_ARGUMENT
    assert lib.rbs_gauss_result(None, None, None) == _capi.RBS_ERR_INVALID_ARGUMENT


def test_new_kernels_neither_spill_nor_use_scratch():
    path = os.path.join(os.path.dirname(_capi.LIB_PATH), "resource_usage.txt")
    assert os.path.exists(path), "make -C dbot_ros_amd/csrc writes lib/resource_usage.txt"
    txt = open(path).read()
    for k in NEW_KERNELS:
        u = _usage(txt, k)
        assert u["spills"] == 0 and u["scratch"] == 0, (k, u)


def test_cpp_mirror_submit_result_compiles(tmp_path):
    exe = build_driver(tmp_path)
    assert os.access(exe, os.X_OK)
    # usage errors are the driver's own, before any device is touched
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stderr
