"""The C++ mirror of the pose refiner (include/dbot_amd/pose_refiner.hpp): it compiles cleanly on its own, and a small
program over it (tests/cpp/refine_check.cpp) linked against the library fails loudly where there is no GPU."""
import os
import subprocess

from dbot_ros_amd import _capi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
INC = os.path.join(ROOT, "include")
LIB = os.path.join(ROOT, "dbot_ros_amd", "lib")


def test_pose_refiner_header_compiles_on_its_own(tmp_path):
    tu = tmp_path / "only_the_header.cpp"
    tu.write_text("#include <dbot_amd/pose_refiner.hpp>\n")
    r = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I" + INC, str(tu)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr[-3000:]


def test_program_over_the_mirror_runs_or_fails_loudly(tmp_path):
    exe = str(tmp_path / "refine_check")
    r = subprocess.run(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-I" + INC, "-o", exe, os.path.join(HERE, "cpp", "refine_check.cpp"),
                        "-L" + LIB, "-lrbsensor_mi355x", "-Wl,-rpath," + LIB, "-Wl,-rpath,/opt/rocm/lib"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout, run.stderr[-2000:])
    if _capi.load().rbs_device_count() > 0:
        tag, status, iterations, first, last, before, after, h0 = run.stdout.split()
        # a noise-free frame of the truth: the 3 mm come back (three faces show, so nothing is left free to slide)
        assert tag == "OK" and int(status) == _capi.RBS_REFINE_CONVERGED and 1 <= int(iterations) <= 10, run.stdout
        assert int(first) >= 16 and int(last) >= int(first) and float(after) < 0.1 * float(before), run.stdout
        assert int(h0) == _capi.RBS_REFINE_MAX_ITERATIONS
    else:
        assert run.stdout.startswith("NO_DEVICE") and "no CPU path" in run.stdout
