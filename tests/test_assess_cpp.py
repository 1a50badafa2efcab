"""The C++ mirror of the pose assessor (include/dbot_amd/pose_assessor.hpp): it compiles cleanly on its own, and a
small program over it (tests/cpp/assess_check.cpp) linked against the library fails loudly where there is no GPU."""
import os
import subprocess

from dbot_ros_amd import _capi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
INC = os.path.join(ROOT, "include")
LIB = os.path.join(ROOT, "dbot_ros_amd", "lib")


def test_pose_assessor_header_compiles_on_its_own(tmp_path):
    tu = tmp_path / "only_the_header.cpp"
    tu.write_text("#include <dbot_amd/pose_assessor.hpp>\n")
    r = subprocess.run(["g++", "-std=c++14", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I" + INC, str(tu)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr[-3000:]


def test_program_over_the_mirror_runs_or_fails_loudly(tmp_path):
    exe = str(tmp_path / "assess_check")
    r = subprocess.run(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-I" + INC, "-o", exe, os.path.join(HERE, "cpp", "assess_check.cpp"),
                        "-L" + LIB, "-lrbsensor_mi355x", "-Wl,-rpath," + LIB, "-Wl,-rpath,/opt/rocm/lib"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout, run.stderr[-2000:])
    if _capi.load().rbs_device_count() > 0:
        tag, *nums = run.stdout.split()
        rendered, valid, support, in_front, behind, verdict, first = (int(v) for v in nums)
        # the frame is the pose's own depth image: every owned pixel agrees
        assert tag == "OK" and rendered >= 16 and valid == rendered and support == rendered and in_front == 0 and behind == 0
        assert verdict == _capi.RBS_ASSESS_SUPPORTED and first == 0
    else:
        assert run.stdout.startswith("NO_DEVICE") and "no CPU path" in run.stdout
