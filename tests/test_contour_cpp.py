"""The contour rule through the C++ mirror of the pose assessor (include/dbot_amd/pose_assessor.hpp): a small program
over it (tests/cpp/contour_check.cpp) linked against the library runs, or fails loudly where there is no GPU."""
import os
import subprocess

from dbot_ros_amd import _capi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
INC = os.path.join(ROOT, "include")
LIB = os.path.join(ROOT, "dbot_ros_amd", "lib")


def test_program_over_the_mirror_runs_or_fails_loudly(tmp_path):
    exe = str(tmp_path / "contour_check")
    r = subprocess.run(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + INC, "-o", exe,
                        os.path.join(HERE, "cpp", "contour_check.cpp"),
                        "-L" + LIB, "-lrbsensor_mi355x", "-Wl,-rpath," + LIB, "-Wl,-rpath,/opt/rocm/lib"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout, run.stderr[-2000:])
    if _capi.load().rbs_device_count() > 0:
        tag, *nums = run.stdout.split()
        assert tag == "OK" and len(nums) == 15, run.stdout
        rim, valid, flush, in_front, beyond, verdict, confirmed = (int(v) for v in nums[:7])
        # the body's own depth image in front of a wall at 1.5 m: every rim pixel lies beyond its anchor
        assert rim >= 16 and valid == rim and beyond == rim and flush == 0 and in_front == 0
        assert verdict == _capi.RBS_CONTOUR_PRESENT and confirmed == 0
        rim2, valid2, flush2, in_front2, beyond2, verdict2, supported2, confirmed2 = (int(v) for v in nums[7:])
        # the same image with the rim at its anchors' depth: SUPPORTED as before, every rim pixel flush, not confirmed
        assert rim2 == rim and valid2 == rim and flush2 == rim and in_front2 == 0 and beyond2 == 0
        assert verdict2 == _capi.RBS_CONTOUR_ABSENT and supported2 == 0 and confirmed2 == -1
    else:
        assert run.stdout.startswith("NO_DEVICE") and "no CPU path" in run.stdout
