"""The raster kernels that do the windowed copy themselves (rbs_raster_kernel_wcopy_*) keep the budget of the kernels they
stand in for: three waves per SIMD in 160 VGPRs, and the binary64 one (the headline's) with nothing in scratch.  Read from
the compiler's report the Makefile writes next to the library."""
import os
import re

from dbot_ros_amd import _capi


def _usage(txt, mangled_part):
    m = re.search(r"Function Name: (\S*" + re.escape(mangled_part) + r"\S*).*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+)"
                  r".*?Occupancy \[waves/SIMD\]: (\d+).*?VGPRs Spill: (\d+)", txt, re.S)
    assert m, mangled_part
    return {"vgprs": int(m.group(2)), "scratch": int(m.group(3)), "occupancy": int(m.group(4)), "spills": int(m.group(5))}


def test_fused_copy_kernels_keep_the_register_budget():
    path = os.path.join(os.path.dirname(_capi.LIB_PATH), "resource_usage.txt")
    assert os.path.exists(path), "make -C dbot_ros_amd/csrc writes lib/resource_usage.txt"
    txt = open(path).read()
    f64 = _usage(txt, "rbs_raster_kernel_wcopy_one_f64")
    assert f64 == {"vgprs": 160, "scratch": 0, "occupancy": 3, "spills": 0}, f64
    # precision F32: the bound tests/test_capi_cpu.py holds the float32 raster kernels to (a few kernel-lifetime dwords in scratch)
    f32 = _usage(txt, "rbs_raster_kernel_wcopy_f32")
    assert f32["vgprs"] <= 160 and f32["occupancy"] == 3 and f32["spills"] <= 4, f32
