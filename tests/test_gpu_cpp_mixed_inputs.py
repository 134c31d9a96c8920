"""GPU test: the mixed-aggregation array form of include/bpp.h and the overload pair of include/bpp.hpp from compiled code with
arrays the program hipMalloc'ed itself, tests/cpp/mixed_inputs.cpp.  What bpp_prove_openings wrote goes into a bpp_mixed_batch as it
is.  What the program prints for the host form and for the device form -- return code, recovered masks, presence, the point of the
final check (BPP_TRACE_MSM_RESULT), the exception of a finding -- must equal what it prints for the bpp_verify_item array over the
same rows, and the point must be the identity."""
import importlib
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_mixed_inputs_equal_the_item_form(tmp_path):
    pkg = importlib.import_module("bulletproofs-plus_amd")
    lib = pkg._build.build()
    exe = str(tmp_path / "mixed_inputs")
    libdir = os.path.dirname(lib)
    subprocess.run(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                    os.path.join(ROOT, "tests", "cpp", "mixed_inputs.cpp"), "-o", exe, "-L", libdir, "-lbpp_hip", "-L/opt/rocm/lib",
                    "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "mixed_inputs ok" in out.stdout, (out.stdout[-500:], out.stderr[-2000:])
    got = dict(line.split(" ", 1) for line in out.stdout.splitlines() if " " in line)
    assert got["items_code"] == got["host_code"] == got["device_code"] == "0"
    for what in ("masks", "present", "msm"):
        assert got["host_" + what] == got["items_" + what] and got["device_" + what] == got["items_" + what], what
    assert got["items_present"] == "0001000101" and len(got["items_masks"]) == 2 * 32 * 5
    assert got["device_msm"] == "00" * 32  # the identity
    masks = [k for k in got if k.startswith("hpp_host_mask_")]
    assert len(masks) == 3
    for k in masks:
        assert got[k.replace("host", "device", 1)] == got[k]
    assert got["hpp_device_error_0"] == got["hpp_host_error_0"] and "Invalid parsing" in got["hpp_device_error_0"]
    assert got["hpp_device_error_1"] == got["hpp_host_error_1"] and "Number of commitments must be a power of two" in got["hpp_device_error_1"]
