"""GPU test: the device-memory entry points of include/bpp.h and the overload pair of include/bpp.hpp from compiled code with arrays
the program hipMalloc'ed itself, tests/cpp/device_inputs.cpp.  What it prints for the device form -- return code, recovered masks,
presence, the point of the final check (BPP_TRACE_MSM_RESULT), the exception of a finding -- must equal what it prints for the host
form on the same bytes, and the point must be the identity."""
import importlib
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_device_inputs_equal_host_inputs(tmp_path):
    pkg = importlib.import_module("bulletproofs-plus_amd")
    lib = pkg._build.build()
    exe = str(tmp_path / "device_inputs")
    libdir = os.path.dirname(lib)
    subprocess.run(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                    os.path.join(ROOT, "tests", "cpp", "device_inputs.cpp"), "-o", exe, "-L", libdir, "-lbpp_hip", "-L/opt/rocm/lib",
                    "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "device_inputs ok" in out.stdout, (out.stdout[-500:], out.stderr[-2000:])
    got = dict(line.split(" ", 1) for line in out.stdout.splitlines() if " " in line)
    assert got["host_code"] == got["device_code"] == "0"
    for what in ("masks", "present", "msm", "error"):
        pairs = [(k, k.replace("host_", "device_", 1)) for k in got if k.startswith(("host_" + what, "hpp_host_" + what))]
        assert pairs, what
        for h, d in pairs:
            assert got[d] == got[h], (h, got[h], got[d])
    assert got["host_present"] == "01" * 5 and len(got["host_masks"]) == 2 * 32 * 5
    assert got["device_msm"] == "00" * 32  # the identity
    assert sum(1 for k in got if k.startswith("hpp_device_mask_")) == 5
    assert got["hpp_device_error"].startswith("2 ") and "Invalid parsing" in got["hpp_device_error"]
