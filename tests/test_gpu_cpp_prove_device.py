"""GPU test: bpp_prove_openings_device, bpp_prove_status_result and bpp_prove_device_stats of include/bpp.h and the overload of
RangeProof::prove_openings of include/bpp.hpp from compiled code with arrays the program hipMalloc'ed itself (one input array at an
odd byte address), tests/cpp/prove_device_inputs.cpp.  What the device form leaves in device memory must equal, slack included, what
bpp_prove_openings wrote for the same arrays in host memory, and the verifier must accept it where it lies."""
import importlib
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_prove_device_inputs_equal_the_host_form(tmp_path):
    pkg = importlib.import_module("bulletproofs-plus_amd")
    lib = pkg._build.build()
    exe = str(tmp_path / "prove_device_inputs")
    libdir = os.path.dirname(lib)
    subprocess.run(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                    os.path.join(ROOT, "tests", "cpp", "prove_device_inputs.cpp"), "-o", exe, "-L", libdir, "-lbpp_hip", "-L/opt/rocm/lib",
                    "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "prove_device_inputs ok" in out.stdout, (out.stdout[-500:], out.stderr[-2000:])
    got = dict(line.split(" ", 1) for line in out.stdout.splitlines() if " " in line)
    assert got["device_code"].split()[0] == "0" and got["verify_code"].split()[0] == "0"
    for what in ("proofs_equal", "commitments_equal", "lens_equal", "status_equal", "hpp_proofs_equal"):
        assert got[what] == "1", what
    for i in range(5):
        assert got["record_%d" % i] == "0 0 ''"
    assert got["present"] == "0001000101" and got["hpp_code"] == "0"
    assert got["hpp_finding"] == "3 00300 'Value exceeds bit vector capacity!'"
    assert got["hpp_refusal"].startswith("2 ") and "values is not device memory" in got["hpp_refusal"]
    assert got["stats"] == "3 15 1 0"
