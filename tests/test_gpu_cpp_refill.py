"""GPU test: bpp_batch_refill_enqueue, bpp_refill_result and bpp_refill_stats of include/bpp.h through the mirror of include/bpp.hpp
from compiled code with arrays the program hipMalloc'ed itself, tests/cpp/refill.cpp: three refills of one batch (clean, l in r1 of
proof 3, clean again), each followed by an enqueued verification, one wait at the end."""
import importlib
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_refill_records(tmp_path):
    pkg = importlib.import_module("bulletproofs-plus_amd")
    lib = pkg._build.build()
    exe = str(tmp_path / "refill")
    libdir = os.path.dirname(lib)
    subprocess.run(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                    os.path.join(ROOT, "tests", "cpp", "refill.cpp"), "-o", exe, "-L", libdir, "-lbpp_hip", "-L/opt/rocm/lib",
                    "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "refill ok" in out.stdout, (out.stdout[-500:], out.stderr[-2000:])
    got = dict(line.split(" ", 1) for line in out.stdout.splitlines() if " " in line)
    # code, tier, index, flags (1 written, 2 finding), text: the blocking upload's finding for the second contents
    assert got["refill_0"].split()[:4] == ["0", "0", "0", "1"] == got["refill_2"].split()[:4]
    assert got["refill_1"] == "2 1 3 3 Invalid parsing"
    # code, tier, index, flags (1 written, 4 the last refill did not take)
    assert got["verdict_0"] == "0 0 0 1" == got["verdict_2"]
    assert got["verdict_1"] == "2 1 3 5"
    assert got["stats"] == "3 1 0"
    assert "transcript" in got["refused"] and "upload the arrays for a blocking call" in got["blocking"]
