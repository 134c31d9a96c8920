"""GPU test: bpp_rows_msm_enqueue and bpp_rows_scalar_enqueue from compiled code through Engine::rows_msm_enqueue and
Engine::rows_scalar_enqueue of include/bpp.hpp, with arrays the program hipMalloc'ed itself, tests/cpp/rows_msm.cpp: the commit /
challenge / response step around a transcript on nine rows (one dead, one with the identity as its public key), four enqueues and one
wait.  The program holds every row and every output to the host helpers of include/bpp.h and to bpp_msm_ct, checks s G == R + c X per
row, and this test reads what it printed."""
import importlib
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_commit_challenge_response_on_the_stream(tmp_path):
    pkg = importlib.import_module("bulletproofs-plus_amd")
    lib = pkg._build.build()
    exe = str(tmp_path / "rows_msm")
    libdir = os.path.dirname(lib)
    subprocess.run(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                    os.path.join(ROOT, "tests", "cpp", "rows_msm.cpp"), "-o", exe, "-L", libdir, "-lbpp_hip", "-L/opt/rocm/lib",
                    "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "rows_msm ok" in out.stdout, (out.stdout[-500:], out.stderr[-2000:])
    got = dict(line.split(" ", 1) for line in out.stdout.splitlines() if " " in line)
    # nine rows, row 4 dead, row 6 void from the APPEND_POINT of the identity on
    assert got["responses_verified"] == "7" and got["void_rows_all_zero"] == "1"
    assert got["record_msm"].split() == ["8", "0", "4294967295", "1"]
    assert got["record_transcripts"].split() == ["7", "1", "6", "3"]
    assert got["record_scalar"].split() == ["7", "0", "4294967295", "1"]
    # out may alias none of the inputs
    assert got["refusal"].startswith("2 ") and "c.dev and out_dev overlap" in got["refusal"]
    assert got["stats"] == "2 1 0"
