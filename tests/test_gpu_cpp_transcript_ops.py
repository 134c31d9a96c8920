"""GPU test: bpp_transcripts_enqueue from compiled code through Engine::transcripts_enqueue and the op builders of include/bpp.hpp, with
arrays the program hipMalloc'ed itself, tests/cpp/transcript_ops.cpp: eight rows under a live mask, NEW + APPEND + CHALLENGE and a second
call that appends per-row lengths and draws again, with one wait at the end.  The program holds every row and every challenge to the
host helpers of include/bpp.h (bpp_transcript_new, bpp_transcript_append_message, bpp_transcript_challenge_bytes) and this test reads
what it printed."""
import importlib
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_transcript_ops_against_the_host_helpers(tmp_path):
    pkg = importlib.import_module("bulletproofs-plus_amd")
    lib = pkg._build.build()
    exe = str(tmp_path / "transcript_ops")
    libdir = os.path.dirname(lib)
    subprocess.run(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                    os.path.join(ROOT, "tests", "cpp", "transcript_ops.cpp"), "-o", exe, "-L", libdir, "-lbpp_hip", "-L/opt/rocm/lib",
                    "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "transcript_ops ok" in out.stdout, (out.stdout[-500:], out.stderr[-2000:])
    got = dict(line.split(" ", 1) for line in out.stdout.splitlines() if " " in line)
    # six live rows; five of them come through both calls, row 6 is void in the second
    assert got["rows_equal_to_the_host_helpers"] == "5"
    assert got["record_1"].split() == ["6", "0", str(0xFFFFFFFF), "1"]
    assert got["record_2"].split() == ["5", "1", "6", "1"]
    # a challenge written into the rows themselves is refused with the ranges named
    assert got["refusal"].startswith("2 ") and "overlap" in got["refusal"] and "states203_dev" in got["refusal"]
    # two calls, the context's first among them, no wait on the host
    assert got["stats"] == "2 1 0"
