"""GPU test: the transcript-protocol and transcript-RNG kinds of bpp_transcripts_enqueue from compiled code through
Engine::transcripts_enqueue and the op builders of include/bpp.hpp, with arrays the program hipMalloc'ed itself,
tests/cpp/transcript_rng.cpp: eight rows under a live mask, NEW + APPEND_POINT (one identity), then RNG_BEGIN / RNG_REKEY /
RNG_FINALIZE / RNG_FILL32 / RNG_SCALARS / CHALLENGE_SCALAR, with one wait at the end.  The program holds every row and every output to
the host helpers of include/bpp.h and to their wrappers on bpp_host::Transcript, and this test reads what it printed."""
import importlib
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_transcript_rng_against_the_host_helpers(tmp_path):
    pkg = importlib.import_module("bulletproofs-plus_amd")
    lib = pkg._build.build()
    exe = str(tmp_path / "transcript_rng")
    libdir = os.path.dirname(lib)
    subprocess.run(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                    os.path.join(ROOT, "tests", "cpp", "transcript_rng.cpp"), "-o", exe, "-L", libdir, "-lbpp_hip", "-L/opt/rocm/lib",
                    "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "transcript_rng ok" in out.stdout, (out.stdout[-500:], out.stderr[-2000:])
    got = dict(line.split(" ", 1) for line in out.stdout.splitlines() if " " in line)
    # six live rows; row 6 appends the identity and is void in both calls: flags WRITTEN | IDENTITY, then WRITTEN alone
    assert got["rows_equal_to_the_host_helpers"] == "5" and got["void_rows_all_zero"] == "1"
    assert got["record_1"].split() == ["5", "1", "6", "3"]
    assert got["record_2"].split() == ["5", "1", "6", "1"]
    # a draw without a finalised RNG is refused with the field named
    assert got["refusal"].startswith("2 ") and "ops[1].kind" in got["refusal"] and "finalised RNG" in got["refusal"]
    assert got["stats"] == "2 1 0"
