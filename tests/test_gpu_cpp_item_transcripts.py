"""GPU test: the per-item transcript calls of include/bpp.h from compiled code with arrays the program hipMalloc'ed itself, on a context
made with bpp_ctx_create_on_stream, tests/cpp/item_transcripts.cpp: six m = 1 items per set, each proved under a transcript of its own
(bpp_transcript_new + bpp_transcript_append_message); bpp_batch_upload_packed_device_transcripts, a refill under a mask with new
proofs and new transcripts, and bpp_verify_enqueue_states behind each, with one wait at the end.  The program holds every (step, group)
to a blocking bpp_verify_batch_states over the group's live items -- the code, and the 203-byte rows of the live slots; zero rows for
dead slots and for the rejected group -- and this test reads what it printed."""
import importlib
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_item_transcripts_in_and_out(tmp_path):
    pkg = importlib.import_module("bulletproofs-plus_amd")
    lib = pkg._build.build()
    exe = str(tmp_path / "item_transcripts")
    libdir = os.path.dirname(lib)
    subprocess.run(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                    os.path.join(ROOT, "tests", "cpp", "item_transcripts.cpp"), "-o", exe, "-L", libdir, "-lbpp_hip", "-L/opt/rocm/lib",
                    "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "item transcripts ok" in out.stdout, (out.stdout[-500:], out.stderr[-2000:])
    got = dict(line.split(" ", 1) for line in out.stdout.splitlines() if " " in line)
    # one refill, two enqueues, no wait on the host in either
    assert got["stats"] == "1 0 2 0"
    # the refill took: the bad state and the invalid proof at the dead slot are nothing
    assert got["record"].split() == ["0", "0", "0", "1"]
    # code, tier, flags of the enqueued call, and the blocking call's code
    assert got["group_0_0"].split() == ["0", "0", "1", "reference", "0"] and got["group_0_1"].split() == ["0", "0", "1", "reference", "0"]
    assert got["group_1_0"].split() == ["1", "7", "1", "reference", "1"]  # VerificationFailed from the final check
    assert got["group_1_1"].split() == ["0", "0", "1", "reference", "0"]
    assert "unknown batch handle" in got["refused"] and "unknown batch handle" in got["refused_states"]
