"""GPU test: bpp_batch_refill_enqueue_mixed of include/bpp.h from compiled code with arrays the program hipMalloc'ed itself, on a context
made with bpp_ctx_create_on_stream, tests/cpp/refill_mixed.cpp: the buffers bpp_prove_batch_mixed wrote go into a ring of three device
input sets as they are; three steps of refill under a mask + bpp_verify_enqueue run with one wait at the end; every (step, group) is
held to a blocking bpp_verify_batch_mixed over the group's live rows.  Findings at dead slots change nothing, an invalid proof at a
live slot is the blocking call's rejection, a group without a live row gets the EMPTY record."""
import importlib
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_mixed_refill_under_masks(tmp_path):
    pkg = importlib.import_module("bulletproofs-plus_amd")
    lib = pkg._build.build()
    exe = str(tmp_path / "refill_mixed")
    libdir = os.path.dirname(lib)
    subprocess.run(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                    os.path.join(ROOT, "tests", "cpp", "refill_mixed.cpp"), "-o", exe, "-L", libdir, "-lbpp_hip", "-L/opt/rocm/lib",
                    "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "refill mixed ok" in out.stdout, (out.stdout[-500:], out.stderr[-2000:])
    got = dict(line.split(" ", 1) for line in out.stdout.splitlines() if " " in line)
    # three refills, the first one made the batch's words and its mask; no refill waited on the host
    assert got["stats"] == "3 1 0"
    rejected = []
    for k in range(3):
        # the refill record: code, tier, index, flags (1 written): every refill took, whatever lay at dead slots
        assert got["record_%d" % k].split() == ["0", "0", "0", "1"], (k, got["record_%d" % k])
        for g in range(2):
            verdict, ref = got["verdict_%d_%d" % (k, g)].split(), got["reference_%d_%d" % (k, g)].split()
            if ref == ["empty"]:
                assert verdict[:3] == ["0", "0", "9"], (k, g, verdict)  # written | no live item
                continue
            code, tier, flags = verdict[:3]
            assert code == ref[0] and flags == "1", (k, g, verdict, ref)
            if ref[0] == "0":  # accepted: the masks and the presence of the live slots are the blocking call's
                assert tier == "0" and verdict[3:] == ref[1:], (k, g)
                assert any(item.startswith("1:") and item.strip("1:0,") for item in ref[1].split(",") if item), (k, g, ref)
            else:
                assert (code, tier) == ("1", "7"), (k, g, verdict)  # VerificationFailed from the final check
                rejected.append((k, g))
    assert rejected == [(2, 1)] and got["reference_2_0"] == "empty"
    assert "unknown batch handle" in got["refused"]
    assert "count_dev and live_dev" in got["both"]
