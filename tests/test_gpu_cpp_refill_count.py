"""GPU test: bpp_batch_refill_enqueue_count and bpp_enqueue_weights of include/bpp.h through the mirror of include/bpp.hpp from
compiled code with arrays the program hipMalloc'ed itself, tests/cpp/refill_count.cpp: a batch of six proofs verified in chunks of
two after refills with count 4 (a proof that does not verify and a non-canonical scalar lie beyond it), count 7, count 6 and no
count, the weights copied out behind every enqueue, one wait at the end."""
import importlib
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_refill_with_a_count(tmp_path):
    pkg = importlib.import_module("bulletproofs-plus_amd")
    lib = pkg._build.build()
    exe = str(tmp_path / "refill_count")
    libdir = os.path.dirname(lib)
    subprocess.run(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                    os.path.join(ROOT, "tests", "cpp", "refill_count.cpp"), "-o", exe, "-L", libdir, "-lbpp_hip", "-L/opt/rocm/lib",
                    "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "refill count ok" in out.stdout, (out.stdout[-500:], out.stderr[-2000:])
    got = dict(line.split(" ", 1) for line in out.stdout.splitlines() if " " in line)
    # refill records: code, tier, index, flags (1 written, 8 the count exceeds the batch), text
    assert got["refill_0"].split()[:4] == ["0", "0", "0", "1"] == got["refill_2"].split()[:4] == got["refill_3"].split()[:4]
    assert got["refill_1"].split()[:4] == ["0", "0", "0", "9"] and "count" in got["refill_1"]
    # verdict records: code, tier, index, flags (1 written, 4 the last refill did not take, 8 no live item), text
    assert got["verdict_0_0"].split() == ["0", "0", "0", "1"] == got["verdict_0_1"].split()
    assert got["verdict_0_2"].split()[:4] == ["0", "0", "0", "9"] and "no live item" in got["verdict_0_2"]
    for g in range(3):
        assert got["verdict_1_%d" % g].split()[:4] == ["0", "0", "0", "5"]
        assert got["verdict_2_%d" % g].split() == ["0", "0", "0", "1"] == got["verdict_3_%d" % g].split()
    # weights: non-zero for live items, zero rows for dead ones; the groups below the cut draw what they draw in the full batch
    assert [got["weights_%d" % k] for k in range(4)] == ["111100", "000000", "111111", "111111"]
    assert got["same_weights"] == "1 1"
    assert got["stats"] == "4 1 0"
    assert "count_dev" in got["refused"]
