"""GPU test: bpp_batch_refill_enqueue_live of include/bpp.h through the mirror of include/bpp.hpp from compiled code with arrays the
program hipMalloc'ed itself, tests/cpp/refill_live.cpp: a batch of six proofs refilled under the mask {1, 0, 0, 0, 255, 2} (a proof
that does not verify and a non-canonical scalar lie at dead slots) and verified in chunks of two, against a fresh upload of items 0,
4 and 5 alone with the boundaries [0, 1, 3]; the weights copied out behind both enqueues, one wait at the end."""
import importlib
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_refill_under_a_mask(tmp_path):
    pkg = importlib.import_module("bulletproofs-plus_amd")
    lib = pkg._build.build()
    exe = str(tmp_path / "refill_live")
    libdir = os.path.dirname(lib)
    subprocess.run(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                    os.path.join(ROOT, "tests", "cpp", "refill_live.cpp"), "-o", exe, "-L", libdir, "-lbpp_hip", "-L/opt/rocm/lib",
                    "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "refill live ok" in out.stdout, (out.stdout[-500:], out.stderr[-2000:])
    got = dict(line.split(" ", 1) for line in out.stdout.splitlines() if " " in line)
    # the refill record: code, tier, index, flags (1 written), text
    assert got["record"].split()[:4] == ["0", "0", "0", "1"]
    # verdict records: code, tier, index, flags (1 written, 8 no live item), text; live groups as the fresh upload's
    assert got["reference_0"].split() == ["0", "0", "0", "1"] == got["reference_1"].split()
    assert got["verdict_0"].split() == got["reference_0"].split() and got["verdict_2"].split() == got["reference_1"].split()
    assert got["verdict_1"].split()[:4] == ["0", "0", "0", "9"] and "no live item" in got["verdict_1"]
    # weights: the fresh upload's at live slots, zero rows at dead ones
    assert got["weights"] == "100011" + "111"
    assert got["same_weights"] == "1"
    assert got["stats"] == "1 1 0"
    assert "live_dev" in got["refused"]
