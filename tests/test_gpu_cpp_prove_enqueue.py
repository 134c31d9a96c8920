"""GPU test: bpp_prove_plan_create / bpp_prove_enqueue of include/bpp.h through Engine::prove_plan_create, the RAII Engine::ProvePlan
and Engine::prove_enqueue of include/bpp.hpp, from compiled code with arrays the program hipMalloc'ed itself
(tests/cpp/prove_enqueue.cpp).  The program holds an enqueue, byte for byte over whole prefilled buffers, to the blocking
RangeProof::prove_openings over the same device arrays, and runs the loop prove_enqueue -> batch_refill_enqueue_mixed(live = the
prover's ok mask) -> verify_enqueue_states with one wait at its end; it checks its own results and prints what it found."""
import importlib
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_prove_enqueue_parity_and_the_loop(tmp_path):
    pkg = importlib.import_module("bulletproofs-plus_amd")
    lib = pkg._build.build()
    exe = str(tmp_path / "prove_enqueue")
    libdir = os.path.dirname(lib)
    subprocess.run(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                    os.path.join(ROOT, "tests", "cpp", "prove_enqueue.cpp"), "-o", exe, "-L", libdir, "-lbpp_hip", "-L/opt/rocm/lib",
                    "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "prove_enqueue ok" in out.stdout, (out.stdout[-500:], out.stderr[-2000:])
    got = dict(line.split(" ", 1) for line in out.stdout.splitlines() if " " in line)
    assert got["parity"] == "ok"
    assert got["refusal"].startswith("2 ") and "item_states_dev is null" in got["refusal"]
    assert got["ok_mask"] == "1010"
    assert got["summary"] == "2 3 2 1 1 'blinding factor is not canonical'"
    assert got["verify_code"] == "0 ''"
