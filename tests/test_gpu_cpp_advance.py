"""GPU test: the advancing forms of the C++ mirror (include/bpp.hpp: Transcript's own operations, and verify_batch / prove_batch /
prove_with_rng with their transcripts by pointer) from compiled code, tests/cpp/advance_mirror.cpp.  What the program prints --
the proof, the transcript the prover left, the one the verifier left, a challenge drawn from each afterwards -- is held to
oracle.pyref, whose prove_with_rng and verify advance their Transcript objects in place."""
import importlib
import os
import subprocess

import pytest

from oracle.pyref import merlin as M
from oracle.pyref import protocol as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_advancing_forms_equal_the_oracle(tmp_path):
    pkg = importlib.import_module("bulletproofs-plus_amd")
    lib = pkg._build.build()
    exe = str(tmp_path / "advance_mirror")
    libdir = os.path.dirname(lib)
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "advance_mirror.cpp"),
                    "-o", exe, "-L", libdir, "-lbpp_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "advance_mirror ok" in out.stdout, (out.stdout[-500:], out.stderr[-2000:])
    names = ("proof", "prover_state", "verifier_state", "prover_after", "verifier_after")  # the lines "<name> <hex>" of its output
    got = {k: bytes.fromhex(v) for k, v in (line.split(" ", 1) for line in out.stdout.splitlines() if line.split(" ", 1)[0] in names)}
    assert sorted(got) == sorted(names)

    def start():
        t = M.Transcript(b"outer protocol v1")
        t.append_message(b"context", b"block 42")
        t.append_u64(b"height", 42)
        return t
    params = O.RangeParameters(64, 1, O.PedersenGens(1))
    st = O.RangeStatement(params, [params.pc_gens.commit(123456789, [7])], [None], None)
    w = O.RangeWitness([O.CommitmentOpening(123456789, [7])])
    tp = start()
    proof = O.prove_with_rng(tp, st, w, M.ByteStreamRng(bytes(i & 0xff for i in range(32 * 9))))
    assert got["proof"] == proof.to_bytes()
    assert got["prover_state"] == tp.strobe.to_bytes()
    tv = start()
    O.verify([tv], [st], [proof], 0)
    assert got["verifier_state"] == tv.strobe.to_bytes()
    assert got["prover_after"] == tp.challenge_bytes(b"after", 32)
    assert got["verifier_after"] == tv.challenge_bytes(b"after", 32)
