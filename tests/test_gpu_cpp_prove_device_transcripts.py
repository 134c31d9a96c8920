"""GPU test: bpp_prove_openings_device_transcripts of include/bpp.h through the overload of RangeProof::prove_openings of
include/bpp.hpp that takes the two device pointers, from compiled code with arrays the program hipMalloc'ed itself (the rows going
in and coming out at odd byte addresses), tests/cpp/prove_device_transcripts.cpp.  The commitments, proofs and advanced transcripts
the program prints must equal what bpp_prove_openings_states gives here, through the Python mirror, on the same openings under the
same per-item transcripts; the outputs must be accepted by Engine::verify_enqueue_states under the rows they continued."""
import ctypes
import importlib
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MS, M_STRIDE, ROW = [2, 1, 1], 4, 203


def _host_form(bpp, engine):
    """the program's inputs, formula for formula, through bpp_prove_openings_states -> (commitments, proofs, states) per item"""
    packed = importlib.import_module("bulletproofs-plus_amd.packed")
    params = bpp.RangeParameters.init(8, 4, bpp.create_pedersen_gens_with_extension_degree(1), engine=engine)
    n, rng_stride = 3, 32 * 7 + 5
    values = np.full((n, M_STRIDE), 2 ** 64 - 1, dtype=np.uint64)
    blind = np.full((n, M_STRIDE, 1, 32), 0xFF, dtype=np.uint8)
    ext = np.full((n, rng_stride), 0xFF, dtype=np.uint8)
    rows = np.zeros((n, ROW), dtype=np.uint8)
    for i, m in enumerate(MS):
        for j in range(m):
            values[i, j] = 10 * i + j + 1
            blind[i, j, 0] = [(7 * i + 3 * j + k + 1) & 0xFF if k < 31 else 0 for k in range(32)]
        need = 32 * (3 + 3 + (m > 1))
        ext[i, :need] = [(31 * i + 5 * k + 3) & 0xFF for k in range(need)]
        tr = bpp.Transcript.new(b"prove device transcripts")
        tr.append_message(b"tx", bytes([i + 1]) * (5 + 11 * i))
        rows[i] = np.frombuffer(tr.state, dtype=np.uint8)
    items = np.zeros(n, dtype=packed._PROVE_ITEM)
    items["values"], items["blindings32"], items["m"] = packed._rows(values), packed._rows(blind), MS
    items["transcript_state"] = packed._rows(rows)
    items["rng_bytes"], items["rng_len"] = packed._rows(ext), rng_stride
    ps, cs = 1 + 32 * (1 + 5 + 2 * 4), 32 * M_STRIDE
    proofs, commits, states = np.zeros((n, ps), dtype=np.uint8), np.zeros((n, cs), dtype=np.uint8), np.zeros((n, ROW), dtype=np.uint8)
    lens, codes, err = np.zeros(n, dtype=np.uintp), np.zeros(n, dtype=np.intc), ctypes.create_string_buffer(256)
    rc = engine.lib.bpp_prove_openings_states(engine.ctx, params.handle, items.ctypes.data_as(ctypes.POINTER(packed._lib.ProveItem)), n,
                                              commits.ctypes.data, cs, proofs.ctypes.data, ps, lens.ctypes.data_as(ctypes.POINTER(ctypes.c_size_t)),
                                              codes.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), states.ctypes.data, err, 256)
    assert rc == 0, err.value
    return [(bytes(commits[i, :32 * m]).hex(), bytes(proofs[i, :int(lens[i])]).hex(), bytes(states[i]).hex()) for i, m in enumerate(MS)]


def test_cpp_prove_device_transcripts_equal_the_host_form(bpp, engine, tmp_path):
    pkg = importlib.import_module("bulletproofs-plus_amd")
    lib = pkg._build.build()
    exe = str(tmp_path / "prove_device_transcripts")
    libdir = os.path.dirname(lib)
    subprocess.run(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"), "-I/opt/rocm/include",
                    os.path.join(ROOT, "tests", "cpp", "prove_device_transcripts.cpp"), "-o", exe, "-L", libdir, "-lbpp_hip", "-L/opt/rocm/lib",
                    "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "prove_device_transcripts ok" in out.stdout, (out.stdout[-500:], out.stderr[-2000:])
    got = dict(line.split(" ", 1) for line in out.stdout.splitlines() if " " in line)
    assert got["code"] == "0 ''"
    for i, (commitments, proof, state) in enumerate(_host_form(bpp, engine)):
        assert got["commitments_%d" % i] == commitments, i
        assert got["proof_%d" % i] == proof, "proof %d differs from bpp_prove_openings_states on the same openings" % i
        assert got["state_%d" % i] == state, "advanced transcript %d differs" % i
    assert got["finding"] == "2 020 'transcript state has pos >= rate'" and got["finding_row_zero"] == "1"
    assert got["refusal"].startswith("2 ") and "item_states_dev" in got["refusal"]
    assert got["upload_code"].split()[0] == "0" and got["verify_code"] == "0 ''" and got["verifier_rows_advanced"] == "1"
    assert got["stats"] == "3 9 1 0"
