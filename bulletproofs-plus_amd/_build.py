"""Build libbpp_hip.so (gfx950) in-tree with hipcc.  Called by __graft_entry__.build() and by tests."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libbpp_hip.so")
HOSTTEST_LIB = os.path.join(HERE, "libbpp_hosttest.so")
SOURCES = ["engine.hip"]
# every header / include file next to the sources is a dependency (a stale .so after a header-only edit is a silent trap)
HEADERS = sorted(f for f in os.listdir(CSRC) if f.endswith((".h", ".inc"))) + [os.path.join("..", "..", "include", "bpp.h")]


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps if os.path.exists(d))


def hipcc_path():
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if cand and (os.path.isabs(cand) and os.path.exists(cand) or not os.path.isabs(cand)):
            return cand
    return "hipcc"


def build(force=False, verbose=False):
    """Compile every HIP source for gfx950 into libbpp_hip.so (cross-compiles without a GPU)."""
    deps = [os.path.join(CSRC, s) for s in SOURCES] + [os.path.join(CSRC, h) for h in HEADERS]
    if not force and not _stale(LIB, deps):
        return LIB
    cmd = [hipcc_path(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-shared", "-fPIC",
           "-o", LIB] + os.environ.get("BPP_HIPCC_FLAGS", "").split() + [os.path.join(CSRC, s) for s in SOURCES]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True, cwd=CSRC)
    _check_isa_hazards(LIB)
    return LIB


def _check_isa_hazards(lib):
    """Refuse a code object in which a DPP result is read as store data by the very next instruction, or which holds a
    v_subrev in DPP form (both wrong on the MI355X; the compiler guards against neither): tools/isa/dpp_hazard_check.py
    disassembles what was just built.  A build that CANNOT be checked -- no llvm-objdump next to the hipcc in use, in the
    usual ROCm prefixes or on PATH -- fails as well, unless BPP_SKIP_ISA_CHECK=1 says so explicitly: a verifier must not
    ship unchecked by accident."""
    script = os.path.join(os.path.dirname(HERE), "tools", "isa", "dpp_hazard_check.py")
    import importlib.util
    spec = importlib.util.spec_from_file_location("dpp_hazard_check", script)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    llvm = mod.llvm_bin(hipcc_path())
    if llvm is None:
        if os.environ.get("BPP_SKIP_ISA_CHECK") == "1":
            print("WARNING: libbpp_hip.so built WITHOUT the gfx950 DPP hazard check (no llvm-objdump; BPP_SKIP_ISA_CHECK=1)", file=sys.stderr)
            return
        os.remove(lib)
        raise RuntimeError("cannot disassemble the built code object (llvm-objdump / llvm-objcopy not found next to %s, in /opt/rocm "
                           "or on PATH): the gfx950 DPP hazard check is mandatory; set BPP_SKIP_ISA_CHECK=1 to build without it" % hipcc_path())
    mod.LLVM = llvm
    _, hits = mod.check(lib)
    if hits:
        os.remove(lib)
        raise RuntimeError("gfx950 hazard in the built code object: DPP result stored by the next instruction: %s" % (hits[:3],))


def build_hosttest(force=False):
    """Host-compiled probes of the shared host/device arithmetic headers (CPU test suite only)."""
    src = os.path.join(CSRC, "hosttest.cpp")
    deps = [src] + [os.path.join(CSRC, h) for h in HEADERS]
    if not force and not _stale(HOSTTEST_LIB, deps):
        return HOSTTEST_LIB
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", HOSTTEST_LIB, src], check=True, cwd=CSRC)
    return HOSTTEST_LIB


SANITIZER_BIN = os.path.join(HERE, "hosttest_upload_asan")


def build_sanitizer_harness(force=False):
    """hosttest_upload.cpp (host packer of bpp_batch_upload + the arithmetic probes) under ASan + UBSan: an executable,
    run by tests/test_host_sanitizers.py.  GPU sanitizers are not available on the pool; this is the CPU build."""
    src = os.path.join(CSRC, "hosttest_upload.cpp")
    deps = [src, os.path.join(CSRC, "hosttest.cpp")] + [os.path.join(CSRC, h) for h in HEADERS]
    if not force and not _stale(SANITIZER_BIN, deps):
        return SANITIZER_BIN
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", "-DBPP_FE_BOUNDS_CHECK", "-o", SANITIZER_BIN, src], check=True, cwd=CSRC)
    return SANITIZER_BIN


PROVE_JOB_SANITIZER_BIN = os.path.join(HERE, "hosttest_prove_job_asan")


def build_prove_job_harness(force=False):
    """hosttest_prove_job.cpp (the job copy bpp_prove_submit takes of its caller's items: per-item check, deep copy, wipe) under
    ASan + UBSan: an executable, run by tests/test_prove_pipeline_host.py."""
    src = os.path.join(CSRC, "hosttest_prove_job.cpp")
    deps = [src] + [os.path.join(CSRC, h) for h in HEADERS]
    if not force and not _stale(PROVE_JOB_SANITIZER_BIN, deps):
        return PROVE_JOB_SANITIZER_BIN
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", "-o", PROVE_JOB_SANITIZER_BIN, src], check=True, cwd=CSRC)
    return PROVE_JOB_SANITIZER_BIN


LANES_BINS = {"tsan": os.path.join(HERE, "hosttest_lanes_tsan"), "asan": os.path.join(HERE, "hosttest_lanes_asan")}
LANES_FLAGS = {"tsan": ["-fsanitize=thread"], "asan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]}


def build_lanes_harness(kind, force=False):
    """hosttest_lanes.cpp (lanes_host.h: the submit/collect and the leader protocol behind the pipelines, the batcher and the prove
    pool) under ThreadSanitizer (kind "tsan") or ASan + UBSan ("asan"): an executable, run by tests/test_lanes_host.py."""
    src = os.path.join(CSRC, "hosttest_lanes.cpp")
    exe = LANES_BINS[kind]
    if not force and not _stale(exe, [src, os.path.join(CSRC, "lanes_host.h")]):
        return exe
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-pthread"] + LANES_FLAGS[kind] + ["-o", exe, src], check=True, cwd=CSRC)
    return exe


RUNTIME_BINS = {"tsan": os.path.join(HERE, "hosttest_runtime_tsan"), "asan": os.path.join(HERE, "hosttest_runtime_asan")}


def build_runtime_harness(kind, force=False):
    """hosttest_runtime.cpp (runtime_host.h: the small-call gate, the host worker pool, the wait schedule; chain_host.h: the chain
    scheduler) under ThreadSanitizer (kind "tsan") or ASan + UBSan ("asan"): an executable, run by tests/test_runtime_host.py."""
    src = os.path.join(CSRC, "hosttest_runtime.cpp")
    exe = RUNTIME_BINS[kind]
    if not force and not _stale(exe, [src] + [os.path.join(CSRC, h) for h in HEADERS]):
        return exe
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-pthread"] + LANES_FLAGS[kind] + ["-o", exe, src], check=True, cwd=CSRC)
    return exe


CT_SANITIZER_BIN = os.path.join(HERE, "hosttest_ct_asan")


def build_ct_harness(force=False):
    """hosttest_ct.cpp (ct.h: the one-lane model of the constant-time multiscalar multiplication; ct_plan.h: its chunk planner)
    under ASan + UBSan: an executable, run by tests/test_msm_ct_host.py."""
    src = os.path.join(CSRC, "hosttest_ct.cpp")
    deps = [src, os.path.join(CSRC, "hosttest.cpp")] + [os.path.join(CSRC, h) for h in HEADERS]
    if not force and not _stale(CT_SANITIZER_BIN, deps):
        return CT_SANITIZER_BIN
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", "-o", CT_SANITIZER_BIN, src], check=True, cwd=CSRC)
    return CT_SANITIZER_BIN


INGEST_SANITIZER_BIN = os.path.join(HERE, "hosttest_ingest_asan")


def build_ingest_harness(force=False):
    """hosttest_ingest.cpp (ingest.h: the one-item routines of the device form of the packed upload, held to the host packer of
    upload_host.h over a corpus) under ASan + UBSan: an executable, run by tests/test_ingest_host.py."""
    src = os.path.join(CSRC, "hosttest_ingest.cpp")
    deps = [src] + [os.path.join(CSRC, h) for h in HEADERS]
    if not force and not _stale(INGEST_SANITIZER_BIN, deps):
        return INGEST_SANITIZER_BIN
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", "-o", INGEST_SANITIZER_BIN, src], check=True, cwd=CSRC)
    return INGEST_SANITIZER_BIN


VERDICT_SANITIZER_BIN = os.path.join(HERE, "hosttest_verdict_asan")


def build_verdict_harness(force=False):
    """hosttest_verdict.cpp (verdict.h: the verdict resolution that bpp_verify_enqueue runs on the device, held to the throwing
    routines of upload_host.h) under ASan + UBSan: an executable, run by tests/test_verdict_host.py."""
    src = os.path.join(CSRC, "hosttest_verdict.cpp")
    deps = [src] + [os.path.join(CSRC, h) for h in HEADERS]
    if not force and not _stale(VERDICT_SANITIZER_BIN, deps):
        return VERDICT_SANITIZER_BIN
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", "-o", VERDICT_SANITIZER_BIN, src], check=True, cwd=CSRC)
    return VERDICT_SANITIZER_BIN


REFILL_SANITIZER_BIN = os.path.join(HERE, "hosttest_refill_asan")


def build_refill_harness(force=False):
    """hosttest_refill.cpp (refill.h: the one-lane model of the kernels of bpp_batch_refill_enqueue, held to the device upload's
    routines of ingest.h; verdict.h with a refill state) under ASan + UBSan: an executable, run by tests/test_refill_host.py."""
    src = os.path.join(CSRC, "hosttest_refill.cpp")
    deps = [src] + [os.path.join(CSRC, h) for h in HEADERS]
    if not force and not _stale(REFILL_SANITIZER_BIN, deps):
        return REFILL_SANITIZER_BIN
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", "-o", REFILL_SANITIZER_BIN, src], check=True, cwd=CSRC)
    return REFILL_SANITIZER_BIN


REFILL_COUNT_SANITIZER_BIN = os.path.join(HERE, "hosttest_refill_count_asan")


def build_refill_count_harness(force=False):
    """hosttest_refill_count.cpp (refill.h with a live count: the one-lane model of the kernels of bpp_batch_refill_enqueue_count, held
    to the device upload's routines on the first c items; verdict.h: the live routines on cut groups) under ASan + UBSan: an
    executable, run by tests/test_refill_count_host.py."""
    src = os.path.join(CSRC, "hosttest_refill_count.cpp")
    deps = [src] + [os.path.join(CSRC, h) for h in HEADERS]
    if not force and not _stale(REFILL_COUNT_SANITIZER_BIN, deps):
        return REFILL_COUNT_SANITIZER_BIN
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", "-o", REFILL_COUNT_SANITIZER_BIN, src], check=True, cwd=CSRC)
    return REFILL_COUNT_SANITIZER_BIN


REFILL_LIVE_SANITIZER_BIN = os.path.join(HERE, "hosttest_refill_live_asan")


def build_refill_live_harness(force=False):
    """hosttest_refill_live.cpp (refill.h under a live mask: the one-lane model of the kernels of bpp_batch_refill_enqueue_live, held
    to the device upload's routines on the live items alone; verdict.h: the live routines on compacted groups) under ASan + UBSan: an
    executable, run by tests/test_refill_live_host.py."""
    src = os.path.join(CSRC, "hosttest_refill_live.cpp")
    deps = [src] + [os.path.join(CSRC, h) for h in HEADERS]
    if not force and not _stale(REFILL_LIVE_SANITIZER_BIN, deps):
        return REFILL_LIVE_SANITIZER_BIN
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", "-o", REFILL_LIVE_SANITIZER_BIN, src], check=True, cwd=CSRC)
    return REFILL_LIVE_SANITIZER_BIN


INGEST_MIXED_SANITIZER_BIN = os.path.join(HERE, "hosttest_ingest_mixed_asan")


def build_ingest_mixed_harness(force=False):
    """hosttest_ingest_mixed.cpp (ingest_mixed.h: the one-item routines, the host prelude and the plan of the device form of the mixed
    upload, held to the item form of upload_host.h over a corpus) under ASan + UBSan: an executable, run by
    tests/test_ingest_mixed_host.py."""
    src = os.path.join(CSRC, "hosttest_ingest_mixed.cpp")
    deps = [src] + [os.path.join(CSRC, h) for h in HEADERS]
    if not force and not _stale(INGEST_MIXED_SANITIZER_BIN, deps):
        return INGEST_MIXED_SANITIZER_BIN
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", "-o", INGEST_MIXED_SANITIZER_BIN, src], check=True, cwd=CSRC)
    return INGEST_MIXED_SANITIZER_BIN


REFILL_MIXED_SANITIZER_BIN = os.path.join(HERE, "hosttest_refill_mixed_asan")


def build_refill_mixed_harness(force=False):
    """hosttest_refill_mixed.cpp (refill_mixed.h: the one-lane model of the kernels of bpp_batch_refill_enqueue_mixed, plain, with a
    count and under a mask, held to the device form of the mixed upload on the rows in question) under ASan + UBSan: an executable, run
    by tests/test_refill_mixed_host.py."""
    src = os.path.join(CSRC, "hosttest_refill_mixed.cpp")
    deps = [src] + [os.path.join(CSRC, h) for h in HEADERS]
    if not force and not _stale(REFILL_MIXED_SANITIZER_BIN, deps):
        return REFILL_MIXED_SANITIZER_BIN
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", "-o", REFILL_MIXED_SANITIZER_BIN, src], check=True, cwd=CSRC)
    return REFILL_MIXED_SANITIZER_BIN


ITEM_STATES_SANITIZER_BIN = os.path.join(HERE, "hosttest_item_states_asan")


def build_item_states_harness(force=False):
    """hosttest_item_states.cpp (item_states.h: the one-lane models of k_item_states -- every row, a live count, a live mask -- held to
    the states table and tr_err_index upload_host.h makes of the equivalent item array, and the row rule of k_states_out) under
    ASan + UBSan: an executable, run by tests/test_item_states_host.py."""
    src = os.path.join(CSRC, "hosttest_item_states.cpp")
    deps = [src] + [os.path.join(CSRC, h) for h in HEADERS]
    if not force and not _stale(ITEM_STATES_SANITIZER_BIN, deps):
        return ITEM_STATES_SANITIZER_BIN
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", "-o", ITEM_STATES_SANITIZER_BIN, src], check=True, cwd=CSRC)
    return ITEM_STATES_SANITIZER_BIN


PROVE_INGEST_SANITIZER_BIN = os.path.join(HERE, "hosttest_prove_ingest_asan")


def build_prove_ingest_harness(force=False):
    """hosttest_prove_ingest.cpp (prove_ingest.h: the per-item routines of k_prove_ingest and the host plan of
    bpp_prove_openings_device, held to ProvePack::pack and prove_item_check_host on the sorted equivalent items) under ASan + UBSan:
    an executable, run by tests/test_prove_ingest_host.py."""
    src = os.path.join(CSRC, "hosttest_prove_ingest.cpp")
    deps = [src] + [os.path.join(CSRC, h) for h in HEADERS]
    if not force and not _stale(PROVE_INGEST_SANITIZER_BIN, deps):
        return PROVE_INGEST_SANITIZER_BIN
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", "-o", PROVE_INGEST_SANITIZER_BIN, src], check=True, cwd=CSRC)
    return PROVE_INGEST_SANITIZER_BIN


if __name__ == "__main__":
    build(force="--force" in sys.argv, verbose=True)
    build_hosttest(force="--force" in sys.argv)
