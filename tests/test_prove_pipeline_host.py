"""CPU suite: the host side of the prove pipeline (bpp_prove_submit / bpp_prove_collect).  The job copy submit takes of its
caller's items (csrc/prove_job_host.h: the per-item check, the deep copy, the wipe) runs under AddressSanitizer + UBSan
(csrc/hosttest_prove_job.cpp) and through libbpp_hosttest.so; the entry points refuse a null context without a GPU; the C++ and
Python faces exist."""
import ctypes
import importlib
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_HANDLE, INVALID_ARGUMENT, INVALID_LENGTH = -3, 2, 3


def test_job_copy_under_asan_ubsan():
    pkg = importlib.import_module("bulletproofs-plus_amd")
    exe = pkg._build.build_prove_job_harness()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.split("\n")
    for case in ("optional_fields", "failing_items_beside_passing", "copy_survives_the_source", "wiped_before_freed"):
        assert "ok " + case in lines, (case, r.stdout[-2000:])
    assert "all ok" in lines
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-4000:]


def test_job_copy_in_the_host_library():
    """ht_prove_job_copy (libbpp_hosttest.so): items over bytearrays this test owns; the check's codes, the number copied, and the
    probe's own comparison (copy == source, all zero after the wipe)"""
    pkg = importlib.import_module("bulletproofs-plus_amd")
    lib = ctypes.CDLL(pkg._build.build_hosttest())
    Item = pkg._lib.ProveItem
    lib.ht_prove_job_copy.restype = ctypes.c_int
    lib.ht_prove_job_copy.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(Item), ctypes.c_size_t,
                                      ctypes.c_size_t, ctypes.c_int, ctypes.c_size_t, ctypes.POINTER(ctypes.c_int),
                                      ctypes.POINTER(ctypes.c_size_t)]
    n_bits, m_max, t = 8, 4, 1
    keep = []

    def buf(data):
        b = (ctypes.c_uint8 * len(data)).from_buffer(bytearray(data))
        keep.append(b)
        return ctypes.cast(b, ctypes.c_void_p)

    ms = [1, 2, 3, 4, 0, 8, 4, 1]
    items = (Item * len(ms))()
    for i, m in enumerate(ms):
        mm = max(m, 1)
        rounds = max((n_bits * mm).bit_length() - 1, 0)
        items[i].values = buf(b"".join((17 + j).to_bytes(8, "little") for j in range(mm)))
        items[i].blindings32 = buf(bytes([3] * 31 + [0]) * (mm * t))
        items[i].commitments32 = buf(bytes([9]) * (32 * mm))
        items[i].m = m
        items[i].transcript_label = buf(b"label")
        items[i].label_len = 5
        items[i].rng_bytes = buf(bytes([5]) * (32 * (rounds + 3)))
        items[i].rng_len = 32 * (rounds + 3) - (32 if i == 6 else 0)  # item 6: one draw short
    items[7].seed_nonce32 = buf(bytes([0xff]) * 32)  # not canonical
    codes = (ctypes.c_int * len(ms))()
    size = ctypes.c_size_t()
    copied = lib.ht_prove_job_copy(n_bits, m_max, t, items, len(ms), 4096, 0, 0, codes, ctypes.byref(size))
    assert list(codes) == [0, 0, INVALID_ARGUMENT, 0, INVALID_ARGUMENT, INVALID_ARGUMENT, INVALID_LENGTH, INVALID_ARGUMENT]
    assert copied == 3 and size.value >= sum(8 * m + 32 * m + 32 * m + 32 * ((8 * m).bit_length() + 2) for m in (1, 2, 4))
    # as openings items with a commit_stride that holds two commitments: the m = 4 item fails on it
    copied = lib.ht_prove_job_copy(n_bits, m_max, t, items, len(ms), 4096, 1, 64, codes, ctypes.byref(size))
    assert list(codes)[:4] == [0, 0, INVALID_ARGUMENT, INVALID_LENGTH] and copied == 2


def test_entry_points_refuse_a_null_context_without_a_gpu():
    pkg = importlib.import_module("bulletproofs-plus_amd")
    pkg._build.build()
    lib = pkg._lib.load()
    ticket = ctypes.c_uint64(77)
    err = ctypes.create_string_buffer(64)
    items = (pkg._lib.ProveItem * 1)()
    assert lib.bpp_prove_submit(None, 1, items, 1, 4096, 0, 0, ctypes.byref(ticket), err, 64) == BAD_HANDLE
    assert ticket.value == 77
    out = (ctypes.c_uint8 * 4096)()
    lens = (ctypes.c_size_t * 1)()
    assert lib.bpp_prove_collect(None, 1, None, out, lens, None, err, 64) == BAD_HANDLE
    assert lib.bpp_prove_pipeline_depth(None, 2) == BAD_HANDLE
    done = ctypes.c_int(5)
    assert lib.bpp_prove_ticket_done(None, 1, ctypes.byref(done)) == BAD_HANDLE and done.value == 5


def test_bpp_hpp_prove_pipeline_compiles():
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "prove_pipeline_hpp.cpp")], check=True, timeout=300)


def test_python_prove_pipeline_exists():
    packed = importlib.import_module("bulletproofs-plus_amd.packed")
    for name in ("submit", "submit_openings", "done", "collect", "close"):
        assert callable(getattr(packed.ProvePipeline, name)), name
