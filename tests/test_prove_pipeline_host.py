"""CPU suite: the host side of the prove pipeline (bpp_prove_submit / bpp_prove_collect).  The job copy submit takes of its
caller's items (csrc/prove_job_host.h: the per-item check, the deep copy, the wipe) runs under AddressSanitizer + UBSan
(csrc/hosttest_prove_job.cpp) and through libbpp_hosttest.so; the entry points refuse a null context without a GPU; the C++ and
Python faces exist.  The prover's witness packer (csrc/prove_pack_host.h) is driven by the same two harnesses."""
import ctypes
import importlib
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_HANDLE, INVALID_ARGUMENT, INVALID_LENGTH = -3, 2, 3


def test_job_copy_under_asan_ubsan():
    pkg = importlib.import_module("bulletproofs-plus_amd")
    exe = pkg._build.build_prove_job_harness()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.split("\n")
    for case in ("optional_fields", "failing_items_beside_passing", "copy_survives_the_source", "wiped_before_freed",
                 "pack_uniform_and_mixed", "pack_openings", "pack_transcripts", "pack_failing_item_at_every_position",
                 "pack_wiped_by_wipe_and_by_the_destructor"):
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


def _rounds(n_bits, m):
    return (n_bits * m).bit_length() - 1


@pytest.mark.parametrize("t", [1, 3])
@pytest.mark.parametrize("openings", [0, 1])
def test_prove_pack_in_the_host_library(t, openings):
    """ht_prove_pack (libbpp_hosttest.so, csrc/prove_pack_host.h): a mixed call's items packed; the descriptors' offsets, the
    packed bytes, roff / mslot and the minimum-value rows against values this test lays out on its own, the 203-byte states against
    oracle.pyref.merlin after the seven call-level appends"""
    from oracle.pyref import merlin as M
    pkg = importlib.import_module("bulletproofs-plus_amd")
    lib = ctypes.CDLL(pkg._build.build_hosttest())
    Item = pkg._lib.ProveItem
    n_bits, m_max = 8, 4
    rnd = random.Random(1000 * t + openings)
    keep = []

    def buf(data):
        b = (ctypes.c_uint8 * max(len(data), 1)).from_buffer(bytearray(data) or bytearray(1))
        keep.append(b)
        return ctypes.cast(b, ctypes.c_void_p)

    def scalar():
        return rnd.getrandbits(250).to_bytes(32, "little")

    hg = bytes(rnd.getrandbits(8) for _ in range(32 * (t + 1)))
    outer = M.Transcript(b"outer protocol")
    outer.append_message(b"ctx", b"pack")
    state = outer.strobe.to_bytes()
    # (m, transcript): L1 / L2 labels, S a state; items 0-1 share ONE label buffer, 2 has the same label in a buffer of its own,
    # 5 and 7 the same state bytes at two addresses; the same label under another m is another state
    plan = [(4, "L1"), (4, "L1"), (4, "L1copy"), (2, "L2"), (2, "L1"), (2, "S"), (1, "L1"), (1, "S"), (1, "S2")]
    shared_label = buf(b"label one")
    items = (Item * len(plan))()
    want_bytes, want_desc, want_states, state_ids, py = b"", [], [], {}, []
    m0, r0 = plan[0][0], _rounds(n_bits, plan[0][0])
    for i, (m, tr) in enumerate(plan):
        rounds = _rounds(n_bits, m)
        vals = [rnd.getrandbits(n_bits) for _ in range(m)]
        blinds = [scalar() for _ in range(m * t)]
        comms = bytes(rnd.getrandbits(8) for _ in range(32 * m)) if not (openings and i % 3 == 1) else None
        mins = [(v // 2 if (i + j) % 2 else None) for j, v in enumerate(vals)] if i % 2 == 0 else None
        seed = scalar() if m == 1 and i != 7 else None
        ext = bytes(rnd.getrandbits(8) for _ in range(32 * (rounds + 3) + (40 if i == 3 else 0)))  # (item 3 brings more than is read)
        items[i].values = buf(b"".join(v.to_bytes(8, "little") for v in vals))
        items[i].blindings32 = buf(b"".join(blinds))
        items[i].commitments32 = buf(comms) if comms else None
        items[i].m = m
        if mins:
            items[i].min_values = buf(b"".join((x or 0).to_bytes(8, "little") for x in mins))
            items[i].min_present = buf(bytes(x is not None for x in mins))
        items[i].seed_nonce32 = buf(seed) if seed else None
        if tr.startswith("S"):
            items[i].transcript_state = buf(state)
            base, key = outer.clone(), ("S", m)
        else:
            label = b"label one" if tr.startswith("L1") else b"label two"
            items[i].transcript_label = shared_label if tr == "L1" and i < 2 else buf(label)
            items[i].label_len = len(label)
            base, key = M.Transcript(label), (label, m)
        items[i].rng_bytes = buf(ext)
        items[i].rng_len = len(ext)
        if key not in state_ids:
            state_ids[key] = len(want_states)
            base.append_message(b"dom-sep", b"Bulletproofs+ Range Proof")
            base.append_message(b"H", hg[:32])
            for k in range(t):
                base.append_message(b"G", hg[32 * (k + 1):32 * (k + 2)])
            base.append_u64(b"N", n_bits)
            base.append_u64(b"T", t)
            base.append_u64(b"M", m)
            want_states.append(base.strobe.to_bytes())
        wit_off = len(want_bytes)
        for j in range(m):
            want_bytes += vals[j].to_bytes(8, "little") + b"".join(blinds[j * t:(j + 1) * t])
        commit_off = len(want_bytes)
        want_bytes += comms or bytes(32 * m)
        ext_off = len(want_bytes)
        want_bytes += ext[:32 * (rounds + 3)]
        seed_off = len(want_bytes)
        want_bytes += seed or bytes(32)
        flags = (1 if seed else 0) | (0 if comms else 2)
        want_desc.append([m, wit_off, commit_off, ext_off, i * m0, state_ids[key], flags, seed_off, r0 - rounds, m0])
        py.append((mins, m))
    n = len(plan)
    desc = (ctypes.c_uint32 * (10 * n))()
    sizes = (ctypes.c_uint64 * 6)()
    out_bytes = (ctypes.c_uint8 * (len(want_bytes) + 64))()
    out_states = (ctypes.c_uint8 * (203 * n))()
    minvals = (ctypes.c_uint64 * (n * m0))()
    minpres = (ctypes.c_uint8 * (n * m0))()
    roff = (ctypes.c_uint32 * n)()
    wiped = ctypes.c_int(0)
    msg = ctypes.create_string_buffer(160)
    lib.ht_prove_pack.restype = ctypes.c_int

    def pack(count, mixed, opn):
        return lib.ht_prove_pack(ctypes.c_uint32(n_bits), ctypes.c_uint32(m_max), ctypes.c_uint32(t), hg, items, ctypes.c_size_t(count),
                                 mixed, opn, desc, sizes, out_bytes, ctypes.c_size_t(len(out_bytes)), out_states,
                                 ctypes.c_size_t(len(out_states)), minvals, minpres, roff, ctypes.byref(wiped), msg, ctypes.c_size_t(160))

    assert pack(n, 1, openings) == 0, msg.value
    assert list(sizes) == [m0, r0, _rounds(n_bits, 1), 1 + 32 * (t + 5 + 2 * r0), len(want_bytes), 203 * len(want_states)]
    assert [list(desc[10 * i:10 * i + 10]) for i in range(n)] == want_desc
    assert bytes(out_bytes[:len(want_bytes)]) == want_bytes
    assert bytes(out_states[:203 * len(want_states)]) == b"".join(want_states)
    assert len(want_states) == 6  # (label one, 4) (label two, 2) (label one, 2) (S, 2) (label one, 1) (S, 1)
    assert list(roff) == [d[8] for d in want_desc]
    for i, (mins, m) in enumerate(py):
        row = [(x or 0) if mins else 0 for x in (mins or [None] * m)] + [0] * (m0 - m)
        pres = [int(mins is not None and x is not None) for x in (mins or [None] * m)] + [0] * (m0 - m)
        assert list(minvals[i * m0:(i + 1) * m0]) == row and list(minpres[i * m0:(i + 1) * m0]) == pres, i
    assert wiped.value == 1
    # the call's own rules: a uniform call refuses the first item of another m, a mixed one an item larger than the one before
    assert pack(3, 0, openings) == 0 and list(sizes)[:3] == [4, r0, r0]
    assert pack(4, 0, openings) == INVALID_ARGUMENT and msg.value == b"all items of one prove batch must share the aggregation factor"
    items[4].m = 4
    assert pack(n, 1, openings) == INVALID_ARGUMENT and msg.value == b"mixed prove batch: items must be sorted by aggregation factor"
    items[4].m = 2
    if openings:  # an item without commitments passes as an openings item only
        assert pack(n, 1, 0) == INVALID_ARGUMENT and msg.value == b"null witness / statement field"


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
