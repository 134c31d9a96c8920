"""CPU suite: the constant-time multiscalar multiplication of seam B1 (bpp_msm_ct) as far as it goes without a device -- the one-lane
model that defines the kernels' result (csrc/ct.h: ct_straus_model, host-compiled with its table reads recorded), the chunk planner
(csrc/ct_plan.h) and the branch-free canonicity check, through libbpp_hosttest.so; then the same model and planner in a stand-alone
program under AddressSanitizer + UBSan (csrc/hosttest_ct.cpp), run as a child process."""
import ctypes
import hashlib
import importlib
import os
import subprocess

import pytest

from oracle.pyref import curve as C

L = C.L
COUNTS = (1, 2, 3, 16, 17, 33)
GROUP_SIZES = [0, 1, 16, 17, 0, 32, 33, 65, 0]


def _r(tag, i, n=32):
    out = b""
    k = 0
    while len(out) < n:
        out += hashlib.sha256(tag + b"%d.%d" % (i, k)).digest()
        k += 1
    return out[:n]


def edge_scalars(tag):
    """0, 1, l - 1, 2^252, 2^252 - 1, every digit 8 (the longest carry chain of the recoding), every digit 7, a random one"""
    return [0, 1, L - 1, 2**252, 2**252 - 1, int("8" * 63, 16), int("7" * 63, 16), int.from_bytes(_r(tag, 0), "little") % L]


def terms(n, tag):
    """n terms: the edge scalars in turn; random points with the identity encoding and a repeated point mixed in"""
    edge = edge_scalars(tag)
    scalars = [edge[i % 8] if i % 8 != 7 else int.from_bytes(_r(tag + b"s", i), "little") % L for i in range(n)]
    points = []
    for i in range(n):
        if i % 5 == 3:
            points.append(C.Point.identity())
        elif i % 5 == 4:
            points.append(points[i - 2])
        else:
            points.append(C.from_uniform_bytes(_r(tag + b"p", i, 64)))
    return scalars, points


@pytest.fixture(scope="module")
def ht():
    pkg = importlib.import_module("bulletproofs-plus_amd")
    lib = ctypes.CDLL(pkg._build.build_hosttest())
    lib.ht_ct_straus.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_size_t,
                                 ctypes.POINTER(ctypes.c_size_t)]
    lib.ht_ct_chunk_plan.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t,
                                     ctypes.POINTER(ctypes.c_size_t), ctypes.c_void_p]
    return lib


def straus(ht, scalars, points, want_trace=False):
    n = len(scalars)
    out = ctypes.create_string_buffer(32)
    cap = 64 * 4 * 8 * n + 16
    tr, tl = ctypes.create_string_buffer(cap), ctypes.c_size_t()
    sb = b"".join(s.to_bytes(32, "little") for s in scalars)
    pb = b"".join(p.compress() for p in points)
    assert ht.ht_ct_straus(sb, pb, n, out, tr, cap, ctypes.byref(tl)) == 1
    return (out.raw, tr.raw[:tl.value]) if want_trace else out.raw


@pytest.mark.parametrize("n", COUNTS)
def test_model_equals_the_oracle(ht, n):
    scalars, points = terms(n, b"m%d" % n)
    assert straus(ht, scalars, points) == C.multiscalar_mul(scalars, points).compress()
    if n >= 2:  # P and -P under equal scalars: the neutral element, 32 zero bytes
        p = points[0]
        for k in edge_scalars(b"pm")[1:]:
            assert straus(ht, [k, k], [p, -p]) == bytes(32)


def test_model_every_edge_scalar_on_one_term(ht):
    p = C.from_uniform_bytes(_r(b"one", 0, 64))
    for k in edge_scalars(b"one"):
        assert straus(ht, [k], [p]) == (p * k).compress(), hex(k)
        assert straus(ht, [k], [C.Point.identity()]) == bytes(32)


@pytest.mark.parametrize("n", COUNTS)
def test_table_reads_do_not_depend_on_the_scalars(ht, n):
    """the sequence of table entries read (BPP_CT_TOUCH) is the same for all-zero, all-(l - 1) and random scalars: 64 digit positions x
    n terms x four coordinates x all eight entries, in order"""
    _, points = terms(n, b"t%d" % n)
    vectors = [[0] * n, [L - 1] * n, [int.from_bytes(_r(b"tr", i), "little") % L for i in range(n)]]
    traces = {straus(ht, v, points, want_trace=True)[1] for v in vectors}
    assert traces == {bytes(range(8)) * (64 * n * 4)}, "a table read depends on a scalar"


def test_trace_changes_with_n_only(ht):
    lengths = set()
    for n in COUNTS:
        _, points = terms(n, b"l%d" % n)
        lengths.add(len(straus(ht, [1] * n, points, want_trace=True)[1]))
    assert lengths == {64 * 4 * 8 * n for n in COUNTS}


def plan(ht, off, n_terms, K):
    g = len(off) - 1
    go = (ctypes.c_uint32 * len(off))(*off)
    cap = n_terms + 1
    chunks, choff, nc = (ctypes.c_uint32 * (3 * cap))(), (ctypes.c_uint32 * (g + 1))(), ctypes.c_size_t()
    rc = ht.ht_ct_chunk_plan(go, g, n_terms, K, chunks, cap, ctypes.byref(nc), choff)
    if rc != 0:
        return rc, None, None
    return 0, [tuple(chunks[3 * c:3 * c + 3]) for c in range(nc.value)], list(choff)


@pytest.mark.parametrize("K", [1, 2])
def test_chunk_plan(ht, K):
    off = [0]
    for s in GROUP_SIZES:
        off.append(off[-1] + s)
    n = off[-1]
    rc, chunks, choff = plan(ht, off, n, K)
    assert rc == 0
    seen = [0] * n
    for c, (g, first, count) in enumerate(chunks):
        assert 1 <= count <= 16 * K                                   # no chunk exceeds 16 K terms, none is empty
        assert off[g] <= first and first + count <= off[g + 1]        # no chunk crosses a group
        assert choff[g] <= c < choff[g + 1]
        for i in range(first, first + count):
            seen[i] += 1
    assert seen == [1] * n                                            # every term lies in exactly one chunk
    for g, s in enumerate(GROUP_SIZES):
        assert choff[g + 1] - choff[g] == -(-s // (16 * K))           # empty groups make no chunk
    assert choff[-1] == len(chunks)
    assert chunks == sorted(chunks)                                   # group order, then term order: a function of the offsets alone
    # offsets that decrease, that end past the term count, that do not start at 0; a K that is no kernel form
    assert plan(ht, [0, 5, 3], 5, K)[0] == -1
    assert plan(ht, [0, 2, 6], 5, K)[0] == -1
    assert plan(ht, [1, 2], 5, K)[0] == -1
    assert plan(ht, [0, 2], 5, 3)[0] == -1 and plan(ht, [0, 2], 5, 0)[0] == -1


def test_form_rule_and_canonicity(ht):
    ht.ht_ct_form_rule.restype = ctypes.c_uint32
    ht.ht_ct_form_rule.argtypes = [ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int]
    sizes, chunk_counts = (0, 1, 2, 16, 17, 32, 33, 4096), (0, 1, 256, 1024, 1025, 1536, 2048, 10**6)
    for forced in (1, 2):
        assert {ht.ht_ct_form_rule(n, c, forced) for n in sizes for c in chunk_counts} == {forced}
    for auto in (0, -1):  # both mean the engine's rule: a function of public counts, monotone in each of them
        for c in chunk_counts:
            forms = [ht.ht_ct_form_rule(n, c, auto) for n in sizes]
            assert set(forms) <= {1, 2} and forms == sorted(forms)
        for n in sizes:
            forms = [ht.ht_ct_form_rule(n, c, auto) for c in chunk_counts]
            assert forms == sorted(forms)
            if n <= 16:
                assert set(forms) == {1}  # the commitment shape, whatever the number of outputs
    for v in [0, 1, L - 1, L, L + 1, 2**252, 2**253, 2**256 - 1, 2**255 - 19] + edge_scalars(b"c"):
        assert ht.ht_ct_sc_canonical(v.to_bytes(32, "little")) == (1 if v < L else 0), hex(v)


def test_model_and_planner_under_sanitizers():
    """csrc/hosttest_ct.cpp: a program of its own under ASan + UBSan, over the term counts and the group sizes above"""
    pkg = importlib.import_module("bulletproofs-plus_amd")
    exe = pkg._build.build_ct_harness()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.split("\n")
    for case in ["model_%d" % n for n in COUNTS] + ["plan_k1", "plan_k2", "canonical"]:
        assert "ok " + case in lines, (case, r.stdout[-2000:])
    assert "all ok" in lines
    assert r.stderr.strip() == "", r.stderr[-4000:]  # a sanitizer that has something to say says it here
