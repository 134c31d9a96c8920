"""CPU suite for the joint final check and the sliced MSM prelude: the new entry points are declared, exported and bound on every
side of the ABI, they answer without a device the way their siblings do, and the MSM plan's host-side rules (csrc/recode.h, compiled
into the host test library with plain g++) hold: every plan the window rule can produce fits a workgroup's LDS in both prelude
forms, a plan that cannot is refused, and the rule itself gives what it gave before it moved into the shared header."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["bpp_verify_joint_stats", "bpp_batcher_verify_joint_stats"]
LDS_LIMIT = 160 * 1024  # what a gfx950 workgroup may hold


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("bulletproofs-plus_amd")


@pytest.fixture(scope="module")
def ht(pkg):
    lib = ctypes.CDLL(pkg._build.build_hosttest())
    for name in ("ht_msm_choose_window", "ht_msm_prelude_min_lds", "ht_msm_prelude_slices", "ht_msm_window_sweep"):
        getattr(lib, name).restype = ctypes.c_uint32
    lib.ht_msm_prelude_fits.restype = ctypes.c_int
    return lib


def test_new_symbols_on_every_side_of_the_abi(pkg):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bpp.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(bpp_[a-z0-9_]+)\s*\(", hdr)))
    ffi = open(os.path.join(ROOT, "rust", "bpp-gpu-shim", "src", "ffi.rs")).read()
    rust = sorted(set(re.findall(r"pub fn (bpp_[a-z0-9_]+)\s*\(", ffi)))
    assert rust == declared == sorted(n for n, _, _ in pkg._lib.SYMBOLS)
    pkg._build.build()
    lib = pkg._lib.load()
    for n in NEW:
        assert n in declared and hasattr(lib, n), n
    assert "struct bpp_verify_joint_stats" in hdr and "pub struct bpp_verify_joint_stats" in ffi
    assert re.search(r"#define BPP_TRACE_JOINT_RESULT 8\b", hdr)
    assert [n for n, _ in pkg._lib.VerifyJointStats._fields_] == ["calls", "accepted", "fallbacks", "fallback_all_ok"]
    assert ctypes.sizeof(pkg._lib.VerifyJointStats) == 32
    hpp = open(os.path.join(ROOT, "include", "bpp.hpp")).read()
    assert "verify_joint_stats()" in hpp and '"verify_joint"' in hpp


def test_stats_without_a_context_answer_like_their_siblings(pkg):
    """no device, no context: the joint counters refuse a null handle with the code the recheck's counters give"""
    lib = pkg._lib.load()
    j, c = pkg._lib.VerifyJointStats(), pkg._lib.VerifyCheckStats()
    assert lib.bpp_verify_joint_stats(None, ctypes.byref(j)) == lib.bpp_verify_check_stats(None, ctypes.byref(c)) < 0
    assert lib.bpp_batcher_verify_joint_stats(None, ctypes.byref(j)) == lib.bpp_batcher_verify_check_stats(None, ctypes.byref(c)) < 0
    import torch
    if not torch.cuda.is_available():  # and the context itself cannot be made: BPP_ERR_NO_DEVICE, there is no CPU fall-back
        ctx = ctypes.c_void_p()
        assert lib.bpp_ctx_create(ctypes.byref(ctx), 0) == -2


def _choose_window_before(n, all_terms):
    """the engine's rule as it stood in engine.hip before it moved to recode.h (default options), over arrays of group sizes"""
    thresholds = np.array([(1 << c) * 12 for c in range(4, 14)], dtype=np.int64)  # c goes up by one at each, from 4 to 14
    c = 4 + np.searchsorted(thresholds, n, side="right")
    c = np.minimum(c, np.where(n < 200000, 11, 14))
    return np.where(all_terms <= 20000, np.clip(c + 3, 4, 11), c)


def test_every_plan_of_the_window_rule_fits_in_both_forms(ht):
    """every group size from 1 to 2 000 000 terms, as a call of its own, as one of 64 such groups and as a small group of a large
    call: the width is what the rule gave before it moved, and its plan fits a workgroup in both prelude forms at 256 and 1024 lanes
    (the sweep itself runs in the host test library: six million ctypes calls would take a minute)"""
    lo, hi = 1, 2_000_000
    n = np.arange(lo, hi + 1, dtype=np.int64)
    seen = set()
    for mode, all_terms in ((0, n), (1, 64 * n), (2, np.maximum(n, 30000))):
        got = np.zeros(hi - lo + 1, dtype=np.uint8)
        assert ht.ht_msm_window_sweep(lo, hi, mode, got.ctypes.data_as(ctypes.c_void_p)) == 0, mode
        want = _choose_window_before(n, all_terms)
        diff = np.flatnonzero(got != want)
        assert diff.size == 0, (mode, int(n[diff[0]]), int(got[diff[0]]), int(want[diff[0]]))
        seen |= set(int(c) for c in np.unique(got))
    for c in seen:
        for threads in (256, 1024):
            for form in (0, 1):
                assert ht.ht_msm_prelude_fits(1 << (c - 1), threads, form) == 1, (c, threads, form)
                assert ht.ht_msm_prelude_min_lds(1 << (c - 1), threads, form) <= LDS_LIMIT
    assert seen == set(range(4, 12)) | {14}, seen  # (12 and 13 bits are forced widths: msm_c_max)
    # the table next to msm_prelude_fits, at the widths the rule produces for large groups
    assert ht.ht_msm_prelude_min_lds(4096, 1024, 0) == 39936 and ht.ht_msm_prelude_min_lds(4096, 256, 0) == 36864
    assert ht.ht_msm_prelude_min_lds(8192, 1024, 0) == 72704 and ht.ht_msm_prelude_min_lds(8192, 256, 0) == 69632
    assert ht.ht_msm_prelude_min_lds(8192, 256, 1) == 32768 and ht.ht_msm_prelude_min_lds(4096, 256, 1) == 16384
    assert ht.ht_msm_prelude_min_lds(512, 256, 1) == 7168  # the scan kernel's static arrays outweigh a small table


def test_plans_that_do_not_fit_are_refused(ht):
    for nb, threads, form in [(1 << 15, 1024, 0), (1 << 15, 256, 0), (1 << 16, 1024, 0), (1 << 16, 256, 1), (1 << 20, 256, 1), (0, 256, 0), (1 << 21, 256, 1)]:
        assert ht.ht_msm_prelude_fits(nb, threads, form) == 0, (nb, threads, form)
    assert ht.ht_msm_prelude_min_lds(1 << 15, 1024, 0) == 269312 > LDS_LIMIT
    assert ht.ht_msm_prelude_fits(1 << 15, 256, 1) == 1  # 128 KB: the sliced form holds one table where the other holds two


def test_slicing_rule(ht):
    S = ht.ht_msm_prelude_slices
    # every existing shape (the largest group any test or bench leg sends has 119 809 terms) keeps the one-workgroup form
    for n in (1, 300, 4226, 16514, 61570, 119809, 199999):
        for G in (1, 16, 64, 256):
            for c in (7, 11, 13, 14):
                assert S(n, G, -(-253 // c), 1 << (c - 1), 1024, 0) == 0, (n, G, c)
                assert S(n, G, -(-253 // c), 1 << (c - 1), 1024, -1) == 0
    # by rule: one joint group of 64 x 1024 proofs (130 + 16 x 65 536 terms, 14-bit windows, 19 of them)
    assert S(1_048_706, 1, 19, 8192, 1024, 0) == 34
    assert S(200_000, 1, 19, 8192, 1024, 0) == 34 and S(200_000, 64, 19, 8192, 1024, 0) == 2
    assert S(200_000, 1, 23, 1024, 1024, 0) == 28 and S(2_000_000, 8, 19, 8192, 1024, 0) == 5
    assert S(1_048_706, 1, 19, 8192, 1024, 1) == 0  # 1: the one-workgroup form whatever the size (A/B timing)
    # forced: S slices whatever the size, 64 at most
    for s in (2, 3, 7, 64):
        assert S(1, 1, 37, 64, 1024, s) == s and S(1_048_706, 3, 19, 8192, 1024, s) == s
    assert S(300, 1, 37, 64, 1024, 1000) == 64
