#!/usr/bin/env python3
"""Where a checked configs[4] call's extra time goes ("prove_check" = 1): the verifier's item-form upload of 1024 proofs (host
parse, staging, commitment decompression) against the resident verification as ONE reference batch -- the two steps the self-check
runs after the prover -- one call at a time on one context, median of 20 after 4 warm-up calls.  One JSON line."""
import ctypes
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import bench  # noqa: E402

bpp = importlib.import_module("bulletproofs-plus_amd")
packed = importlib.import_module("bulletproofs-plus_amd.packed")


def main():
    eng = bpp.Engine(0)
    p = bpp.RangeParameters.init(64, 4, bpp.create_pedersen_gens_with_extension_degree(3), engine=eng)
    d = bench.make_inputs(np, packed, p, 1024, seed=8675309 + 5)
    pr, cm, mv = (np.ascontiguousarray(d[k]) for k in ("proofs", "commitments", "min_values"))
    mp = np.ascontiguousarray(d["min_present"]).astype(np.uint8)
    n, plen = pr.shape
    lab = ctypes.create_string_buffer(bench.LABEL, len(bench.LABEL))
    items = (bpp._lib.VerifyItem * n)()  # the item form, as the self-check builds it: pointers into the proofs and statements
    for i in range(n):
        it = items[i]
        it.proof, it.proof_len = pr.ctypes.data + i * plen, plen
        it.commitments32, it.m = cm.ctypes.data + i * 4 * 32, 4
        it.min_values, it.min_present = mv.ctypes.data + i * 4 * 8, mp.ctypes.data + i * 4
        it.transcript_label, it.label_len = ctypes.cast(lab, ctypes.c_void_p), len(bench.LABEL)
    err = ctypes.create_string_buffer(256)
    up, ver = [], []
    for k in range(24):
        h = ctypes.c_uint64()
        t0 = time.perf_counter()
        assert eng.lib.bpp_batch_upload(eng.ctx, p.handle, items, n, ctypes.byref(h), err, 256) == 0, err.value
        t1 = time.perf_counter()
        assert eng.lib.bpp_verify_resident(eng.ctx, h.value, 0, 0, None, None, err, 256) == 0, err.value
        t2 = time.perf_counter()
        eng.lib.bpp_batch_destroy(eng.ctx, h.value)  # (its buffers serve the next upload, as the check's do)
        if k >= 4:
            up.append(t1 - t0)
            ver.append(t2 - t1)
    print(json.dumps({"metric": "checking batch of configs[4] (1024 x m4, t3) on one context, one call at a time",
                      "upload_ms_median": 1e3 * float(np.median(up)), "verify_ms_median": 1e3 * float(np.median(ver)),
                      "upload_ms_min": 1e3 * min(up), "verify_ms_min": 1e3 * min(ver), "calls": len(up)}))
    p.close()
    eng.close()


if __name__ == "__main__":
    main()
