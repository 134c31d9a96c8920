#!/usr/bin/env python3
"""RESULTS.md from the committed files under profiles/ -- the ONE place where measured figures are written down.
README.md, DESIGN.md, BASELINE.md and INTEGRATION.md describe mechanisms and point here instead of re-quoting numbers.

    python tools/results_table.py r03_v2 > RESULTS.md

reads (each optional) profiles/<TAG>_bench_full.json (a complete `python bench.py --full` line), _bench_steps20.json (the driver's
form: --steps 20 --warmup 5), _bench_torchrun1.json (one rank under torch.distributed.run: the RCCL legs),
_kernel_stats_cfg2_default.csv and _pmc_sq_summary.csv (tools/profile_round.sh), _wave_probe.jsonl (tools/wave_probe.py),
_chunk_probe.jsonl (tools/chunk_probe.py)."""
import csv
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = os.path.join(ROOT, "profiles")


def load(tag, name):
    f = os.path.join(P, "%s_%s" % (tag, name))
    if not os.path.exists(f):
        return None, None
    if f.endswith(".jsonl"):
        return [json.loads(x) for x in open(f) if x.strip().startswith("{")], os.path.relpath(f, ROOT)
    if f.endswith(".json"):
        txt = [x for x in open(f).read().splitlines() if x.strip().startswith("{")]
        return json.loads(txt[-1]), os.path.relpath(f, ROOT)
    return list(csv.DictReader(open(f))), os.path.relpath(f, ROOT)


def M(x):
    return "%.2f M" % (x / 1e6)


def prove_device_section():
    """profiles/prove_device.json (a list of runs of tools/bench_prove_device.py): per shape, every arm over the runs"""
    f = os.path.join(P, "prove_device.json")
    out = ["## Proving from openings in device memory against proving from host arrays (`bpp_prove_openings_device`, "
           "`tools/bench_prove_device.py`, `profiles/prove_device.json`)", ""]
    if not os.path.exists(f):
        return out + ["unmeasured", ""]
    runs = json.load(open(f))
    one = runs[0]
    out += ["One thread, one context, %d items per call at %d bits; `bpp_prove_openings` over host rows against `bpp_prove_openings_device` over "
            "the same rows resident in device memory (`csrc/prove_ingest.h`), and each followed by a mixed upload of what it wrote "
            "(`bpp_batch_upload_mixed` / `bpp_batch_upload_mixed_device` + `bpp_batch_destroy`); the arms alternate in one process after a "
            "warm-up, %d rounds of %d calls per run, median (lowest-highest round) over the runs.  Box: an MI355X, recorded by the tool as "
            "\"%s\".  A record: no rate is promised -- the prover is bound by its instruction rate, the copies this form removes are a "
            "small part of a call." % (one["items"], one["n_bits"], one["reps"], one["inner"], one["box"]), "",
            "| shape | arm | ms per call | proofs/s |", "|---|---|---|---|"]
    for shape in [r["shape"] for r in one["shapes"]]:
        rows = [r for run in runs for r in run["shapes"] if r["shape"] == shape]
        for arm in rows[0]["arms"]:
            ms = [r["arms"][arm]["ms_per_call"] for r in rows]
            lo, hi = min(r["arms"][arm]["ms_low"] for r in rows), max(r["arms"][arm]["ms_high"] for r in rows)
            med = statistics.median(ms)
            out.append("| %s (m = %d, t = %d%s) | %s | %.3f (%.3f-%.3f) | %.1f k |" % (shape, rows[0]["m"], rows[0]["t"], ", nonces" if rows[0]["nonces"] else "",
                                                                                    arm, med, lo, hi, one["items"] / med))
    return out + [""]


def prove_enqueue_section():
    """profiles/prove_enqueue.json (a list of runs of tools/bench_prove_enqueue.py): per shape, every arm over the runs of this tree's
    library; the runs of another library (BPP_LIB_PATH: the parent commit's, blocking arm only) in a table of their own"""
    f = os.path.join(P, "prove_enqueue.json")
    out = ["## Proving on the stream from a resident plan against the blocking call (`bpp_prove_enqueue`, `tools/bench_prove_enqueue.py`, "
           "`profiles/prove_enqueue.json`)", ""]
    if not os.path.exists(f):
        return out + ["unmeasured", ""]
    runs = json.load(open(f))
    solo = lambda r: list(r["shapes"][0]["arms"]) == ["blocking"]  # noqa: E731  (a run of the A/B: the blocking arm alone)
    mine = [r for r in runs if r["library"] == "this tree" and not solo(r)]
    ab_mine = [r for r in runs if r["library"] == "this tree" and solo(r)]
    other = [r for r in runs if r["library"] != "this tree"]
    one = (mine or runs)[0]
    out += ["One thread, one context on a caller's stream, %d items per step at %d bits; the arms alternate in one process after a warm-up, "
            "%d rounds of %d steps per run, median (lowest-highest round) over the runs; host ms in the calls: wall time until the step's calls "
            "had returned (a blocking arm: the whole step); thread CPU: the calling thread's CPU time over the whole step, the wait included "
            "(`bpp_enqueue_wait` is the runtime's spinning event wait, the blocking call naps through most of its own).  "
            "`enqueue`: plan.enqueue + ticket wait; `+verify`: the blocking prove, a mixed device upload and a resident verification "
            "against enqueue, refill under the prover's ok mask, `bpp_verify_enqueue` and one wait.  Box: recorded by the tool as \"%s\".  "
            "A record: the kernels are the same, so equal GPU time and less host time was the expectation, not a speed-up." %
            (one["items"], one["n_bits"], one["reps"], one["inner"], one["box"]), "",
            "| shape | arm | ms per step | proofs/s | host ms in the step's calls | thread CPU ms per step |", "|---|---|---|---|---|---|"]

    def table(group):
        lines = []
        for shape in [r["shape"] for r in group[0]["shapes"]]:
            rows = [r for run in group for r in run["shapes"] if r["shape"] == shape]
            for arm in rows[0]["arms"]:
                have = [r["arms"][arm] for r in rows if arm in r["arms"]]
                med = statistics.median(a["ms_per_step"] for a in have)
                lines.append("| %s (m = %d, t = %d%s) | %s | %.3f (%.3f-%.3f) | %.1f k | %.3f | %.3f |" %
                             (shape, rows[0]["m"], rows[0]["t"], ", nonces" if rows[0]["nonces"] else "", arm, med, min(a["ms_low"] for a in have),
                              max(a["ms_high"] for a in have), group[0]["items"] / med, statistics.median(a["host_ms_in_calls"] for a in have),
                              statistics.median(a["host_cpu_ms_per_step"] for a in have)))
        return lines

    if mine:
        out += table(mine)
        med = lambda shape, arm: statistics.median(r["arms"][arm]["ms_per_step"] for run in mine for r in run["shapes"]  # noqa: E731
                                                   if r["shape"] == shape and arm in r["arms"])
        shapes = [r["shape"] for r in mine[0]["shapes"] if all(a in r["arms"] for a in ("blocking", "enqueue", "blocking+verify", "enqueue+verify"))]
        if shapes:
            out += ["", "What the verification adds to each prove arm, from the medians above: " +
                    "; ".join("%s: %.3f ms behind the blocking prove (upload + `bpp_verify_resident`), %.3f ms behind the enqueued one (refill + "
                              "`bpp_verify_enqueue`)" % (s, med(s, "blocking+verify") - med(s, "blocking"), med(s, "enqueue+verify") - med(s, "enqueue"))
                              for s in shapes) +
                    ".  The `enqueue+verify` step is SLOWER than `blocking+verify`, and the prove arms say where: not in the fork and join (the "
                    "enqueued prove alone is no slower than the blocking one) but in the verifier's own two forms -- one enqueued verification of "
                    "1024 proofs is a latency chain of about 3 ms whichever prover fed it (the refill section above: 3.1 ms per step for a refill "
                    "and `bpp_verify_enqueue` of 1024 proofs from one thread), the blocking upload and resident verification of the same batch the "
                    "smaller figure.  What the enqueue form buys is the calling thread: a third of a millisecond in its calls per step.  No kernel "
                    "timeline of the step was taken."]
        last =[r for r in mine[-1]["shapes"] if "stats_after" in r]
        if last:
            b, a = last[-1]["stats_before"], last[-1]["stats_after"]
            out += ["", "Counters over the timed steps of the last run's last shape: `bpp_prove_enqueue_stats` calls %d -> %d, first_calls %d -> %d, "
                    "host_waits %d -> %d, allocations %d -> %d; refill host_waits %d -> %d; `bpp_enqueue_stats` host_waits %d -> %d." %
                    (b["prove_enqueue"]["calls"], a["prove_enqueue"]["calls"], b["prove_enqueue"]["first_calls"], a["prove_enqueue"]["first_calls"],
                     b["prove_enqueue"]["host_waits"], a["prove_enqueue"]["host_waits"], b["prove_enqueue"]["allocations"],
                     a["prove_enqueue"]["allocations"], b["refill"]["host_waits"], a["refill"]["host_waits"], b["enqueue"]["host_waits"],
                     a["enqueue"]["host_waits"])]
    if other:
        out += ["", "The blocking call of this tree against the parent commit's library (`tools/gpu_ab.py --leg cmd`, the builds alternating on one "
                "box, a process per run with the blocking arm alone; the parent's rows are runs with `BPP_LIB_PATH` set):", "", "| shape | arm | ms per step | proofs/s | host ms in the step's calls | "
                "thread CPU ms per step |", "|---|---|---|---|---|---|"]
        out += [x.replace("| blocking |", "| blocking, this tree |") for x in (table(ab_mine) if ab_mine else [])]
        out += [x.replace("| blocking |", "| blocking, parent commit |") for x in table(other)]
    return out + [""]


def refill_mixed_section():
    """profiles/refill_mixed.json (a list of runs of tools/bench_refill_mixed.py): per batch size, both arms over every repetition of
    every run"""
    fmx = os.path.join(P, "refill_mixed.json")
    out = ["## A step of mixed aggregation factors: a fresh mixed upload per step against a refill (`bpp_batch_refill_enqueue_mixed`, "
           "`tools/bench_refill_mixed.py`, `profiles/refill_mixed.json`)", ""]
    if not os.path.exists(fmx):
        return out + ["unmeasured", ""]
    runs = json.load(open(fmx))
    sizes = sorted({r["items"] for r in runs})
    one = runs[0]
    out += ["One thread, one context, a ring of %d device input sets of one shape vector (m in the pattern %s, %d bits, t = %d, promises, no "
            "nonces), one verification enqueued per step: `bpp_batch_upload_mixed_device` + `bpp_verify_enqueue` + `bpp_batch_destroy` per step "
            "against `bpp_batch_refill_enqueue_mixed` (no `proof_lens` / `m`, no count, no mask) + `bpp_verify_enqueue` on one batch "
            "(`csrc/refill.h`); the arms alternate in one process, the sizes alternate through `tools/gpu_ab.py`; median (lowest-highest) "
            "over the repetitions of %d steps of every run.  The expectation was that the refill arm is not slower.  Box: an MI355X, recorded by the tool as \"%s\".  A record: no ratio "
            "is promised." % (one["ring"], ", ".join(str(m) for m in one["pattern"]), one["n_bits"], one["t"], one["steps"], one["box"]), "",
            "| slots per step | runs x repetitions | upload arm, ms per step | refill arm, ms per step | upload arm, steps/s | refill arm, steps/s | "
            "host ms in the step's calls, upload / refill | refill arm: host waits (refill, enqueue), layouts planned |", "|---|---|---|---|---|---|---|---|"]
    for n in sizes:
        mine = [r for r in runs if r["items"] == n]
        rows = [x for r in mine for x in r["rows"]]
        val = lambda arm, k: [x[k] for x in rows if x["arm"] == arm]  # noqa: E731
        cell = lambda arm, k, f: (f + " (" + f + "-" + f + ")") % (statistics.median(val(arm, k)), min(val(arm, k)), max(val(arm, k)))  # noqa: E731
        st = {k: sum(r["refill_arm"][k] for r in mine) for k in ("refill_host_waits", "enqueue_host_waits", "layouts_in_call")}
        out.append("| %d | %d x %d | %s | %s | %.1f | %.1f | %.3f / %.3f | %d, %d; %d |" %
                   (n, len(mine), mine[0]["reps"], cell("upload", "ms_per_step", "%.4f"), cell("refill", "ms_per_step", "%.4f"),
                    statistics.median(val("upload", "steps_per_s")), statistics.median(val("refill", "steps_per_s")),
                    statistics.median(val("upload", "host_ms_per_step_median")), statistics.median(val("refill", "host_ms_per_step_median")),
                    st["refill_host_waits"], st["enqueue_host_waits"], st["layouts_in_call"]))
    return out + [""]


def item_transcripts_section():
    """profiles/item_transcripts.json: the step with per-item transcripts against the existing step (tools/bench_item_transcripts.py),
    the two kernels alone, and the callers that do not use the feature against the parent commit's library (tools/gpu_ab.py)"""
    fit = os.path.join(P, "item_transcripts.json")
    out = ["## Per-item transcripts on the stream: refill with transcripts + `bpp_verify_enqueue_states` against refill + `bpp_verify_enqueue` "
           "(`tools/bench_item_transcripts.py`, `profiles/item_transcripts.json`)", ""]
    if not os.path.exists(fit):
        return out + ["unmeasured", ""]
    doc = json.load(open(fit))
    step = doc["step"]
    summary = [r for r in step if r.get("tool") == "bench_item_transcripts"][-1]
    arm = lambda a, k: [r[k] for r in step if r.get("arm") == a]  # noqa: E731
    cell = lambda v, f: (f + " (" + f + "-" + f + ")") % (statistics.median(v), min(v), max(v))  # noqa: E731
    out += ["One thread, one context, %d slots of 64 bits, m = 1, t = 1, a ring of 4 device input sets, both arms on one tree alternating in one "
            "process, %d repetitions of %d steps; median (lowest-highest).  The transcripts arm brings 203 bytes per proof in (`k_item_states`), "
            "runs PASS 1 in its STATES form and writes 203 bytes per proof out (`k_states_out`).  Nothing was promised; the expectation was a "
            "few microseconds per kernel and a PASS 1 within a per cent of the default form.  Box: recorded by the tool as \"%s\"." %
            (summary["items"], summary["reps"], summary["steps"], summary["box"]), "",
            "| arm | ms per step | steps/s | host ms in the step's calls | host waits (refill, enqueue), layouts planned |", "|---|---|---|---|---|"]
    st = summary["steady_state"]
    for a in ("plain", "transcripts"):
        out.append("| %s | %s | %.1f | %.3f | %s |" % (a, cell(arm(a, "ms_per_step"), "%.4f"), statistics.median(arm(a, "steps_per_s")),
                                                        statistics.median(arm(a, "host_ms_per_step_median")),
                                                        "%d, %d; %d (both arms)" % (st["refill_host_waits"], st["enqueue_host_waits"], st["layouts_in_call"])))
    out += ["", "Difference of the medians: %.4f ms per step (%.2f %%)." %
            (summary["difference_ms_per_step"], 100 * summary["difference_ms_per_step"] / summary["plain_ms_per_step"]), "",
            "| kernel (rocprofv3 kernel trace of a 40-step run) | calls | average us | lowest-highest us |", "|---|---|---|---|"]
    for r in step:
        if "kernel" in r:
            out.append("| `%s` | %d | %.2f | %.2f-%.2f |" % (r["kernel"].replace("void bpp::", "").replace("bpp::", ""), r["calls"], r["avg_us"], r["min_us"], r["max_us"]))
    ab = doc.get("callers_without_the_feature")
    if ab:
        out += ["", "Callers that do not use the feature, this tree against the parent commit's library, alternating (`tools/gpu_ab.py`); "
                "median (lowest-highest) over every repetition of every run:", "",
                "| program, arm | this tree | parent commit |", "|---|---|---|"]
        runs = ab["bench_refill"]["runs"]
        for name in ("refill", "refill_count_512", "refill_live_0.5", "upload"):
            vals = {b: [v for r in runs if r["build"] == b for v in r["steps_per_s"].get(name, [])] for b in ("this", "parent")}
            out.append("| `tools/bench_refill.py` %s, steps/s | %s | %s |" % (name, cell(vals["this"], "%.1f"), cell(vals["parent"], "%.1f")))
        hl = ab["bench_py"]["runs"]
        for s in sorted({r["session"] for r in hl}):
            vals = {b: [r["M_proofs_per_s"] for r in hl if r["build"] == b and r["session"] == s] for b in ("this", "parent")}
            clk = {b: [r["clock_GHz"] for r in hl if r["build"] == b and r["session"] == s] for b in ("this", "parent")}
            out.append("| `bench.py`, M proofs/s, session %d (%d runs each; clocks %.2f-%.2f / %.2f-%.2f GHz) | %s | %s |" %
                       (s, len(vals["this"]), min(clk["this"]), max(clk["this"]), min(clk["parent"]), max(clk["parent"]),
                        cell(vals["this"], "%.2f"), cell(vals["parent"], "%.2f")))
    return out + [""]


def transcript_ops_section():
    """profiles/transcript_ops.json (tools/bench_transcript_ops.py): bpp_transcripts_enqueue against the host route, the call alone and
    inside the full step; "bench_ab": bench.py's headline on this tree and on the parent commit's library, alternating (tools/gpu_ab.py)"""
    f = os.path.join(P, "transcript_ops.json")
    out = ["## Merlin on the stream: `bpp_transcripts_enqueue` against the host route (`tools/bench_transcript_ops.py`, "
           "`profiles/transcript_ops.json`)", ""]
    if not os.path.exists(f):
        return out + ["unmeasured", ""]
    doc = json.load(open(f))
    out += ["One thread, an engine on torch's stream.  make = NEW + APPEND(32 bytes per row); challenge = CHALLENGE(32).  Device: calls back to "
            "back for a window of %.1f s around one stream synchronise.  Host route: rows (or ids) copied down, the three host helpers per row, the "
            "result copied up -- called from Python through ctypes; the last columns take the measured cost of as many empty ctypes calls off.  "
            "Nothing was promised.  Box: \"%s\"." % (doc["window_s"], doc["box"]), "",
            "| rows | arm | device ms per call | device M rows/s | host route ms per step (lowest-highest) | host / device | less ctypes: host ms | host / device |",
            "|---|---|---|---|---|---|---|---|"]
    for r in doc["sizes"]:
        for k, a in r["arms"].items():
            out.append("| %d | %s | %.4f | %.1f | %.3f (%.3f-%.3f) | %.1f | %.3f | %.1f |" %
                       (r["n"], k, a["device_ms_per_call"], a["device_rows_per_s"] / 1e6, a["host_ms_per_step"], a["host_ms_low"], a["host_ms_high"],
                        a["host_over_device"], a["host_ms_less_ctypes"], a["host_less_ctypes_over_device"]))
    fs = doc.get("full_step")
    if fs:
        out += ["", "The full step (make the rows -> `bpp_prove_enqueue` -> refill -> `bpp_verify_enqueue_states` -> challenge on the rows handed back) at "
                "%d proofs of %d bits, m = %d, t = %d, the arms alternating, %d rounds of %d steps; median of the rounds' medians (lowest-highest round):" %
                (fs["items"], fs["n_bits"], fs["m"], fs["t"], fs["reps"], fs["inner"]), "",
                "| arm | ms per step | proofs/s |", "|---|---|---|"]
        for k, a in fs["arms"].items():
            out.append("| %s | %.3f (%.3f-%.3f) | %.0f |" % (k, a["ms_per_step"], a["ms_low"], a["ms_high"], a["proofs_per_s"]))
        st = fs["stats"]
        out += ["", "host / device: %.3f.  Host waits inside the calls over the whole run: transcripts %d (of %d calls), prove enqueue %d, refill %d, "
                "verify enqueue %d." % (fs["host_over_device"], st["transcripts"]["host_waits"], st["transcripts"]["calls"],
                                        st["prove_enqueue"]["host_waits"], st["refill"]["host_waits"], st["enqueue"]["host_waits"])]
    ab = doc.get("bench_ab")
    if ab:
        cell = lambda v: "%.2f (%.2f-%.2f)" % (statistics.median(v), min(v), max(v))  # noqa: E731
        out += ["", "`bench.py`'s headline, this tree against the parent commit's library, alternating in one call (`tools/gpu_ab.py --leg headline`, "
                "%s); M proofs/s, median (lowest-highest) of %d runs each:" % (ab["args"], len(ab["this"])), "",
                "| this tree | parent commit |", "|---|---|", "| %s | %s |" % (cell(ab["this"]), cell(ab["parent"]))]
    return out + [""]


def transcript_rng_section():
    """profiles/transcript_rng.json (tools/bench_transcript_rng.py): the transcript-RNG program of bpp_transcripts_enqueue against the
    host route; "existing_program_ab": the NEW + APPEND + CHALLENGE program on this tree and on the parent commit's library"""
    f = os.path.join(P, "transcript_rng.json")
    out = ["## The transcript RNG on the stream: `RNG_BEGIN .. RNG_SCALARS` against the host route (`tools/bench_transcript_rng.py`, "
           "`profiles/transcript_rng.json`)", ""]
    if not os.path.exists(f):
        return out + ["unmeasured", ""]
    doc = json.load(open(f))
    if doc.get("sizes"):
        out += ["One thread, an engine on torch's stream.  The program: RNG_BEGIN, RNG_REKEY(32 B), RNG_FINALIZE(32 B of entropy), RNG_FILL32 of %d bytes "
                "(a configs[4]-shaped rng row), RNG_SCALARS x %d.  Device: calls back to back for a window of %.1f s around one stream synchronise.  "
                "Host route: the host helpers per row on one core -- called from Python through ctypes; the last columns take the measured cost of as "
                "many empty ctypes calls off -- plus the copy to the device.  Nothing was promised.  Box: \"%s\"." %
                (doc["rng_row_bytes"], doc["scalars"], doc["window_s"], doc["box"]), "",
                "| rows | device ms per call | device M rows/s | host route ms per step (lowest-highest) | host / device | less ctypes: host ms | host / device |",
                "|---|---|---|---|---|---|---|"]
        for r in doc["sizes"]:
            out.append("| %d | %.4f | %.2f | %.1f (%.1f-%.1f) | %.0f | %.1f | %.0f |" %
                       (r["n"], r["device_ms_per_call"], r["device_rows_per_s"] / 1e6, r["host_ms_per_step"], r["host_ms_low"], r["host_ms_high"],
                        r["host_over_device"], r["host_ms_less_ctypes"], r["host_less_ctypes_over_device"]))
    ab = doc.get("existing_program_ab")
    if ab:
        out += ["", "The existing program (%s) on this tree against the parent commit's library, alternating in one call (`tools/gpu_ab.py --leg cmd`), "
                "%s; the parent stands twice in every repetition, and its own lowest-highest is the spread this tree is held to:" % (ab["program"], ab["unit"]),
                "", "| rows | parent: median (lowest-highest) | this tree: median (lowest-highest) | inside the parent's spread |", "|---|---|---|---|"]
        for size, a in ab["sizes"].items():
            out.append("| %s | %.4f (%.4f-%.4f) | %s | %s |" %
                       (size, a["parent_median"], a["parent_spread"][0], a["parent_spread"][1],
                        "%.4f (%.4f-%.4f)" % (a["this_median"], min(a["this"]), max(a["this"])) if a["this"] else "unmeasured",
                        "yes" if a["this_inside_parent_spread"] else "no"))
    return out + [""]


def rows_msm_section():
    """profiles/rows_msm.json (tools/bench_rows_msm.py): bpp_rows_msm_enqueue against the host-hop route through bpp_msm_ct_batched, the call
    alone and inside the commit / challenge / response step; "kernels": registers, scratch and LDS from the build"""
    f = os.path.join(P, "rows_msm.json")
    out = ["## Constant-time sums over device rows: `bpp_rows_msm_enqueue` against the host hop (`tools/bench_rows_msm.py`, "
           "`profiles/rows_msm.json`)", ""]
    if not os.path.exists(f):
        return out + ["unmeasured", ""]
    doc = json.load(open(f))
    out += ["One thread, an engine on torch's stream.  Device: calls back to back for a window of %.1f s around one stream synchronise.  Host hop: "
            "the parent commit's route for the same rows -- the scalars copied down, `bpp_msm_ct_batched` (`k_ct_straus<1>`, one workgroup per "
            "output; its own upload, wait and download), the outputs copied up.  The arms alternate, %d rounds; median (lowest-highest round).  "
            "Both routes gave the same bytes.  Nothing was promised.  Box: \"%s\"." % (doc["window_s"], doc["reps"], doc["box"]), "",
            "| rows | case | device ms per call | device us per output | host hop ms per step | host hop us per output | host hop / device |",
            "|---|---|---|---|---|---|---|"]
    for c in doc["cases"]:
        out.append("| %d | K = %d, %s | %.4f (%.4f-%.4f) | %.4f | %.3f (%.3f-%.3f) | %.4f | %.2f |" %
                   (c["n"], c["K"], "shared bases" if c["shared"] else "per-row points", c["device_ms_per_call"], c["device_ms_low"],
                    c["device_ms_high"], c["device_us_per_output"], c["host_hop_ms_per_step"], c["host_hop_ms_low"], c["host_hop_ms_high"],
                    c["host_hop_us_per_output"], c["host_hop_over_device"]))
    st = doc.get("step")
    if st:
        out += ["", "The commit / challenge / response step (transcript + `RNG_SCALARS` -> r; R = r G; `APPEND_POINT` X, R, `CHALLENGE_SCALAR` -> c; "
                "s = c x + r) at %d rows, the arms alternating, %d rounds of %d steps; median of the rounds' medians (lowest-highest round):" %
                (st["items"], st["reps"], st["inner"]), "", "| arm | ms per step | rows/s |", "|---|---|---|"]
        for k, a in st["arms"].items():
            out.append("| %s | %.3f (%.3f-%.3f) | %.0f |" % (k.replace("_", " "), a["ms_per_step"], a["ms_low"], a["ms_high"], a["rows_per_s"]))
        out += ["", "host hops / device: %.2f.  Host waits inside the calls over the whole run: rows %d (of %d calls, %d of them first calls), "
                "transcripts %d." % (st["host_hops_over_device"], st["stats"]["rows"]["host_waits"], st["stats"]["rows"]["calls"],
                                     st["stats"]["rows"]["first_calls"], st["stats"]["transcripts"]["host_waits"])]
    if doc.get("kernels"):
        out += ["", "| kernel (from the build) | VGPRs | SGPRs | scratch bytes | LDS bytes |", "|---|---|---|---|---|"]
        for k in doc["kernels"]:
            out.append("| `%s` | %d | %d | %d | %d |" % (k["kernel"], k["vgpr"], k["sgpr"], k["scratch"], k["lds"]))
    return out + [""]


def main():
    tag = sys.argv[1] if len(sys.argv) > 1 else "r03_v1"
    out = ["# RESULTS — measured figures (generated by `tools/results_table.py %s` from `profiles/`; do not edit)" % tag, "",
           "One MI355X (gfx950), ROCm 7.2, this repository's `bench.py`. Proofs are 64-bit Bulletproofs+ range proofs over "
           "ristretto255; every figure is bit-exact work (the GPU suite holds the same kernels to the oracle). "
           "Mechanisms: `DESIGN.md`; earlier rounds: `profiles/r01_*`, `profiles/r02_*`, `profiles/r03_*`, `HISTORY.md`.", ""]
    full, ffull = load(tag, "bench_full.json")
    s20, fs20 = load(tag, "bench_steps20.json")
    tr1, ftr1 = load(tag, "bench_torchrun1.json")
    rows = []
    if full:
        r = full.get("roofline", {})
        rows.append(("headline (`value`): BASELINE configs[1], 64 reference batches of 1024 proofs per step, inputs resident, "
                     "%d steps, %d in flight" % (full["steps"], full["config"]["steps_in_flight_per_gpu"]),
                     "**%s proofs/s**, %.3f ms per 65 536-proof step at %.2f GHz" % (M(full["value"]), full["ms_per_step"], full.get("shader_clock_ghz") or 0), ffull))
        if r:
            rows.append(("roofline kernel `k_msm_accumulate`: 64 B x %d terms per launch" % r["msm_terms_per_launch"],
                         "%.1f GB/s = %.4f of the 8 TB/s HBM peak in the timed region (%.3f ms per launch); alone %.3f ms = %.4f; "
                         "`v_mad_u64_u32` rate: %.3f of 39.3 T/s in the timed region, %.3f alone" %
                         (r["achieved"], r["frac"], r["kernel_ms"], r.get("alone", {}).get("kernel_ms", 0), r.get("alone", {}).get("frac", 0),
                          r["valu"]["frac"], r.get("alone", {}).get("valu_frac", 0)), ffull))
            if r.get("traffic"):
                rows.append(("its HBM-side traffic per launch (FETCH_SIZE / WRITE_SIZE passes of the run itself, calibrated)",
                             "%.0f MB = %.1f x the algorithmic %.1f MB" % (r["traffic"] / 1e6, r["traffic"] / r["algorithmic_bytes"], r["algorithmic_bytes"] / 1e6), ffull))
        d = full.get("roofline_decompress")
        if d:
            a = d.get("alone", {})
            rows.append(("`k_decompress` (the other dominant kernel): 32 B x %d points per launch" % d["points_per_launch"],
                         "%.3f ms in the timed region, mad rate %.3f of peak; alone: %.3f ms, %.0f VALU instructions per point, %.2f of wave cycles waiting"
                         % (d["kernel_ms"], d["valu"]["frac"], a.get("kernel_ms", 0), a.get("valu_instr_per_point", 0), a.get("wait_inst_frac", 0)), ffull))
        if full.get("stages_ms"):
            rows.append(("stage intervals per step, %d steps sharing the chip (ms)" % full["config"]["steps_in_flight_per_gpu"], ", ".join("%s %.2f" % (k[:-3], v) for k, v in full["stages_ms"].items() if v), ffull))
    if s20:
        rows.append(("the driver's form: `--steps 20 --warmup 5`", "%s proofs/s, %.3f ms per step" % (M(s20["value"]), s20["ms_per_step"]), fs20))
    ex = (full or {}).get("extra", {})
    h = ex.get("host_in")
    if h:
        rows.append(("host buffers in -> verdict out, 64 x 1024 proofs per call as ONE `bpp_packed_batch` (`pcie_inclusive_value`)",
                     "one context, pipelined (depth %d): **%s proofs/s**, %.1f GB/s of host bytes; four contexts: %s; one context, blocking call: %s"
                     % (h["one_context"]["pipeline_depth"], M(h["one_context"]["proofs_per_s"]), h["one_context"]["host_to_device_GBps"],
                        M(h["four_contexts"]["proofs_per_s"]), M(h["one_context_blocking"]["proofs_per_s"])), ffull))
    c3 = ex.get("cfg3")
    if c3:
        t = c3["roofline"].get("traffic")
        rows.append(("configs[2]: 256 x aggregation-8 batches, 64 per step (generator columns as an int8 matrix product over the proofs of a "
                     "batch on the matrix cores: `kernels_static_gemm.h`; per-proof products: 10.0-10.2 M, `profiles/r04_v2_bench_full.json`, "
                     "`profiles/r04_agg_probe.jsonl`)", "%s proofs/s, %.3f ms per step%s" %
                     (M(c3["proofs_per_s"]), c3["ms_per_step"], "; accumulate traffic %.0f MB per launch (%.1f x algorithmic)" % (t / 1e6, t / c3["roofline"]["algorithmic_bytes"]) if t else ""), ffull))
    a4 = (c3 or {}).get("agg4096")
    if a4 and "proofs_per_s" in a4:
        rows.append(("north_star's target shape: 4096 x aggregation-8 proofs as ONE reference batch per call (chunk = 0: a 119 809-term MSM; "
                     "`extra.cfg3.agg4096`; target: >= 100 k aggregated verifications/s)",
                     "**%s proofs/s** (%s committed values/s), %.2f ms per batch alone, %.2f ms with the other calls in flight"
                     % (M(a4["proofs_per_s"]), M(a4["values_per_s"]), a4["ms_per_batch_alone"], a4["ms_per_batch_in_flight"]), ffull))
    w = ex.get("wide4096")
    if w:
        rows.append(("one 4096-proof reference batch per call (chunk = 0), one GPU", "%s proofs/s with 12 calls in flight; %.2f ms per batch alone"
                     % (M(w["proofs_per_s"]), w["ms_per_batch_alone"]), ffull))
    la = ex.get("latency")
    if la:
        rows.append(("one `verify_batch` call at a time", ", ".join("%.3f ms for %s proof(s)" % (la[k]["ms_per_call_median"], k[6:]) for k in ("batch_1", "batch_64", "batch_256") if k in la), ffull))
    ro = ex.get("recover_only")
    if ro and "proofs_per_s" in ro:
        rows.append(("`VerifyAction::RecoverOnly` over the headline's 65 536 resident proofs (seed nonces resident), 1024-proof reference batches: PASS 1 + decompression + mask recovery, no weight chain, no MSM",
                     "**%s proofs/s**, %.3f ms per step; stage intervals (ms): %s; `k_decompress` %.1f GB/s of its 32 B per point = %.4f of the HBM peak, mad rate %.3f of 39.3 T/s; masks == the prover's blindings: %s" %
                     (M(ro["proofs_per_s"]), ro["ms_per_step"], ", ".join("%s %.2f" % (k[:-3], v) for k, v in ro["stages_ms"].items()), ro["roofline"]["achieved"], ro["roofline"]["frac"],
                      ro["roofline"]["valu"]["frac"], ro.get("masks_equal_blindings")), ffull))
    sc_ = ex.get("small_calls")
    if sc_ and "batcher" in sc_:
        rows.append(("32 separate callers, one 256-proof `verify_batch` call each at a time, host buffers in",
                     "a context per caller, admission gate at %s calls per device: **%.0f calls/s** = %s proofs/s (%d of the calls queued at the gate); gate off: %.0f calls/s; through ONE `bpp_batcher`: **%.0f calls/s = %s proofs/s** (%.2f ms per call, largest pool %s calls); `RecoverOnly` calls through the batcher (nonces in, masks out, checked): **%.0f calls/s = %s proofs/s**" %
                     (sc_.get("small_call_limit"), sc_["separate_contexts"]["calls_per_s"], M(sc_["separate_contexts"]["proofs_per_s"]), sc_["separate_contexts"].get("calls_that_queued_at_the_gate", 0),
                      sc_.get("separate_contexts_gate_off", {}).get("calls_per_s", 0), sc_["batcher"]["calls_per_s"], M(sc_["batcher"]["proofs_per_s"]), sc_["batcher"]["ms_per_call"],
                      sc_["batcher"].get("largest_pool", {}).get("calls"), sc_.get("batcher_recover_only", {}).get("calls_per_s", 0), M(sc_.get("batcher_recover_only", {}).get("proofs_per_s", 0))), ffull))
    pr = ex.get("prover")
    if pr:
        rr = pr["roofline"]
        rows.append(("configs[4]: `bpp_prove_batch`, 1024 x aggregation-4, extension degree 3", "%.0f k proofs/s one call at a time%s; the fixed-base MSM %.2f ms of summed event time per call (the two sub-batches' launches overlap), %.1f G additions/s over the call's %.2f ms, %s" %
                     (pr["proofs_per_s"] / 1e3, (", %.0f k with four calls in flight" % (pr["four_calls_in_flight"]["proofs_per_s"] / 1e3)) if pr.get("four_calls_in_flight") else "", rr["kernel_ms"],
                      rr.get("additions_per_s_call_wall", 0) / 1e9, rr.get("engine_call_ms", 0), ("traffic %.1f GB per call = %.0f x its algorithmic bytes" %
                      (rr["traffic"] / 1e9, rr["traffic"] / rr["algorithmic_bytes"])) if rr.get("traffic") else "traffic not measured"), ffull))
        c2 = pr.get("uniform_access_A1_B") or {}
        if c2.get("proofs_per_s"):
            rows.append(("the same with A1 and B in the uniform-access form as well (option `ct` = 2: the reference's constant-time `&P * Scalar`, "
                         "`src/range_proof.rs:572-584`; DESIGN 4.3)", "%.0f k proofs/s one call at a time (%.1f %% below the default, same run); proof bytes equal: %s"
                         % (c2["proofs_per_s"] / 1e3, 100 * c2.get("cost_against_default", 0), c2.get("bytes_equal_default")), ffull))
    oc = ex.get("other_chain")
    if oc and "proofs_per_s" in oc:
        rows.append(("the headline's step with the weight chains on the other side: `%s` (the headline ran `%s`), %d steps" %
                     (oc["weight_chains"], oc.get("headline_weight_chains"), oc["steps"]),
                     "%s proofs/s, %.3f ms per step, **%.2f host cores busy** (the headline: %.2f)" %
                     (M(oc["proofs_per_s"]), oc["ms_per_step"], oc["host_cores_busy"], full.get("host_cores_busy") or 0), ffull))
    pl, fpl = load(tag, "prover_leg.json")
    if pl:
        rows.append(("the same call from `tools/bench_prover_leg.py` (8 calls back to back, nothing else resident)", "%.0f k proofs/s, %.2f ms per call (%.2f ms inside the engine)" %
                     (pl["proofs_per_s"] / 1e3, pl["ms_per_call"], pl["engine_total_ms"]), fpl))
    cb = (full or {}).get("cpu_baseline")
    if cb:
        rows.append(("`oracle/c` (CPU port with dalek's algorithms) on the box's host", "%.1f k proofs/s on one core, %.0f k on %d cores" %
                     (cb["value"] / 1e3, cb["all_cores"]["value"] / 1e3, cb["all_cores"]["cores"]), ffull))
    wd = (tr1 or {}).get("extra", {}).get("wide")
    if wd:
        rows.append(("configs[3] through `bpp_verify_sharded_groups_wave` over RCCL, %d rank(s), %d calls in flight, each %d x %d batches resident as one" % (wd["rccl_ranks"], wd["waves"], wd.get("slots_per_call", 1), wd["batches_per_wave"]),
                     "%s proofs/s, %.3f ms per 4096-proof batch; the last call on the host (ms): %s" % (M(wd["proofs_per_s"]), wd["ms_per_batch"], ", ".join("%s %.2f" % (k[:-3], v) for k, v in (wd.get("last_wave_host_ms") or {}).items() if k.endswith("_ms"))), ftr1))
        rows.append(("headline under `torch.distributed.run`, 1 rank", "%s proofs/s" % M(tr1["value"]), ftr1))
    out += ["| what | value | source |", "|---|---|---|"] + ["| %s | %s | `%s` |" % r for r in rows] + [""]
    # ---- GPU and CPU side by side, per BASELINE config: every figure from the SAME run and the same inputs (bench.py's cpu_baseline objects)
    if full:
        def cpu(cbo):
            if not cbo or "value" not in cbo:
                return "-", "-"
            ac = cbo.get("all_cores")
            return "%.4g" % cbo["value"], ("%.4g on %d cores" % (ac["value"], ac["cores"])) if ac else "-"
        side = []
        la = ex.get("latency") or {}
        for k in ("batch_1", "batch_64", "batch_256"):
            if k in la:
                c1, _ = cpu(la[k].get("cpu_baseline"))
                side.append(("configs[0]'s shape: ONE verify call of %s proof(s) at a time" % k[6:], "%.4g (%.3f ms per call)" % (la[k]["proofs_per_s"], la[k]["ms_per_call_median"]),
                             "%s (%.3f ms per call)" % (c1, la[k].get("cpu_baseline", {}).get("ms_per_batch", 0)), "-"))
        c1, ca = cpu(full.get("cpu_baseline"))
        side.append(("configs[1] (headline): reference batches of 1024 x aggregation-1 (CPU: of 256, the reference's MAX_RANGE_PROOF_BATCH_SIZE)", "%.4g" % full["value"], c1, ca))
        for key, name in (("cfg3", "configs[2]: reference batches of 256 x aggregation-8"), ("wide4096", "one 4096-proof reference batch per call (configs[3]'s batch on one GPU)"),
                          ("recover_only", "VerifyAction::RecoverOnly, reference batches of 1024 (CPU: of 256)")):
            o = ex.get(key)
            if o and "proofs_per_s" in o:
                c1, ca = cpu(o.get("cpu_baseline"))
                side.append((name, "%.4g" % o["proofs_per_s"], c1, ca))
        a4 = (ex.get("cfg3") or {}).get("agg4096")
        if a4 and "proofs_per_s" in a4:
            c1, ca = cpu(a4.get("cpu_baseline"))
            side.append(("north_star's target shape: one reference batch of 4096 x aggregation-8", "%.4g" % a4["proofs_per_s"], c1, ca))
        pr_ = ex.get("prover")
        if pr_ and "proofs_per_s" in pr_:
            c1, ca = cpu(pr_.get("cpu_baseline"))
            eq = pr_.get("cpu_baseline", {}).get("bytes_equal_engine")
            side.append(("configs[4]: prover, 1024 x aggregation-4, extension degree 3 (the CPU port's proof bytes == the engine's: %s)" % eq, "%.4g" % pr_["proofs_per_s"], c1, ca))
        out += ["## GPU and CPU side by side, per BASELINE config (proofs/s; `%s`)" % ffull, "",
                "The CPU column is `oracle/c` -- the plain-C port of the reference's algorithms (precomputed Straus, Straus / Pippenger, generator folding "
                "in the prover), `kind: \"port\"` -- timed on the GPU box's host in the same `bench.py` run on the same inputs: one thread (the reference is "
                "single-threaded), and one reference batch per schedulable core side by side.  The Rust reference itself cannot be built here (no toolchain).", "",
                "| config | MI355X (this engine) | CPU port, 1 core | CPU port, all schedulable cores |", "|---|---|---|---|"]
        out += ["| %s | %s | %s | %s |" % r for r in side] + [""]
        if full.get("host_chain_cpu_ms_per_step") is not None:
            out += ["Host side of the headline step: %.2f ms of CPU time in the library's host pool per %.2f ms step (the batch weight chains), %.2f ms for the whole process: "
                    "**%.1f host cores busy per rank** (`host_threads` %s, `usable_cpus` %s, weight chains: %s, `host_bound`: %s) -- what N ranks on one node need N times over.  "
                    "By thread name: %s.  The driver's 20-step form of the same build: %s."
                    % (full["host_chain_cpu_ms_per_step"], full["ms_per_step"], full.get("host_process_cpu_ms_per_step", 0), full.get("host_cores_busy", 0),
                       full.get("host_threads"), full.get("usable_cpus"), full.get("weight_chains"), full.get("host_bound"),
                       ", ".join("%s %.2f (%d threads)" % (e["thread"], e["cores_busy"], e["threads"]) for e in full.get("host_cores_busy_by_thread") or []) or "n/a",
                       ("%.2f cores at %s proofs/s" % (s20.get("host_cores_busy") or 0, M(s20["value"]))) if s20 else "n/a"), ""]
    tp, ftp = load(tag, "bench_two_ranks_one_gpu.json")
    if tp:
        w2 = (tp.get("extra") or {}).get("wide") or {}
        out += ["## The multi-rank code as two PROCESSES on the one GPU (`%s`)" % ftp, "",
                "`python -m torch.distributed.run --nproc-per-node 2 bench.py --gpus 2 --one-device`: both ranks on device 0 (a rehearsal, not a scaling point), the sharded leg's "
                "all_gathers through the caller-supplied transport (`bpp_comm_create_callbacks`) over gloo.", "",
                "| what | value |", "|---|---|",
                "| headline, 2 ranks sharing the GPU | %s proofs/s, %.3f ms per step, all steps verified: %s |" % (M(tp["value"]), tp["ms_per_step"], tp.get("all_steps_verified")),
                "| `extra.wide` (configs[3]: one 4096-proof batch over the 2 ranks) | %s |" % (("%s proofs/s, %.3f ms per batch, transport: %s" % (M(w2["proofs_per_s"]), w2["ms_per_batch"], w2.get("transport"))) if "proofs_per_s" in w2 else w2.get("error")),
                "| per rank: host threads, pool CPU ms per step, process CPU ms per step, host cores busy | %s |" % "; ".join("rank %d: %d, %.2f, %.2f, %.2f" % (x["rank"], x["host_threads"], x["host_chain_cpu_ms_per_step"], x["host_process_cpu_ms_per_step"], x.get("host_cores_busy") or 0) for x in tp.get("per_rank", [])),
                "| `host_bound` (all ranks' cores against the schedulable ones) | %s (%.2f cores wanted) |" % (tp.get("host_bound"), tp.get("host_cores_busy_all_ranks") or 0), ""]
    pk, fpk = load(tag, "prover_kernels_serial.csv")
    if pk:
        out += ["## The prover's kernels on configs[4], one sub-batch stream (a dispatch = all 1024 proofs of a call; `%s`)" % fpk, "",
                "VALU instructions per WORKGROUP are what compares launches of different sizes: for `kp_round` a workgroup is one proof's round (the counter pass of the "
                "headline below sees the INPUT GENERATION's dispatches instead -- 4096 non-aggregated proofs per sub-batch -- which is why its per-dispatch figures are larger).", "",
                "| kernel | dispatches | avg us | workgroups per dispatch | VALU instructions per dispatch | per workgroup | wait frac |", "|---|---|---|---|---|---|---|"]
        out += ["| `%s` | %s | %s | %s | %s | %s | %s |" % (r["kernel"], r["dispatches"], r["avg_us"], r.get("workgroups_per_dispatch", ""), r.get("valu_per_dispatch", ""),
                                                        r.get("valu_per_workgroup", ""), r.get("wait_inst_frac", "")) for r in pk[:12]] + [""]
    wp, fwp = load(tag, "wave_probe.jsonl")
    if wp:
        out += ["## The sharded forms on one rank (`tools/wave_probe.py`, `%s`)" % fwp, "",
                "`wave` = k batches on k contexts (`bpp_verify_sharded_wave`), `groups` = k batches resident as ONE batch on one context "
                "(`bpp_verify_sharded_groups`), `pipeS` = one host thread pipelining S such grouped batches (`bpp_verify_sharded_groups_wave`); proofs per batch on this rank: 4096 = the whole reference batch, 512 = what one of eight ranks holds "
                "(its kernels; the weight chain of a real eight-rank run covers all 4096 proofs on every rank).", "",
                "| form | calls in flight x batches | proofs per batch here | proofs/s | ms per call | chains ms | wait phase 2 ms |", "|---|---|---|---|---|---|---|"]
        out += ["| %s | %d x %d | %d | %s | %.2f | %.2f | %.2f |" % (x.get("form", "wave"), x["waves"] * (int(x["form"][4:]) if x.get("form", "").startswith("pipe") else 1), x["batches_per_wave"], x.get("proofs_per_batch", 4096), M(x["proofs_per_s"]), x["ms_per_wave"],
                                                                     x["last_wave_host_ms"]["chains_ms"], x["last_wave_host_ms"]["wait2_ms"]) for x in wp] + [""]
    cp, fcp = load(tag, "chunk_probe.jsonl")
    if cp:
        out += ["## Throughput against the size of the reference batch (`tools/chunk_probe.py`, `%s`)" % fcp, "",
                "65 536 resident proofs per step, several steps in flight, cut into reference batches of `chunk` proofs (the reference's own `verify_batch` "
                "cuts at 256; BASELINE configs[1] is quoted on 1024).", "",
                "| proofs per reference batch | batches per step | proofs/s | ms per step | MSM window bits x windows |", "|---|---|---|---|---|"]
        out += ["| %d | %d | %s | %.3f | %d x %d |" % (x["chunk"], x["groups"], M(x["proofs_per_s"]), x["ms_per_step"], x["profile_mean"].get("msm_window_bits", 0),
                                                   x["profile_mean"].get("msm_windows", 0)) for x in cp] + [""]
    ci, fci = load(tag, "calls_in_flight.jsonl")
    if ci:
        out += ["## Independent small calls (`tools/wide_probe.py`, `%s`)" % fci, "",
                "S host threads, each verifying ONE 256-proof reference batch per call as fast as it can (what separate callers of `verify_batch` "
                "do; the same from C++ threads: `tools/cpp/calls_in_flight.cpp`).  `resident` / `packed`: every thread has a context of its own and "
                "calls `bpp_verify_resident` / `bpp_verify_batch_packed`: the rate stops at about 5 000 calls per second whatever the number of callers "
                "(a small call is a chain of latency-bound kernels with tiny grids and the chip runs about six of them "
                "side by side: DESIGN 4.1) -- and, since round 4, STAYS there with 32 and 64 callers: the library admits twelve small calls per device at a time "
                "(`packed, gate off`: the same callers without the gate, as round 3 measured them).  `batcher`: the same calls through ONE `bpp_batcher`, which pools the calls that are waiting into grouped "
                "engine calls.  A caller that holds a whole list hands it over in ONE call (`chunk = 256`): the table above.", "",
                "| callers | form | calls/s | proofs/s | ms per call |", "|---|---|---|---|---|"]
        out += ["| %d | %s | %.0f | %s | %.2f |" % (x["in_flight"], x.get("form", "packed" if x["host_buffers_in"] else "resident"), x["calls_per_s"], M(x["proofs_per_s"]),
                                              x["ms_per_call_per_context"]) for x in ci] + [""]
    fct = os.path.join(P, "msm_ct.json")
    out += ["## Constant-time MSM for B1 callers (`tools/bench_msm_ct.py`, `profiles/msm_ct.json`)", ""]
    if not os.path.exists(fct):
        out += ["unmeasured", ""]
    else:
        ct = json.loads([x for x in open(fct).read().splitlines() if x.strip().startswith("{")][-1])
        cell = lambda v: "%.3f (%.3f-%.3f)" % (v["ms"], v["lo"], v["hi"]) if v else ""
        out += ["`bpp_msm_ct_batched` per call, ms: upload, decompression of the points and the copy back included; median of %d alternating rounds "
                "of %d calls (lowest-highest round).  Output bytes equal across all columns of a row: %s.  The scalar patterns are a report, not a "
                "test: the argument for uniformity is the recorded table reads (`tests/test_msm_ct_host.py`)." %
                (ct["reps"], ct["inner"], "yes" if all(r["equal_bytes"] for r in ct["shapes"] + ct.get("rule_shapes", [])) else "NO"), "",
                "| groups x terms | K = 1 | K = 2 | `bpp_msm_vartime_batched` | `bpp_pedersen_commit` | rule's form: all-zero scalars | random | all l - 1 |",
                "|---|---|---|---|---|---|---|---|"]
        for r in ct["shapes"] + ct.get("rule_shapes", []):
            f, sp = r["forms_and_others"], r.get("scalar_patterns_rule_form", {"zero": None, "random": None, "l-1": None})
            out.append("| %d x %d | %s | %s | %s | %s | %s | %s | %s |" % (r["groups"], r["terms_per_group"], cell(f["ct_k1"]), cell(f["ct_k2"]), cell(f.get("vartime")),
                                                                    cell(f.get("pedersen_commit")), cell(sp["zero"]), cell(sp["random"]), cell(sp["l-1"])))
        out += ["", "| kernel (from the build) | VGPRs | SGPRs | scratch bytes | LDS bytes |", "|---|---|---|---|---|"]
        out += ["| `%s` | %d | %d | %d | %d |" % (k, v["vgpr"], v["sgpr"], v["scratch"], v["lds"]) for k, v in sorted(ct.get("build", {}).items())] + [""]
    fin = os.path.join(P, "ingest.json")
    out += ["## Upload of a packed batch: host arrays against arrays in device memory (`tools/bench_ingest.py`, `profiles/ingest.json`)", ""]
    if not os.path.exists(fin):
        out += ["unmeasured", ""]
    else:
        ing = json.loads([x for x in open(fin).read().splitlines() if x.strip().startswith("{")][-1])
        out += ["The upload alone, no verification (m = 1, t = 1, 64 bits): `bpp_batch_upload_packed` from page-locked host arrays against "
                "`bpp_batch_upload_packed_device` from arrays already in HBM (`csrc/ingest.h`), ms per call: median of %d alternating rounds of %d calls "
                "(lowest-highest round); CPU time of the process and of the host worker pool per call.  A record: no ratio is promised." %
                (ing["reps"], ing["inner"]), "",
                "| proofs per call | host arrays, ms | device arrays, ms | process CPU ms per call, host / device | worker pool CPU ms per call, host / device |",
                "|---|---|---|---|---|"]
        cell = lambda v: "%.3f (%.3f-%.3f)" % (v["ms"], v["lo"], v["hi"])
        out += ["| %d | %s | %s | %.3f / %.3f | %.3f / %.3f |" % (r["proofs"], cell(r["host"]), cell(r["device"]), r["host"]["cpu_ms_per_call"],
                                                                 r["device"]["cpu_ms_per_call"], r["host"]["pool_cpu_ms_per_call"],
                                                                 r["device"]["pool_cpu_ms_per_call"]) for r in ing["sizes"]] + [""]
    fre = os.path.join(P, "refill.json")
    out += ["## A producer's step from device memory: a fresh upload per step against a refill (`tools/bench_refill.py`, `profiles/refill.json`)", ""]
    if not os.path.exists(fre):
        out += ["unmeasured", ""]
    else:
        rows = json.load(open(fre))
        med = lambda arm, k: statistics.median(r[k] for r in rows if r.get("arm") == arm and k in r)  # noqa: E731
        span = {r["arm"]: r for r in rows if "ingest_span_ms_median" in r}
        kern = {r["kernel"].split("::")[-1]: r for r in rows if "kernel" in r}
        stats = next(r["refill_arm"] for r in rows if "refill_arm" in r)
        reps = len([r for r in rows if r.get("arm") == "refill" and "steps" in r])
        steps = next(r["steps"] for r in rows if "steps" in r)
        out += ["One thread, one context, a ring of 4 device input sets of 1024 proofs (m = 1, 64 bits), one verification enqueued per step: "
                "`bpp_batch_upload_packed_device` + `bpp_verify_enqueue` + `bpp_batch_destroy` per step against `bpp_batch_refill_enqueue` + "
                "`bpp_verify_enqueue` on one batch (`csrc/refill.h`); medians of %d alternating repetitions of %d steps.  Over %d refills: %d host "
                "waits in the refill, %d in the enqueues behind them, %d layouts planned.  A record: no ratio is promised." %
                (reps, steps, stats["refills"], stats["refill_host_waits"], stats["enqueue_host_waits"], stats["layouts_in_call"]), "",
                "| arm | steps/s | ms per step | host ms in the step's calls | process CPU ms per step | the ingest part on the device, ms (events around the call) |",
                "|---|---|---|---|---|---|"]
        for arm in ("upload", "refill"):
            out.append("| %s | %.1f | %.3f | %.3f | %.3f | %.3f |" % (arm, med(arm, "steps_per_s"), med(arm, "ms_per_step"), med(arm, "host_ms_per_step_median"),
                                                                   med(arm, "cpu_ms_per_step"), span[arm]["ingest_span_ms_median"]))
        if kern:
            out += ["", "Kernels, from a kernel trace of a shorter run of the same program (avg us, min-max): " +
                    ", ".join("`%s` %.2f (%.2f-%.2f)" % (k, v["avg_us"], v["min_us"], v["max_us"]) for k, v in sorted(kern.items())) + "."]
        out.append("")
    fco = os.path.join(P, "refill_count.json")
    out += ["## A refill with fewer items than the batch holds (`bpp_batch_refill_enqueue_count`, `tools/bench_refill.py --count K`, `profiles/refill_count.json`)", ""]
    if not os.path.exists(fco):
        out += ["unmeasured", ""]
    else:
        d = json.load(open(fco))
        out += ["Cost with no count: the parent commit's library against the tree with the live count, alternating on one MI355X (`tools/gpu_ab.py`, "
                "`BPP_LIB_PATH`); median (lowest-highest) over the runs of each arm.  A run outside the parent's own range is counted.", "",
                "| figure | parent | with the live count | runs below the parent's lowest | above its highest |", "|---|---|---|---|---|"]
        cell = lambda j, who: "%.2f (%.2f-%.2f)" % (j[who + "_median"], j[who + "_min"], j[who + "_max"])  # noqa: E731
        rows = [("`tools/bench_refill.py`, refill arm, steps/s", d["bench_refill_steps_per_s"]["refill"]),
                ("`tools/bench_refill.py`, upload arm, steps/s", d["bench_refill_steps_per_s"]["upload"])]
        rows += [("`bench.py --gpus 1 --steps 20 --warmup 5`, M proofs/s, %s (%d runs per arm)" % (s.replace("_", " "), len(j["runs"]["parent"])), j)
                 for s, j in sorted(d["bench_py_M_proofs_per_s"].items())]
        for name, j in rows:
            out.append("| %s | %s | %s | %d | %d |" % (name, cell(j, "parent"), cell(j, "this"), len(j["this_below_parent_min"]), len(j["this_above_parent_max"])))
        arms = d["count_arms"]["rows"]
        med = lambda arm, k: statistics.median(r[k] for r in arms if r.get("arm") == arm and k in r)  # noqa: E731
        span = {r["arm"]: r for r in arms if "ingest_span_ms_median" in r}
        names = [a for a in dict.fromkeys(r["arm"] for r in arms if "steps_per_s" in r) if a.startswith("refill")]
        out += ["", "What a step costs when K of the batch's 1024 slots are live (this tree; one group, one verification enqueued per step; no kernel "
                "skips a dead slot, so no figure is promised; that fewer live items came out faster has not been profiled per kernel -- presumably "
                "the final MSM, which has no bucket to visit for the zero scalars of a dead slot).  A record, not a bar.", "",
                "| arm | steps/s | ms per step | host ms in the step's calls | the refill on the device, ms (events around the call) |", "|---|---|---|---|---|"]
        for arm in names:
            out.append("| %s | %.1f | %.3f | %.3f | %.3f |" % (arm, med(arm, "steps_per_s"), med(arm, "ms_per_step"), med(arm, "host_ms_per_step_median"),
                                                              span[arm]["ingest_span_ms_median"]))
        out.append("")
    out += refill_mixed_section()
    out += item_transcripts_section()
    out += prove_device_section()
    out += prove_enqueue_section()
    out += transcript_ops_section()
    out += transcript_rng_section()
    out += rows_msm_section()
    ks, fks = load(tag, "kernel_stats_cfg2_default.csv")
    sq, fsq = load(tag, "pmc_sq_summary.csv")
    if ks:
        alone = {r["kernel"]: r for r in (sq or [])}
        out += ["## Kernels of the headline step (rocprofv3 kernel trace of the default command: `%s`; alone = one step in flight, SQ counter pass: `%s`)" % (fks, fsq), "",
                "(`kp_*`, `k_fb_*`, `k_ct_*` rows: the run's INPUT GENERATION by the batch prover -- 4096 non-aggregated proofs per dispatch -- not part of a step.)", "",
                "| kernel | dispatches | avg us, steps in flight as in the headline | avg us alone | ratio | share of kernel time | VGPRs | scratch bytes | VALU instr per dispatch | per workgroup | wait frac alone |", "|---|---|---|---|---|---|---|---|---|---|---|"]
        for r in ks[:16]:
            a = alone.get(r["kernel"])
            au = float(a["avg_us"]) if a else 0.0
            out.append("| `%s` | %s | %s | %s | %s | %s | %s | %s | %s | %s | %s |" % (r["kernel"], r["dispatches"], r["avg_us"], ("%.1f" % au) if a else "", ("%.1f" % (float(r["avg_us"]) / au)) if au else "",
                                                                          r["share_of_kernel_time"], r["vgpr"], r.get("scratch", ""), a["valu_per_dispatch"] if a else "",
                                                                          a.get("valu_per_workgroup", "") if a else "", a["wait_inst_frac"] if a else ""))
        blits = [r for r in ks if "copyBuffer" in r["kernel"] or "fillBuffer" in r["kernel"]]
        steps = max([int(r["dispatches"]) for r in ks if r["kernel"].startswith("k_msm_accumulate")] or [1])
        out.append("")
        out.append("Copy / fill kernels of the runtime in the whole trace (input generation by the prover, uploads, planning included): %s -- against %d steps: none is part of a step (round 3: five `__amd_rocclr_copyBuffer` dispatches per step)." %
                   (", ".join("`%s` x %s" % (r["kernel"], r["dispatches"]) for r in blits) or "none", steps))
        out.append("")
    print("\n".join(out))


if __name__ == "__main__":
    main()
