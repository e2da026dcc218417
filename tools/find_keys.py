"""Times the leaf search behind the path probe, on one GPU.

  python tools/find_keys.py [--total-keys 100000000] [--queries 25000000] [--path-len 8]
                            [--reps 7] [--kinds bloom,vqf] [--step-limit 180] [--log FILE]
                            [--no-resources]

Setup: the bench's leaves (--total-keys 16-byte keys in 16,384-key leaves: 6,104 leaves at 100M),
each leaf sorted by bytes on the device with torch (outside every timed region), Bloom at 10
bits/key and VQF at 12 built from them; the batch of tools/path_probe.py -- --queries lookups, half
hits (random built keys) and half seed-43 misses, shuffled, each with a path of --path-len leaves:
one random leaf per "level", a hit's own leaf at a random position.

Before timing it checks that every hit query is found at its own index, in its own leaf, and that
no miss is found.  Timed with device events, alternating in one process after all are warm:
  (a) tkv_amq_path_probe alone (keys + CSR lists -> compacted candidates);
  (b) tkv_amq_path_probe -> tkv_amq_find_keys: the whole batched multi-get;
  (c) tkv_amq_find_keys alone, on (a)'s candidates.
Reports each with its spread, (c) relative to (a), the time per searched candidate, and the
compiler's resource report of the kernel.  Every step runs under its own time limit (the process
exits if one overruns).  Prints one JSON line per kind.  Needs a GPU; fails without one."""
import argparse
import contextlib
import ctypes
import faulthandler
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import SEG_KEYS, segment_counts, sort_segments_device, splitmix_keys16  # noqa: E402

VQF_CAP = 32704


def say(log, *a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    if log:
        log.write(line + "\n")
        log.flush()


@contextlib.contextmanager
def step_limit(seconds, what):
    """The step's own time limit: a watchdog thread ends the process (traceback on stderr) if the
    step is still running after `seconds`, even inside a device synchronise."""
    print(f"[step] {what} (limit {seconds}s)", file=sys.stderr, flush=True)
    faulthandler.dump_traceback_later(seconds, exit=True)
    try:
        yield
    finally:
        faulthandler.cancel_dump_traceback_later()


def timed(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def spread(v):
    return {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3),
            "max_ms": round(max(v), 3), "reps": len(v)}


def resource_report(log):
    """Registers, LDS and scratch of the find kernels, from the compiler."""
    src = os.path.join(ROOT, "turtle_kv_amd", "csrc", "tkv_amq_find.hip")
    with tempfile.TemporaryDirectory() as d:
        r = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "--offload-arch=gfx950", "-std=c++17", "-c", "-fPIC",
                            "--cuda-device-only", "-I" + os.path.join(ROOT, "include"),
                            "-Rpass-analysis=kernel-resource-usage", src, "-o", os.path.join(d, "k.o")],
                           capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        say(log, "resource report: compile failed:", r.stderr[-400:])
        return
    cur = {}
    for line in r.stderr.splitlines():
        if "remark:" not in line:
            continue
        text = line.split("remark:", 1)[1].split("[-Rpass")[0].strip()
        if text.startswith("Function Name:"):
            if cur:
                say(log, "resources", json.dumps(cur))
            cur = {"kernel": text.split(":", 1)[1].strip()}
        elif ":" in text:
            k, v = text.split(":", 1)
            if k.strip() in ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]",
                             "LDS Size [bytes/block]", "VGPRs Spill", "SGPRs Spill"):
                cur[k.strip()] = v.strip()
    if cur:
        say(log, "resources", json.dumps(cur))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--total-keys", type=int, default=100_000_000)
    ap.add_argument("--queries", type=int, default=25_000_000)
    ap.add_argument("--path-len", type=int, default=8)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--kinds", default="bloom,vqf")
    ap.add_argument("--step-limit", type=int, default=180)
    ap.add_argument("--log", default=None)
    ap.add_argument("--no-resources", action="store_true")
    args = ap.parse_args()
    import torch
    import turtle_kv_amd as amq
    if not torch.cuda.is_available():
        sys.exit("tools/find_keys.py needs a GPU")
    assert args.reps >= 7, "at least 7 repetitions of each route"
    log = open(args.log, "w") if args.log else None
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lim = args.step_limit
    L, F = amq.abi.lib(), amq.filters
    sh = F._stream_handle()
    say(log, "find_keys:", amq.abi.version(), "|", torch.cuda.get_device_name(0))
    if not args.no_resources:
        with step_limit(300, "resource report"):
            resource_report(log)

    counts = segment_counts(args.total_keys)
    n_leaves, nq, plen = len(counts), args.queries, args.path_len
    n_entries = nq * plen
    assert n_entries < 1 << 31
    with step_limit(lim, "keys, sorted per leaf"):
        keys = sort_segments_device(torch, amq.gen_keys16(42, 0, args.total_keys, device=dev), counts)
        kb = amq.KeyBatch.fixed(keys)
        torch.cuda.synchronize()

    with step_limit(lim, "queries and paths"):
        # half hits (random built keys, by their index in the sorted array), half seed-43 misses
        g = torch.Generator(device=dev)
        g.manual_seed(44)
        perm = torch.randperm(nq, device=dev, generator=g)
        is_hit = perm < nq // 2
        hit_key = torch.randint(0, args.total_keys, (nq,), device=dev, generator=g)
        words = keys.view(torch.int64).reshape(-1, 2)            # (row gathers on the int64 view)
        miss = splitmix_keys16(torch, 43, perm).contiguous().view(torch.int64).reshape(-1, 2)
        q = torch.where(is_hit[:, None], words[hit_key], miss).contiguous().view(torch.uint8).reshape(nq, 16)
        del miss
        own = (hit_key // SEG_KEYS).to(torch.int32)
        leaves = torch.randint(0, n_leaves, (nq, plen), device=dev, dtype=torch.int32, generator=g)
        pos = torch.randint(0, plen, (nq,), device=dev, generator=g)
        at_pos = (torch.arange(plen, device=dev)[None, :] == pos[:, None]) & is_hit[:, None]
        path_leaf = torch.where(at_pos, own[:, None], leaves).reshape(-1).contiguous()
        del at_pos, leaves, perm
        path_begin = (torch.arange(nq + 1, device=dev, dtype=torch.int64) * plen).to(torch.int32)
        n_hits = int(is_hit.sum())
        torch.cuda.synchronize()
    say(log, f"{args.total_keys} keys in {n_leaves} sorted leaves; {nq} queries ({n_hits} hits) x "
             f"{plen} leaves = {n_entries} entries")

    ws = torch.empty(amq.path_probe_workspace_bytes(nq, n_entries), dtype=torch.uint8, device=dev)
    cand_begin = torch.empty(nq + 1, dtype=torch.int32, device=dev)
    cand_leaf = torch.empty(n_entries, dtype=torch.int32, device=dev)
    result = torch.empty(16 * nq, dtype=torch.uint8, device=dev)
    fc = amq.FindCounts(dev)
    pm = amq.ProbeMetrics(dev)

    for name in args.kinds.split(","):
        kind, bpk = (amq.BLOOM, 10) if name == "bloom" else (amq.VQF, 12)
        with step_limit(lim, f"{name}: build"):
            plan = amq.plan_filters(kind, counts, bpk, payload_capacity=VQF_CAP if kind else 0)
            filt = amq.build_all_filters(plan, kb)
            segs = plan.device_segs(dev)
            torch.cuda.synchronize()

        def probe():
            amq.abi.check(L.tkv_amq_path_probe(
                kind, F._ptr(filt), F._ptr(segs), plan.n_segs, F._ptr(q), None, 16, nq, F._ptr(path_begin),
                F._ptr(path_leaf), n_entries, None, F._ptr(cand_begin), F._ptr(cand_leaf), None, None,
                F._ptr(ws), ws.numel(), sh), "tkv_amq_path_probe")

        def find(counted=False):
            o = amq.abi.ProbeOpts(None, None, pm.counts.data_ptr())
            amq.abi.check(L.tkv_amq_find_keys(
                kind, None, F._ptr(segs), plan.n_segs, F._ptr(q), None, 16, nq, F._ptr(cand_begin),
                F._ptr(cand_leaf), None, n_entries, F._ptr(keys), None, 16, args.total_keys, None, 0,
                F._ptr(result), None, ctypes.byref(o) if counted else None, F._ptr(fc.counts) if counted else None,
                sh), "tkv_amq_find_keys")

        def both():
            probe()
            find()

        with step_limit(lim, f"{name}: check"):
            fc.reset()
            pm.reset()
            probe()
            find(counted=True)
            torch.cuda.synchronize()
            total = int(cand_begin[-1].item())
            rec = result.view(torch.int64).view(nq, 2)
            lc = result.view(torch.int32).view(nq, 4)
            assert torch.equal(rec[:, 0][is_hit], hit_key[is_hit]), "a hit query was not found at its own index"
            assert torch.equal(lc[:, 2][is_hit], own[is_hit]), "a hit query was found in another leaf"
            assert bool((rec[:, 0][~is_hit] == -1).all()), "a miss was found"
            c = fc.collect()
            fp = pm.collect()["filter_false_positive_count"]
            assert c["found_count"] == n_hits and c["leaf_search_count"] == c["found_count"] + c["absent_count"]
            say(log, f"{name}: every hit found at its own index; {total} candidates of {n_entries} entries, "
                     f"{c['leaf_search_count']} searched, {fp} filter false positives among them")

        with step_limit(lim, f"{name}: timing"):
            for _ in range(2):   # warm all three
                probe()
                both()
                find()
            ta, tb, tc = [], [], []
            for _ in range(args.reps):   # alternate
                ta.append(timed(torch, probe))
                tb.append(timed(torch, both))
                tc.append(timed(torch, find))
        a, b, cc = spread(ta), spread(tb), spread(tc)
        say(log, json.dumps({
            "kind": name, "bits_per_key": bpk, "leaves": n_leaves, "queries": nq, "entries": n_entries,
            "candidates": total, "searched": c["leaf_search_count"], "found": c["found_count"],
            "filter_false_positives": fp,
            "path_probe": a, "path_probe_then_find": b, "find_keys": cc,
            "path_probe_ms_all": [round(x, 3) for x in ta], "path_probe_then_find_ms_all": [round(x, 3) for x in tb],
            "find_keys_ms_all": [round(x, 3) for x in tc],
            "find_over_path_probe": round(cc["median_ms"] / a["median_ms"], 3),
            "ns_per_searched_candidate": round(cc["median_ms"] * 1e6 / max(c["leaf_search_count"], 1), 3),
            "m_lookups_per_s": round(nq / b["median_ms"] / 1e3, 1)}))
        del filt
    if log:
        log.close()


if __name__ == "__main__":
    main()
