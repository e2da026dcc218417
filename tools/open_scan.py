"""Times tkv_amq_scan_filters against two bandwidth-bound reads of the same bytes, on one GPU.

  python tools/open_scan.py [--total-keys 100000000] [--reps 9] [--step-limit 120] [--log FILE]
                            [--no-resources]

Filter arrays (the bench's, bench.py): config 2's --total-keys 16-byte keys in 16,384-key leaves
as Bloom filters at 10 bits/key (6,104 leaves at 100M), config 3's as VQF at 12 bits/key in
32,704-byte payloads, and ONE monolithic Bloom filter over the same keys (the same bytes in one
segment).  Timed per array with device events (ten back-to-back calls per window, per-call time
reported), alternating in one process after all are warm:
  (a) tkv_amq_scan_filters (its four launches);
  (b) a device-to-device copy of the filter array (reads and writes the bytes: twice the traffic);
  (c) torch.sum over the array viewed as int64 (reads the bytes once).
The bar is relative: (a) should take no longer than (b), and the monolithic (a) should lie within
the run-to-run spread of the many-leaf (a).  tkv_amq_open_filters over the many-leaf arrays is
timed too (a header-sized read per filter; no bar).  Before timing, the scan's totals are checked
against torch (set bits of the Bloom arrays) and against the payload headers (VQF: occupied ==
nelts, no bad block).  Every step runs under its own time limit (--step-limit seconds; the
process exits if one overruns).  Prints one JSON line per array, and the compiler's resource
report of the kernels.  Needs a GPU; fails without one."""
import argparse
import contextlib
import faulthandler
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import segment_counts  # noqa: E402

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


INNER = 10   # calls per timed window, so the window holds device work and not one launch's latency


def timed(torch, fn, inner=INNER):
    """Milliseconds per call: `inner` back-to-back calls between two device events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner


def spread(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4),
            "max_ms": round(max(v), 4), "reps": len(v)}


def popcount_total(torch, t):
    """Set bits of a uint8 tensor (a multiple of 4 bytes), by SWAR on its int32 view."""
    x = t.view(torch.int32)
    x = x - ((x >> 1) & 0x55555555)
    x = (x & 0x33333333) + ((x >> 2) & 0x33333333)
    x = (x + (x >> 4)) & 0x0F0F0F0F
    x = (x * 0x01010101) >> 24
    return int((x & 0xFF).sum(dtype=torch.int64))


def resource_report(log):
    """Registers, LDS and scratch of the open/scan kernels, from the compiler."""
    src = os.path.join(ROOT, "turtle_kv_amd", "csrc", "tkv_amq_open_scan.hip")
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
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--step-limit", type=int, default=120)
    ap.add_argument("--log", default=None)
    ap.add_argument("--no-resources", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch
    import turtle_kv_amd as amq
    if not torch.cuda.is_available():
        sys.exit("tools/open_scan.py needs a GPU")
    assert args.reps >= 7, "at least 7 repetitions of each leg"
    log = open(args.log, "w") if args.log else None
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lim = args.step_limit
    say(log, "open_scan:", amq.abi.version(), "|", torch.cuda.get_device_name(0))
    if not args.no_resources:
        with step_limit(300, "resource report"):
            resource_report(log)

    counts = segment_counts(args.total_keys)
    with step_limit(lim, "keys"):
        keys = amq.gen_keys16(42, 0, args.total_keys, device=dev)
        kb = amq.KeyBatch.fixed(keys)
        torch.cuda.synchronize()

    arrays = [("bloom10_leaves", amq.BLOOM, 10, counts, 0), ("vqf12_leaves", amq.VQF, 12, counts, VQF_CAP),
              ("bloom10_monolithic", amq.BLOOM, 10, [args.total_keys], 0)]
    results = {}
    for name, kind, bpk, cnts, cap in arrays:
        with step_limit(lim, f"{name}: build"):
            plan = amq.plan_filters(kind, cnts, bpk, payload_capacity=cap)
            filt = amq.build_all_filters(plan, kb)
            torch.cuda.synchronize()
        n = plan.n_segs
        nbytes = filt.numel() // 8 * 8
        block_bytes = 64 * int(plan.segs["n_blocks"].astype(np.int64).sum())
        segs = plan.device_segs(dev)
        d_stats = torch.empty(32 * n, dtype=torch.uint8, device=dev)
        ws = torch.empty(amq.scan_filters_workspace_bytes(n), dtype=torch.uint8, device=dev)
        dst = torch.empty_like(filt)
        words = filt[:nbytes].view(torch.int64)

        def scan():
            amq.scan_filters_device(kind, filt, segs, n, d_stats, ws)

        def copy():
            dst.copy_(filt)

        def total():
            return torch.sum(words)

        with step_limit(lim, f"{name}: check"):
            scan()
            st = d_stats.cpu().numpy().view(amq.abi.FILTER_STATS_DTYPE)
            assert not st["bad_blocks"].any()
            assert int(st["header_items"].sum()) == args.total_keys
            if kind == amq.BLOOM:
                # the set bits of the whole array with the 64-byte headers cleared, counted by torch
                body = filt[:nbytes].clone()
                hdr = torch.from_numpy(plan.segs["out_offset"].astype(np.int64)).to(dev)[:, None] + \
                    torch.arange(64, device=dev)[None, :]
                body[hdr.reshape(-1)] = 0
                bits = popcount_total(torch, body)
                assert int(st["occupied"].sum()) == bits, (int(st["occupied"].sum()), bits)
                del body
                fill = amq.filter_fill(plan, st)
                assert 0.3 < float(fill.mean()) < 0.6, float(fill.mean())   # k = 7 at 10 bits/key: ~0.49
            else:
                assert np.array_equal(st["occupied"], st["header_items"])
        with step_limit(lim, f"{name}: warm"):
            for _ in range(3):
                scan()
                copy()
                total()
            torch.cuda.synchronize()
        ta, tb, tc = [], [], []
        with step_limit(lim, f"{name}: timed"):
            for _ in range(args.reps):   # alternate
                ta.append(timed(torch, scan))
                tb.append(timed(torch, copy))
                tc.append(timed(torch, total))
        a, b, c = spread(ta), spread(tb), spread(tc)
        res = {"array": name, "filters": n, "bytes": int(filt.numel()), "block_bytes": block_bytes,
               "scan": {**a, "gb_per_s": round(block_bytes / a["median_ms"] / 1e6, 1)},
               "copy_d2d": {**b, "gb_per_s_read_plus_write": round(2 * filt.numel() / b["median_ms"] / 1e6, 1)},
               "sum_int64": {**c, "gb_per_s": round(nbytes / c["median_ms"] / 1e6, 1)},
               "scan_ms_all": [round(x, 4) for x in ta], "copy_ms_all": [round(x, 4) for x in tb],
               "sum_ms_all": [round(x, 4) for x in tc],
               "calls_per_window": INNER, "scan_le_copy": a["median_ms"] <= b["median_ms"],
               "fill_mean": round(float(amq.filter_fill(plan, st).mean()), 4)}
        if n > 1:
            with step_limit(lim, f"{name}: open"):
                d_off = torch.from_numpy(plan.segs["out_offset"].view(np.int64).copy()).to(dev)
                o_segs = torch.empty(64 * n, dtype=torch.uint8, device=dev)
                o_status = torch.empty(n, dtype=torch.int32, device=dev)
                o_sum = torch.empty(7, dtype=torch.int32, device=dev)

                def opn():
                    amq.open_filters_device(kind, filt, n, o_segs, o_status, o_sum, offsets=d_off)
                opn()
                torch.cuda.synchronize()
                assert o_sum.cpu().tolist() == [n, 0, 0, 0, 0, 0, 0]
                res["open_filters_ms"] = spread([timed(torch, opn) for _ in range(args.reps)])
        results[name] = res
        say(log, json.dumps(res))
        del filt, dst, words, d_stats, ws

    many, mono = results["bloom10_leaves"]["scan"], results["bloom10_monolithic"]["scan"]
    gap = abs(mono["median_ms"] - many["median_ms"])
    many_spread = many["max_ms"] - many["min_ms"]
    say(log, json.dumps({"monolithic_vs_leaves": {"gap_ms": round(gap, 4), "leaves_spread_ms": round(many_spread, 4),
                                                  "within_spread": gap <= many_spread},
                         "scan_le_copy": {k: v["scan_le_copy"] for k, v in results.items()}}))
    if log:
        log.close()


if __name__ == "__main__":
    main()
