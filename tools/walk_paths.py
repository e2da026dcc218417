"""Times the tree walk in front of the path probe and the leaf search, on one GPU.

  python tools/walk_paths.py [--total-keys 100000000] [--queries 25000000] [--reps 7]
                             [--kinds bloom,vqf] [--host-threads 16] [--step-limit 240] [--log FILE]
                             [--no-host] [--no-resources]

Setup: --total-keys 16-byte keys in 16,384-key leaves (6,104 leaves at 100M, the bench's config 2
count) hung into a tree of height 3: a root of 32 pivots over 32 middle nodes of 4 pivots over 128
nodes of height 1 with 32 leaves each (4,096 leaves, 161 nodes).  The other leaves are update-buffer
segments: 4 levels of 6 on the root and, on every middle node, 6 levels of 11, 11, 10, 10, 10 and 10
(fewer where --total-keys is small).  A level is one sorted run cut into leaves, so a lookup meets
the one or two segments of a level whose range covers its pivot.  So that no global sort is needed,
a leaf's key range is the top 12 bits of its keys: a bottom leaf holds one value, a segment a span
of them (random within the span); the other 116 bits are the bench's splitmix keys, and every leaf
is sorted by bytes on the device, outside every timed region.  Bloom at 10 bits/key and VQF at 12 are
built over all leaves.  The batch: --queries lookups, half hits (random built keys) and half seed-43
misses, shuffled.

Before timing it checks that every hit is found at its own index, in its own leaf, through
tkv_amq_walk_paths -> tkv_amq_path_probe (n_entries = the capacity, the walk's page ids) ->
tkv_amq_find_keys, that no miss is found, and that the host walk counts the same entries.
Timed with device events, alternating in one process after all are warm:
  (a) tkv_amq_walk_paths alone (keys -> paths with page ids);
  (b) the three-call chain: the whole batched multi-get from keys;
  (c) TreeIndex::walk_host of the C++ mirror on --host-threads threads over the same batch
      (tools/walk_host_bench.cpp, compiled here; host clock).
Reports each with its spread, the walk's share of the chain, and the compiler's resource report of
the kernels.  Every step runs under its own time limit (the process exits if one overruns).  Prints
one JSON line per kind.  Needs a GPU; fails without one."""
import argparse
import contextlib
import ctypes
import faulthandler
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import SEG_KEYS, segment_counts, sort_segments_device, splitmix_keys16  # noqa: E402

VQF_CAP = 32704
PREFIX_BITS = 12
N_BOTTOM = 1 << PREFIX_BITS            # bottom leaves: one 12-bit prefix each
ROOT_PIVOTS, MID_PIVOTS, H1_PIVOTS = 32, 4, 32
ROOT_LEVELS = [6, 6, 6, 6]
MID_LEVELS = [11, 11, 10, 10, 10, 10]


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


RESOURCE_KEYS = ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]",
                 "LDS Size [bytes/block]", "VGPRs Spill", "SGPRs Spill")


def resource_report(log, source="tkv_amq_walk.hip", wanted=(), timeout=300):
    """Registers, LDS and scratch from the compiler, for the kernels of the unit csrc/`source` whose
    demangled name contains one of `wanted` (none given: every kernel).  The unit is compiled for
    the device only.  False if it did not compile."""
    src = os.path.join(ROOT, "turtle_kv_amd", "csrc", source)
    with tempfile.TemporaryDirectory() as d:
        r = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "--offload-arch=gfx950", "-std=c++17", "-c", "-fPIC",
                            "--cuda-device-only", "-I" + os.path.join(ROOT, "include"),
                            "-Rpass-analysis=kernel-resource-usage", src, "-o", os.path.join(d, "k.o")],
                           capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:
        say(log, "resource report: compile failed:", r.stderr[-400:])
        return False
    names = subprocess.run(["c++filt"], input="\n".join(re.findall(r"Function Name: (\S+)", r.stderr)),
                           capture_output=True, text=True, check=True).stdout.split("\n")
    cur, at = None, 0
    for line in r.stderr.splitlines():
        if "remark:" not in line:
            continue
        text = line.split("remark:", 1)[1].split("[-Rpass")[0].strip()
        if text.startswith("Function Name:"):
            if cur:
                say(log, "resources", json.dumps(cur))
            cur = {"kernel": names[at]} if not wanted or any(w in names[at] for w in wanted) else None
            at += 1
        elif cur is not None and ":" in text:
            k, v = text.split(":", 1)
            if k.strip() in RESOURCE_KEYS:
                cur[k.strip()] = v.strip()
    if cur:
        say(log, "resources", json.dumps(cur))
    return True


# ---------------------------------------------------------------------------------------
# the tree: prefix ranges, so everything about it is arithmetic
# ---------------------------------------------------------------------------------------
def prefix_key(prefix):
    """The smallest 16-byte key whose top 12 bits are `prefix` (4096: above every key)."""
    if prefix >= N_BOTTOM:
        return b"\xff" * 16
    return bytes([prefix >> 4, (prefix & 15) << 4]) + b"\x00" * 14


def cut(lo, hi, j, n):
    """Part j of n of the prefix range [lo, hi)."""
    w = hi - lo
    return lo + -(-w * j // n), lo + -(-w * (j + 1) // n)


def level_shapes(n_seg_leaves):
    """How the segment leaves are spread: the root's levels first, then every middle node's, a
    level dropped where the leaves run out.  Returns (root levels, per middle node its levels)."""
    left = n_seg_leaves
    root = []
    for n in ROOT_LEVELS:
        take = min(n, left)
        if take:
            root.append(take)
        left -= take
    mids = []
    for _ in range(ROOT_PIVOTS):
        levels = []
        for n in MID_LEVELS:
            take = min(n, left)
            if take:
                levels.append(take)
            left -= take
        mids.append(levels)
    assert left == 0, "more leaves than the tree's update buffers hold"
    return root, mids


def build_tree(n_leaves):
    """(nested description, per leaf its prefix range).  Leaves 0..4095 are the bottom ones; the
    segments' leaves follow in the order level_shapes names them."""
    assert n_leaves >= N_BOTTOM
    root_levels, mid_levels = level_shapes(n_leaves - N_BOTTOM)
    ranges = [(s, s + 1) for s in range(N_BOTTOM)]
    nxt = [N_BOTTOM]

    def levels_over(lo, hi, shape, n_pivots):
        out, width = [], (hi - lo) // n_pivots
        for n in shape:
            level = []
            for j in range(n):
                a, b = cut(lo, hi, j, n)
                active = 0
                for p in range(n_pivots):
                    if a < lo + (p + 1) * width and b > lo + p * width:
                        active |= 1 << p
                level.append({"leaf": nxt[0], "page_id": nxt[0], "active": active, "flushed": {}})
                ranges.append((a, b))
                nxt[0] += 1
            out.append(level)
        return out

    per_mid, per_h1 = N_BOTTOM // ROOT_PIVOTS, N_BOTTOM // ROOT_PIVOTS // MID_PIVOTS
    root = {"pivot_keys": [prefix_key(per_mid * m) for m in range(ROOT_PIVOTS + 1)], "children": [], "page_id": 0}
    root["levels"] = levels_over(0, N_BOTTOM, root_levels, ROOT_PIVOTS)
    for m in range(ROOT_PIVOTS):
        lo = per_mid * m
        mid = {"pivot_keys": [prefix_key(lo + per_h1 * c) for c in range(MID_PIVOTS + 1)], "children": [],
               "page_id": 1_000_000 + m, "levels": levels_over(lo, lo + per_mid, mid_levels[m], MID_PIVOTS)}
        for c in range(MID_PIVOTS):
            first = lo + per_h1 * c
            mid["children"].append({"pivot_keys": [prefix_key(first + i) for i in range(H1_PIVOTS + 1)],
                                    "children": [{"leaf": first + i, "page_id": first + i} for i in range(H1_PIVOTS)],
                                    "levels": [], "page_id": 2_000_000 + first})
        root["children"].append(mid)
    assert nxt[0] == n_leaves and len(ranges) == n_leaves
    return root, ranges


def gen_keys(torch, n_keys, ranges, dev, chunk=1 << 23):
    """Key i: the bench's splitmix key i with its top 12 bits replaced by a prefix of its leaf's
    range (leaf i // 16,384), drawn with the bits it replaces."""
    lo = torch.tensor([r[0] for r in ranges], dtype=torch.int64, device=dev)
    span = torch.tensor([r[1] - r[0] for r in ranges], dtype=torch.int64, device=dev)
    out = torch.empty((n_keys, 16), dtype=torch.uint8, device=dev)
    words = out.view(torch.int64).view(n_keys, 2)
    for b in range(0, n_keys, chunk):
        idx = torch.arange(b, min(b + chunk, n_keys), dtype=torch.int64, device=dev)
        w = splitmix_keys16(torch, 42, idx).contiguous().view(torch.int64).view(-1, 2)
        leaf = idx // SEG_KEYS
        old = w[:, 0] & 0xFFFF                                   # bytes 0 and 1 (little-endian word)
        prefix = lo[leaf] + ((old >> 4) & 0xFFF) % span[leaf]
        two = (prefix >> 4) | ((((prefix & 15) << 4) | ((old >> 8) & 15)) << 8)
        words[b:b + idx.numel(), 0] = (w[:, 0] & ~0xFFFF) | two
        words[b:b + idx.numel(), 1] = w[:, 1]
    return out


# ---------------------------------------------------------------------------------------
# the host baseline: TreeIndex::walk_host of the C++ mirror
# ---------------------------------------------------------------------------------------
def host_walk(log, tree, q_host, threads, reps, workdir):
    exe = os.path.join(workdir, "walk_host_bench")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                        os.path.join(ROOT, "tools", "walk_host_bench.cpp"),
                        "-L" + os.path.join(ROOT, "turtle_kv_amd"), "-ltkv_amq", "-pthread",
                        "-Wl,-rpath," + os.path.join(ROOT, "turtle_kv_amd")], capture_output=True, text=True,
                       timeout=300)
    if r.returncode != 0:
        sys.exit("walk_host_bench did not compile: " + r.stderr[-800:])
    for name, a in (("nodes", tree.nodes), ("segments", tree.segments), ("children", tree.children),
                    ("bounds", tree.flushed_bounds)):
        a.tofile(os.path.join(workdir, name + ".bin"))
    assert all(len(k) == 16 for k in tree.pivot_keys)
    with open(os.path.join(workdir, "pivot_keys.bin"), "wb") as f:
        f.write(b"".join(tree.pivot_keys))
    q_host.tofile(os.path.join(workdir, "queries.bin"))
    r = subprocess.run([exe, workdir, str(threads), str(reps)], capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        sys.exit("walk_host_bench failed: " + r.stdout[-400:] + r.stderr[-400:])
    say(log, "host", r.stdout.strip().splitlines()[-1])
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--total-keys", type=int, default=100_000_000)
    ap.add_argument("--queries", type=int, default=25_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--kinds", default="bloom,vqf")
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--step-limit", type=int, default=240)
    ap.add_argument("--log", default=None)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-resources", action="store_true")
    args = ap.parse_args()
    import torch
    import turtle_kv_amd as amq
    if not torch.cuda.is_available():
        sys.exit("tools/walk_paths.py needs a GPU")
    assert args.reps >= 7, "at least 7 repetitions of each route"
    log = open(args.log, "w") if args.log else None
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lim = args.step_limit
    L, F = amq.abi.lib(), amq.filters
    sh = F._stream_handle()
    say(log, "walk_paths:", amq.abi.version(), "|", torch.cuda.get_device_name(0))
    if not args.no_resources:
        with step_limit(300, "resource report"):
            resource_report(log)

    counts = segment_counts(args.total_keys)
    n_leaves, nq = len(counts), args.queries
    with step_limit(lim, "tree"):
        desc, ranges = build_tree(n_leaves)
        tree = amq.TreeIndex.from_description(desc)
        d_nodes, d_segs, d_kids, d_bounds, pk = tree.device(dev)
    say(log, f"tree: height {int(tree.nodes[0]['height'])}, {len(tree.nodes)} nodes, {len(tree.children)} children "
             f"({N_BOTTOM} bottom leaves), {len(tree.segments)} segments, {len(tree.pivot_keys)} pivot keys")
    with step_limit(lim, "keys, sorted per leaf"):
        keys = sort_segments_device(torch, gen_keys(torch, args.total_keys, ranges, dev), counts)
        kb = amq.KeyBatch.fixed(keys)
        torch.cuda.synchronize()

    with step_limit(lim, "queries"):
        # half hits (random built keys, by their index in the sorted array), half seed-43 misses
        g = torch.Generator(device=dev)
        g.manual_seed(44)
        perm = torch.randperm(nq, device=dev, generator=g)
        is_hit = perm < nq // 2
        hit_key = torch.randint(0, args.total_keys, (nq,), device=dev, generator=g)
        words = keys.view(torch.int64).reshape(-1, 2)            # (row gathers on the int64 view)
        miss = splitmix_keys16(torch, 43, perm).contiguous().view(torch.int64).reshape(-1, 2)
        q = torch.where(is_hit[:, None], words[hit_key], miss).contiguous().view(torch.uint8).reshape(nq, 16)
        del miss, perm
        own = (hit_key // SEG_KEYS).to(torch.int32)
        n_hits = int(is_hit.sum())
        torch.cuda.synchronize()

    ws_walk = torch.empty(amq.walk_paths_workspace_bytes(nq), dtype=torch.uint8, device=dev)
    path_begin = torch.empty(nq + 1, dtype=torch.int32, device=dev)
    needed = torch.zeros(1, dtype=torch.int64, device=dev)

    def walk(cap, leaf, page):
        amq.walk_paths_device(d_nodes, len(tree.nodes), d_segs, len(tree.segments), d_kids, len(tree.children),
                              d_bounds, len(tree.flushed_bounds), pk.data, pk.offsets, pk.stride, pk.n, q, None, 16,
                              nq, path_begin, leaf, cap, ws_walk, page, None, None, needed)

    with step_limit(lim, "walk: sizing run"):
        walk(0, None, None)
        torch.cuda.synchronize()
        total = int(needed.item())
    cap = total + 1024                                           # (a capacity past the total, as a caller would size it)
    say(log, f"{args.total_keys} keys in {n_leaves} sorted leaves; {nq} queries ({n_hits} hits); {total} path "
             f"entries ({total / nq:.2f} per query), capacity {cap}")
    assert cap < 1 << 31
    path_leaf = torch.empty(cap, dtype=torch.int32, device=dev)
    path_page = torch.empty(cap, dtype=torch.int64, device=dev)
    ws = torch.empty(amq.path_probe_workspace_bytes(nq, cap), dtype=torch.uint8, device=dev)
    cand_begin = torch.empty(nq + 1, dtype=torch.int32, device=dev)
    cand_leaf = torch.empty(cap, dtype=torch.int32, device=dev)
    cand_entry = torch.empty(cap, dtype=torch.int32, device=dev)
    result = torch.empty(16 * nq, dtype=torch.uint8, device=dev)
    fc = amq.FindCounts(dev)

    host = None
    with step_limit(lim, "walk: check against the host's counts"):
        walk(cap, path_leaf, path_page)
        torch.cuda.synchronize()
        assert int(path_begin[-1].item()) == total == int(needed.item())
        dev_sums = {"entries": total, "leaf_sum": int(path_leaf[:total].to(torch.int64).sum().item()),
                    "begin_sum": int(path_begin.to(torch.int64).sum().item())}
        assert bool((path_page[:total] == path_leaf[:total].to(torch.int64)).all()), "page ids are the leaf numbers"
    if not args.no_host:
        with step_limit(900, "host walk"), tempfile.TemporaryDirectory() as d:
            host = host_walk(log, tree, q.cpu().numpy(), args.host_threads, args.host_reps, d)
        for k, v in dev_sums.items():
            assert host[k] == v, (k, host[k], v)
        say(log, f"host walk: the same {total} entries (leaf sum {dev_sums['leaf_sum']})")

    for name in args.kinds.split(","):
        kind, bpk = (amq.BLOOM, 10) if name == "bloom" else (amq.VQF, 12)
        with step_limit(lim, f"{name}: build"):
            plan = amq.plan_filters(kind, counts, bpk, payload_capacity=VQF_CAP if kind else 0)
            filt = amq.build_all_filters(plan, kb)
            segs = plan.device_segs(dev)
            torch.cuda.synchronize()
        opts = amq.abi.ProbeOpts(path_page.data_ptr(), None, None)

        def walk_full():
            walk(cap, path_leaf, path_page)

        def chain(counted=False):
            walk_full()
            amq.abi.check(L.tkv_amq_path_probe(
                kind, F._ptr(filt), F._ptr(segs), plan.n_segs, F._ptr(q), None, 16, nq, F._ptr(path_begin),
                F._ptr(path_leaf), cap, None, F._ptr(cand_begin), F._ptr(cand_leaf), F._ptr(cand_entry),
                ctypes.byref(opts), F._ptr(ws), ws.numel(), sh), "tkv_amq_path_probe")
            amq.abi.check(L.tkv_amq_find_keys(
                kind, F._ptr(filt), F._ptr(segs), plan.n_segs, F._ptr(q), None, 16, nq, F._ptr(cand_begin),
                F._ptr(cand_leaf), F._ptr(cand_entry), cap, F._ptr(keys), None, 16, args.total_keys, None, 0,
                F._ptr(result), None, ctypes.byref(opts), F._ptr(fc.counts) if counted else None, sh),
                "tkv_amq_find_keys")

        with step_limit(lim, f"{name}: check"):
            fc.reset()
            chain(counted=True)
            torch.cuda.synchronize()
            n_cand = int(cand_begin[-1].item())
            rec = result.view(torch.int64).view(nq, 2)
            lc = result.view(torch.int32).view(nq, 4)
            assert torch.equal(rec[:, 0][is_hit], hit_key[is_hit]), "a hit query was not found at its own index"
            assert torch.equal(lc[:, 2][is_hit], own[is_hit]), "a hit query was found in another leaf"
            assert bool((rec[:, 0][~is_hit] == -1).all()), "a miss was found"
            c = fc.collect()
            assert c["found_count"] == n_hits and c["unsearchable_count"] == 0
            say(log, f"{name}: every hit found at its own index through walk -> path_probe -> find_keys; "
                     f"{n_cand} candidates of {total} entries, {c['leaf_search_count']} searched")

        with step_limit(lim, f"{name}: timing"):
            for _ in range(2):   # warm both
                walk_full()
                chain()
            ta, tb = [], []
            for _ in range(args.reps):   # alternate
                ta.append(timed(torch, walk_full))
                tb.append(timed(torch, chain))
        a, b = spread(ta), spread(tb)
        out = {"kind": name, "bits_per_key": bpk, "leaves": n_leaves, "nodes": len(tree.nodes), "queries": nq,
               "entries": total, "entries_per_query": round(total / nq, 2), "candidates": n_cand,
               "searched": c["leaf_search_count"], "found": c["found_count"],
               "walk_paths": a, "walk_probe_find": b,
               "walk_paths_ms_all": [round(x, 3) for x in ta], "walk_probe_find_ms_all": [round(x, 3) for x in tb],
               "walk_share_of_chain": round(a["median_ms"] / b["median_ms"], 3),
               "ns_per_query_walk": round(a["median_ms"] * 1e6 / nq, 3),
               "m_lookups_per_s_chain": round(nq / b["median_ms"] / 1e3, 1)}
        if host:
            out["walk_host"] = {"threads": host["threads"], "median_ms": host["median_ms"], "min_ms": host["min_ms"],
                                "max_ms": host["max_ms"], "reps": host["reps"]}
            out["walk_host_over_device"] = round(host["median_ms"] / a["median_ms"], 1)
        say(log, json.dumps(out))
        del filt
    if log:
        log.close()


if __name__ == "__main__":
    main()
