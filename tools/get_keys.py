"""Times the fused point lookup (tkv_amq_get_keys) against the three-call chain it replaces, on one GPU.

  python tools/get_keys.py [--total-keys 100000000] [--queries 25000000] [--reps 7]
                           [--kinds bloom,vqf] [--step-limit 240] [--log FILE]
  python tools/get_keys.py --resources-only [--log FILE]        (no GPU needed)

Setup: tools/walk_paths.py's, by import -- --total-keys 16-byte keys in 16,384-key sorted leaves
(6,104 at 100M, the bench's config 2 count) under its tree of height 3 (161 nodes, no flushed
bounds), Bloom at 10 bits/key and VQF at 12 over all leaves, --queries lookups, half hits and half
seed-43 misses, shuffled.

Before timing it checks that
  - the fused lookup finds every hit at its own index in its own leaf and no miss;
  - its (key_index, leaf) equal those of tkv_amq_walk_paths -> tkv_amq_path_probe ->
    tkv_amq_find_keys, query for query (the tree has no flushed bounds);
  - its d_metrics equal a recount on the host from d_query_visits and the results: every visit is a
    filter query; on this tree every leaf is in the plan under its own page id, so no visit is "no
    filter" or a mismatch; the positives are the searches; with no flushed bound every search
    either finds its query's key or is a false positive; the rest were rejected.
Timed with device events, alternating in one process after both are warm:
  (a) the three-call chain with the walk's page ids checked by the probe and the search;
  (b) tkv_amq_get_keys with TKV_AMQ_GET_CHECK_PAGE_ID (results only: no visits, metrics or counts).
Reports each with its spread, their ratio, whether the two ranges overlap, and the visits per
lookup of hits and misses beside the chain's path entries per lookup.  Every step runs under its
own time limit.  Prints one JSON line per kind.  --resources-only prints the compiler's resource
report of the get_keys kernels and exits."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench import SEG_KEYS, segment_counts, sort_segments_device, splitmix_keys16  # noqa: E402
from walk_paths import VQF_CAP, build_tree, gen_keys, resource_report, say, spread, step_limit, timed  # noqa: E402

def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--total-keys", type=int, default=100_000_000)
    ap.add_argument("--queries", type=int, default=25_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--kinds", default="bloom,vqf")
    ap.add_argument("--step-limit", type=int, default=240)
    ap.add_argument("--log", default=None)
    ap.add_argument("--resources-only", action="store_true")
    args = ap.parse_args()
    log = open(args.log, "w") if args.log else None
    if args.resources_only:
        say(log, "get_keys: kernel resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage)")
        # (the read unit alone, tkv_amq_read.hip, compiled for the device)
        sys.exit(0 if resource_report(log, "tkv_amq_read.hip", ("::get_keys_",), timeout=1200) else 1)
    import torch
    import turtle_kv_amd as amq
    if not torch.cuda.is_available():
        sys.exit("tools/get_keys.py needs a GPU")
    assert args.reps >= 7, "at least 7 repetitions of each route"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lim = args.step_limit
    L, F = amq.abi.lib(), amq.filters
    sh = F._stream_handle()
    say(log, "get_keys:", amq.abi.version(), "|", torch.cuda.get_device_name(0))

    counts = segment_counts(args.total_keys)
    n_leaves, nq = len(counts), args.queries
    with step_limit(lim, "tree"):
        desc, ranges = build_tree(n_leaves)
        tree = amq.TreeIndex.from_description(desc)
        d_nodes, d_segs, d_kids, d_bounds, pk = tree.device(dev)
    assert not tree.segments["flushed_pivots"].any()
    say(log, f"tree: height {int(tree.nodes[0]['height'])}, {len(tree.nodes)} nodes, {len(tree.children)} children, "
             f"{len(tree.segments)} segments, no flushed bounds")
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
        words = keys.view(torch.int64).reshape(-1, 2)
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
    cap = total + 1024
    say(log, f"{args.total_keys} keys in {n_leaves} sorted leaves; {nq} queries ({n_hits} hits); the chain's paths: "
             f"{total} entries ({total / nq:.2f} per query)")
    assert cap < 1 << 31
    path_leaf = torch.empty(cap, dtype=torch.int32, device=dev)
    path_page = torch.empty(cap, dtype=torch.int64, device=dev)
    ws = torch.empty(amq.path_probe_workspace_bytes(nq, cap), dtype=torch.uint8, device=dev)
    cand_begin = torch.empty(nq + 1, dtype=torch.int32, device=dev)
    cand_leaf = torch.empty(cap, dtype=torch.int32, device=dev)
    cand_entry = torch.empty(cap, dtype=torch.int32, device=dev)
    chain_result = torch.empty(16 * nq, dtype=torch.uint8, device=dev)
    get_result = torch.empty(16 * nq, dtype=torch.uint8, device=dev)
    visits = torch.empty(nq, dtype=torch.int32, device=dev)
    pm, gc = amq.ProbeMetrics(dev), amq.GetCounts(dev)

    for name in args.kinds.split(","):
        kind, bpk = (amq.BLOOM, 10) if name == "bloom" else (amq.VQF, 12)
        with step_limit(lim, f"{name}: build"):
            plan = amq.plan_filters(kind, counts, bpk, payload_capacity=VQF_CAP if kind else 0,
                                    src_page_ids=list(range(n_leaves)))   # the tree's page ids are the leaf numbers
            filt = amq.build_all_filters(plan, kb)
            segs = plan.device_segs(dev)
            torch.cuda.synchronize()
        opts = amq.abi.ProbeOpts(path_page.data_ptr(), None, None)

        def chain():
            walk(cap, path_leaf, path_page)
            amq.abi.check(L.tkv_amq_path_probe(
                kind, F._ptr(filt), F._ptr(segs), plan.n_segs, F._ptr(q), None, 16, nq, F._ptr(path_begin),
                F._ptr(path_leaf), cap, None, F._ptr(cand_begin), F._ptr(cand_leaf), F._ptr(cand_entry),
                ctypes.byref(opts), F._ptr(ws), ws.numel(), sh), "tkv_amq_path_probe")
            amq.abi.check(L.tkv_amq_find_keys(
                kind, F._ptr(filt), F._ptr(segs), plan.n_segs, F._ptr(q), None, 16, nq, F._ptr(cand_begin),
                F._ptr(cand_leaf), F._ptr(cand_entry), cap, F._ptr(keys), None, 16, args.total_keys, None, 0,
                F._ptr(chain_result), None, ctypes.byref(opts), None, sh), "tkv_amq_find_keys")

        def fused(d_visits=None, d_metrics=None, d_counts=None):
            amq.get_keys_device(kind, filt, segs, plan.n_segs, d_nodes, len(tree.nodes), d_segs, len(tree.segments),
                                d_kids, len(tree.children), d_bounds, len(tree.flushed_bounds), pk.data, pk.offsets,
                                pk.stride, pk.n, q, None, 16, nq, keys, None, 16, args.total_keys, None, get_result,
                                d_visits, amq.abi.GET_CHECK_PAGE_ID, d_metrics, d_counts)

        with step_limit(lim, f"{name}: check"):
            pm.reset()
            gc.reset()
            chain()
            fused(visits, pm.counts, gc.counts)
            torch.cuda.synchronize()
            rec = get_result.view(torch.int64).view(nq, 2)
            lc = get_result.view(torch.int32).view(nq, 4)
            assert torch.equal(rec[:, 0][is_hit], hit_key[is_hit]), "a hit query was not found at its own index"
            assert torch.equal(lc[:, 2][is_hit], own[is_hit]), "a hit query was found in another leaf"
            assert bool((rec[:, 0][~is_hit] == -1).all()), "a miss was found"
            crec = chain_result.view(torch.int64).view(nq, 2)
            clc = chain_result.view(torch.int32).view(nq, 4)
            assert torch.equal(rec[:, 0], crec[:, 0]) and torch.equal(lc[:, 2], clc[:, 2]), "fused != chain"
            m, c = pm.collect(), gc.collect()
            v = visits.to(torch.int64)
            n_visits = int(v.sum().item())
            n_found = int((rec[:, 0] != -1).sum().item())
            recount = {"total_filter_query_count": n_visits, "no_filter_page_count": 0, "page_id_mismatch_count": 0,
                       "filter_reject_count": n_visits - c["leaf_search_count"],
                       "filter_positive_count": c["leaf_search_count"],
                       "filter_false_positive_count": c["leaf_search_count"] - n_found}
            assert m == recount, (m, recount)
            assert c["visit_count"] == n_visits and c["found_count"] == n_found == n_hits
            assert c["flushed_count"] == 0 and c["unsearchable_count"] == 0 and c["absent_count"] == \
                c["leaf_search_count"] - n_found
            hit_visits = float(v[is_hit].sum().item()) / n_hits
            miss_visits = float(v[~is_hit].sum().item()) / (nq - n_hits)
            say(log, f"{name}: every hit found at its own index, no miss found; fused == chain in (key_index, leaf); "
                     f"metrics == the host recount {json.dumps(m)}")
            say(log, f"{name}: visits per lookup {n_visits / nq:.2f} (hits {hit_visits:.2f}, misses {miss_visits:.2f}) "
                     f"of {total / nq:.2f} path entries; {c['leaf_search_count']} leaf searches")

        with step_limit(lim, f"{name}: timing"):
            for _ in range(2):   # warm both
                chain()
                fused()
            ta, tb = [], []
            for _ in range(args.reps):   # alternate
                ta.append(timed(torch, chain))
                tb.append(timed(torch, fused))
        a, b = spread(ta), spread(tb)
        apart = b["max_ms"] < a["min_ms"] or a["max_ms"] < b["min_ms"]
        out = {"kind": name, "bits_per_key": bpk, "leaves": n_leaves, "nodes": len(tree.nodes), "queries": nq,
               "path_entries_per_query": round(total / nq, 2), "visits_per_query": round(n_visits / nq, 2),
               "visits_per_hit": round(hit_visits, 2), "visits_per_miss": round(miss_visits, 2),
               "leaf_searches": c["leaf_search_count"], "found": n_found,
               "walk_probe_find": a, "get_keys": b,
               "walk_probe_find_ms_all": [round(x, 3) for x in ta], "get_keys_ms_all": [round(x, 3) for x in tb],
               "chain_over_get_keys": round(a["median_ms"] / b["median_ms"], 3), "ranges_apart": apart,
               "get_keys_faster": bool(apart and b["median_ms"] < a["median_ms"]),
               "m_lookups_per_s_get_keys": round(nq / b["median_ms"] / 1e3, 1)}
        say(log, json.dumps(out))
        del filt
    if log:
        log.close()


if __name__ == "__main__":
    main()
