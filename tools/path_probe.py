"""Times the path probe against the composed route it replaces, on one GPU.

  python tools/path_probe.py [--total-keys 100000000] [--queries 25000000] [--path-len 8]
                             [--reps 7] [--kinds bloom,vqf] [--log FILE]

Setup: the bench's filter set (--total-keys 16-byte keys in 16,384-key leaves: 6,104 leaves at
100M; Bloom at 10 bits/key, VQF at 12), --queries lookups, half hits and half seed-43 misses,
shuffled, each with a path of --path-len leaves: one random leaf per "level", a hit's own leaf
at a random position.  25M x 8 = 200M entries, the count of the probe workloads.

Timed, with device events, alternating in one process after both are warm:
  (a) tkv_amq_path_probe (keys + CSR lists -> compacted candidates);
  (b) the composed route over pre-expanded pair arrays: tkv_amq_vqf_hash +
      tkv_amq_vqf_probe_hashed (or the Bloom pair), then the compaction a caller would write:
      mask -> nonzero -> gather;
  (c) the pair expansion alone (reported, not charged to (b)).
Before timing it asserts that (a)'s entry answers equal (b)'s pair results and (a)'s candidates
equal (b)'s compacted list.  Prints one JSON line per kind.  Needs a GPU; fails without one."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import SEG_KEYS, segment_counts, splitmix_keys16  # noqa: E402

VQF_CAP = 32704


def say(log, *a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    if log:
        log.write(line + "\n")
        log.flush()


def timed(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def spread(v):
    return {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3),
            "max_ms": round(max(v), 3), "reps": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--total-keys", type=int, default=100_000_000)
    ap.add_argument("--queries", type=int, default=25_000_000)
    ap.add_argument("--path-len", type=int, default=8)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--kinds", default="bloom,vqf")
    ap.add_argument("--log", default=None)
    args = ap.parse_args()
    import torch
    import turtle_kv_amd as amq
    if not torch.cuda.is_available():
        sys.exit("tools/path_probe.py needs a GPU")
    assert args.reps >= 7, "at least 7 repetitions of each route"
    log = open(args.log, "w") if args.log else None
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    L, F = amq.abi.lib(), amq.filters
    sh = F._stream_handle()
    say(log, "path_probe:", amq.abi.version(), "|", torch.cuda.get_device_name(0))

    counts = segment_counts(args.total_keys)
    n_leaves, nq, plen = len(counts), args.queries, args.path_len
    n_entries = nq * plen
    assert n_entries < 1 << 31
    keys = amq.gen_keys16(42, 0, args.total_keys, device=dev)
    kb = amq.KeyBatch.fixed(keys)

    # queries: half hits (random built keys), half seed-43 misses, shuffled; generated in place
    g = torch.Generator(device=dev)
    g.manual_seed(44)
    perm = torch.randperm(nq, device=dev, generator=g)
    is_hit = perm < nq // 2
    hit_key = torch.randint(0, args.total_keys, (nq,), device=dev, generator=g)
    gi = torch.where(is_hit, hit_key, perm)
    q = splitmix_keys16(torch, torch.where(is_hit, 42, 43).to(torch.int64), gi).contiguous()
    qb = amq.KeyBatch.fixed(q)
    own = (hit_key // SEG_KEYS).to(torch.int32)
    leaves = torch.randint(0, n_leaves, (nq, plen), device=dev, dtype=torch.int32, generator=g)
    pos = torch.randint(0, plen, (nq,), device=dev, generator=g)
    rows = torch.arange(nq, device=dev)
    at_pos = (torch.arange(plen, device=dev)[None, :] == pos[:, None]) & is_hit[:, None]
    path_leaf = torch.where(at_pos, own[:, None], leaves).reshape(-1).contiguous()
    del at_pos
    path_begin = (torch.arange(nq + 1, device=dev, dtype=torch.int64) * plen).to(torch.int32)
    own_entry = (rows * plen + pos)[is_hit]
    del perm, gi, leaves
    say(log, f"{args.total_keys} keys in {n_leaves} leaves; {nq} queries ({int(is_hit.sum())} hits) x "
             f"{plen} leaves = {n_entries} entries")

    # (c) the pair expansion a caller of the composed route does first
    def expand():
        pq = torch.repeat_interleave(torch.arange(nq, device=dev, dtype=torch.int32), plen)
        return pq, path_leaf.clone()
    expand()
    t_expand = [timed(torch, expand)[0] for _ in range(args.reps)]
    pair_query, pair_leaf = expand()

    ws = torch.empty(amq.path_probe_workspace_bytes(nq, n_entries), dtype=torch.uint8, device=dev)
    cand_begin = torch.empty(nq + 1, dtype=torch.int32, device=dev)
    cand_leaf = torch.empty(n_entries, dtype=torch.int32, device=dev)
    cand_entry = torch.empty(n_entries, dtype=torch.int32, device=dev)
    entry_result = torch.empty(n_entries, dtype=torch.uint8, device=dev)
    pair_result = torch.empty(n_entries, dtype=torch.uint8, device=dev)

    for name in args.kinds.split(","):
        kind, bpk = (amq.BLOOM, 10) if name == "bloom" else (amq.VQF, 12)
        plan = amq.plan_filters(kind, counts, bpk, payload_capacity=VQF_CAP if kind else 0)
        filt = amq.build_all_filters(plan, kb)
        segs = plan.device_segs(dev)
        k_max = int(plan.segs["hash_count"].max()) if kind == amq.BLOOM else 0
        hashes = (torch.empty(nq, dtype=torch.int64, device=dev) if kind else
                  torch.empty(nq * int(L.tkv_amq_bloom_query_stride(k_max)), dtype=torch.uint8, device=dev))

        def path_route(er=None, ce=None):
            amq.abi.check(L.tkv_amq_path_probe(
                kind, F._ptr(filt), F._ptr(segs), plan.n_segs, F._ptr(q), None, 16, nq, F._ptr(path_begin),
                F._ptr(path_leaf), n_entries, F._ptr(er), F._ptr(cand_begin), F._ptr(cand_leaf), F._ptr(ce),
                None, F._ptr(ws), ws.numel(), sh), "tkv_amq_path_probe")

        def composed_route():
            if kind:
                amq.abi.check(L.tkv_amq_vqf_hash(F._ptr(q), None, 16, nq, F._ptr(hashes), sh), "vqf_hash")
                amq.abi.check(L.tkv_amq_vqf_probe_hashed(
                    F._ptr(filt), F._ptr(segs), plan.n_segs, F._ptr(hashes), F._ptr(pair_query), n_entries,
                    F._ptr(pair_leaf), F._ptr(pair_result), sh), "vqf_probe_hashed")
            else:
                amq.abi.check(L.tkv_amq_bloom_hash(F._ptr(q), None, 16, nq, k_max, F._ptr(hashes), sh),
                              "bloom_hash")
                amq.abi.check(L.tkv_amq_bloom_probe_hashed(
                    F._ptr(filt), F._ptr(segs), plan.n_segs, F._ptr(hashes), k_max, F._ptr(pair_query),
                    n_entries, F._ptr(pair_leaf), F._ptr(pair_result), sh), "bloom_probe_hashed")
            idx = torch.nonzero(pair_result.view(torch.bool)).squeeze(1)   # mask -> nonzero
            return idx, torch.index_select(pair_leaf, 0, idx)             # -> gather

        # correctness first: the same answers and the same candidates
        path_route(entry_result, cand_entry)
        idx, leaf_b = composed_route()
        torch.cuda.synchronize()
        total = int(cand_begin[-1].item())
        assert torch.equal(entry_result, pair_result), "entry answers differ from the pair probe"
        assert total == idx.numel(), (total, idx.numel())
        assert torch.equal(cand_entry[:total].to(torch.int64), idx), "candidate entries differ"
        assert torch.equal(cand_leaf[:total], leaf_b), "candidate leaves differ"
        per_query = torch.bincount(idx // plen, minlength=nq)
        assert torch.equal(cand_begin[1:].to(torch.int64), torch.cumsum(per_query, 0)) and int(cand_begin[0]) == 0
        assert bool(entry_result[own_entry].all()), "a hit's own leaf was rejected"
        say(log, f"{name}: answers and candidates equal; {total} candidates of {n_entries} entries "
                 f"({int(is_hit.sum())} own leaves)")

        for _ in range(2):   # warm both
            path_route()
            composed_route()
        ta, tb = [], []
        for _ in range(args.reps):   # alternate
            ta.append(timed(torch, path_route)[0])
            tb.append(timed(torch, composed_route)[0])
        a, b = spread(ta), spread(tb)
        win = b["median_ms"] - a["median_ms"]
        b_spread = b["max_ms"] - b["min_ms"]
        verdict = ("path probe slower" if win < 0 else
                   "tie (win within the composed route's spread)" if win <= b_spread else "path probe faster")
        say(log, json.dumps({
            "kind": name, "bits_per_key": bpk, "entries": n_entries, "queries": nq, "candidates": total,
            "path_probe": {**a, "g_entries_per_s": round(n_entries / a["median_ms"] / 1e6, 2)},
            "composed": {**b, "g_entries_per_s": round(n_entries / b["median_ms"] / 1e6, 2)},
            "pair_expansion": spread(t_expand),
            "path_probe_ms_all": [round(x, 3) for x in ta], "composed_ms_all": [round(x, 3) for x in tb],
            "speedup": round(b["median_ms"] / a["median_ms"], 3), "a_le_b": a["median_ms"] <= b["median_ms"],
            "verdict": verdict}))
        del filt, hashes
    if log:
        log.close()


if __name__ == "__main__":
    main()
