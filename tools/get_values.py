"""Times the point lookup with values (tkv_amq_get_values) and the gather behind it (tkv_amq_gather_values)
on one GPU, beside tkv_amq_get_keys.

  python tools/get_values.py [--total-keys 100000000] [--queries 25000000] [--reps 7]
                             [--kinds bloom,vqf] [--step-limit 240] [--log FILE]
  python tools/get_values.py --resources-only [--log FILE]        (no GPU needed)

Setup: tools/get_keys.py's, by import of the same pieces -- --total-keys 16-byte keys in 16,384-key
sorted leaves (6,104 at 100M, the bench's config 2 count: 4,096 bottom leaves and 2,008 in the update
buffers) under tools/walk_paths.py's tree of height 3 (161 nodes, no flushed bounds), Bloom at 10
bits/key and VQF at 12, --queries lookups, half hits and half seed-43 misses, shuffled.  Every key
sits in one leaf only.

Three measurements per kind, each timed between device events in one process after a warm-up, 7
repetitions, median and min-max:
  1. all values WRITE (1 op byte + 4 data bytes, fixed stride): tkv_amq_get_values alternated with
     tkv_amq_get_keys (results only, page ids checked).  Checked first: key_index, leaf, where, the
     visits, the metrics and the six shared counts are equal, every found value is a WRITE.
  2. with deltas: the update buffers' items are ADD_I32, the bottom leaves' WRITE, so a hit in a
     buffer goes on to the bottom.  Checked first on a sample: every record and visit count equals a
     host mirror's -- the fold of include/tkv_amq.h, in Python, over the sample's paths as
     tkv_amq_walk_paths lists them (a leaf holds the query's key iff it is the key's own leaf).
  3. the gather over the results of (1) with 101-byte values (1 op byte + 100 data bytes) into
     128-byte slots, beside a device-to-device copy of as many bytes as the gather writes.  Checked
     first on a sample: lengths and bytes.
Every step runs under its own time limit.  Prints one JSON line per kind.  --resources-only prints
the compiler's resource report of the get_keys, get_values and gather kernels and exits."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench import SEG_KEYS, segment_counts, sort_segments_device, splitmix_keys16  # noqa: E402
from walk_paths import (N_BOTTOM, VQF_CAP, build_tree, gen_keys, resource_report, say, spread, step_limit,  # noqa: E402
                        timed)

DELETE, NOOP, WRITE, ADD = 0, 1, 2, 3
COMBINED, BAD_COMBINE = 1, 2
LEAF_LEVEL = 0xFF
SAMPLE = 4096
DATA_BYTES, OUT_STRIDE = 100, 128


def mirror(entries, own, value):
    """The fold of include/tkv_amq.h over one query's path: entries [(leaf, where)] in order, `own` the
    one leaf that holds the key (or None), value = (op, integer) of the key's item there.  Returns (op,
    flags, i32, n_items, leaf, where, visits); the filters cannot change any of these."""
    op, flags, acc, n_items, leaf_at, where_at, visits, left = 0xFF, 0, 0, 0, -1, -1, 0, None
    for leaf, where in entries:
        if where == left:
            continue
        visits += 1
        if leaf != own:
            continue
        n_items += 1
        if n_items == 1:
            op, leaf_at, where_at = value[0], leaf, where
            if op != ADD:
                break
            acc, left = value[1], where
        elif value[0] == WRITE:
            op, acc, flags = WRITE, (acc + value[1]) & 0xFFFFFFFF, flags | COMBINED
            break
        else:                                                    # (one leaf per key: not reached on this tree)
            raise AssertionError("a key in two leaves")
    return op, flags, acc, n_items, leaf_at, where_at, visits


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
        say(log, "get_values: kernel resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage)")
        # (the read unit alone, tkv_amq_read.hip, compiled for the device)
        sys.exit(0 if resource_report(log, "tkv_amq_read.hip", ("::get_keys_", "::get_values_", "::gather_values_"),
                                      timeout=1200) else 1)
    import numpy as np
    import torch
    import turtle_kv_amd as amq
    if not torch.cuda.is_available():
        sys.exit("tools/get_values.py needs a GPU")
    assert args.reps >= 7, "at least 7 repetitions of each route"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lim = args.step_limit
    say(log, "get_values:", amq.abi.version(), "|", torch.cuda.get_device_name(0))

    counts = segment_counts(args.total_keys)
    n_leaves, nq, n_keys = len(counts), args.queries, args.total_keys
    with step_limit(lim, "tree"):
        desc, ranges = build_tree(n_leaves)
        tree = amq.TreeIndex.from_description(desc)
        d_nodes, d_segs, d_kids, d_bounds, pk = tree.device(dev)
    assert not tree.segments["flushed_pivots"].any()
    say(log, f"tree: height {int(tree.nodes[0]['height'])}, {len(tree.nodes)} nodes, {len(tree.children)} children, "
             f"{len(tree.segments)} segments ({n_leaves - N_BOTTOM} update-buffer leaves over {N_BOTTOM} bottom leaves)")
    with step_limit(lim, "keys, sorted per leaf"):
        keys = sort_segments_device(torch, gen_keys(torch, n_keys, ranges, dev), counts)
        kb = amq.KeyBatch.fixed(keys)
        torch.cuda.synchronize()
    with step_limit(lim, "queries"):
        g = torch.Generator(device=dev)
        g.manual_seed(44)
        perm = torch.randperm(nq, device=dev, generator=g)
        is_hit = perm < nq // 2
        hit_key = torch.randint(0, n_keys, (nq,), device=dev, generator=g)
        words = keys.view(torch.int64).reshape(-1, 2)
        miss = splitmix_keys16(torch, 43, perm).contiguous().view(torch.int64).reshape(-1, 2)
        q = torch.where(is_hit[:, None], words[hit_key], miss).contiguous().view(torch.uint8).reshape(nq, 16)
        del miss, perm
        n_hits = int(is_hit.sum())
        torch.cuda.synchronize()
    with step_limit(lim, "values"):
        # item i's integer: i modulo 2^31; (1) every op WRITE, (2) the update buffers' items ADD_I32
        idx = torch.arange(n_keys, dtype=torch.int64, device=dev)
        v_write = torch.empty((n_keys, 5), dtype=torch.uint8, device=dev)
        v_write[:, 0] = WRITE
        v_write[:, 1:] = (idx & 0x7FFFFFFF).to(torch.int32).view(torch.uint8).view(n_keys, 4)
        v_delta = v_write.clone()
        v_delta[N_BOTTOM * SEG_KEYS:, 0] = ADD
        # (3) 101 bytes per item: data byte j of item i is (i + j) modulo 256
        v_wide = torch.empty((n_keys, 1 + DATA_BYTES), dtype=torch.uint8, device=dev)
        v_wide[:, 0] = WRITE
        col = torch.arange(DATA_BYTES, dtype=torch.int64, device=dev)
        for b in range(0, n_keys, 1 << 22):
            e = min(b + (1 << 22), n_keys)
            v_wide[b:e, 1:] = ((idx[b:e, None] + col[None, :]) & 0xFF).to(torch.uint8)
        del idx
        torch.cuda.synchronize()
    say(log, f"{n_keys} keys in {n_leaves} sorted leaves; {nq} queries ({n_hits} hits); values: 5 bytes each "
             f"({v_write.numel() / 1e6:.0f} MB), 101 bytes each for the gather ({v_wide.numel() / 1e9:.1f} GB)")

    keys_result = torch.empty(16 * nq, dtype=torch.uint8, device=dev)
    result = torch.empty(32 * nq, dtype=torch.uint8, device=dev)
    visits_k = torch.empty(nq, dtype=torch.int32, device=dev)
    visits_v = torch.empty(nq, dtype=torch.int32, device=dev)
    slots = torch.empty(nq * OUT_STRIDE, dtype=torch.uint8, device=dev)
    lengths = torch.empty(nq, dtype=torch.int32, device=dev)
    pm_k, pm_v, gc, vc = amq.ProbeMetrics(dev), amq.ProbeMetrics(dev), amq.GetCounts(dev), amq.ValueCounts(dev)
    # the sample's paths, for the host mirror
    with step_limit(lim, "sample paths"):
        pick = torch.arange(0, nq, max(nq // SAMPLE, 1), device=dev)[:SAMPLE]
        walk = amq.walk_paths(tree, amq.KeyBatch.fixed(q[pick].contiguous()), want_where=True)
        torch.cuda.synchronize()
        p_begin = walk.path_begin.cpu().numpy()
        p_leaf = walk.path_leaf.cpu().numpy().view(np.uint32)
        p_where = walk.path_where.cpu().numpy().view(np.uint16)
        s_hit, s_key = is_hit[pick].cpu().numpy(), hit_key[pick].cpu().numpy()
        pick_h = pick.cpu().numpy()

    for name in args.kinds.split(","):
        kind, bpk = (amq.BLOOM, 10) if name == "bloom" else (amq.VQF, 12)
        with step_limit(lim, f"{name}: build"):
            plan = amq.plan_filters(kind, counts, bpk, payload_capacity=VQF_CAP if kind else 0,
                                    src_page_ids=list(range(n_leaves)))   # the tree's page ids are the leaf numbers
            filt = amq.build_all_filters(plan, kb)
            segs = plan.device_segs(dev)
            torch.cuda.synchronize()

        def get_keys(d_visits=None, d_metrics=None, d_counts=None):
            amq.get_keys_device(kind, filt, segs, plan.n_segs, d_nodes, len(tree.nodes), d_segs, len(tree.segments),
                                d_kids, len(tree.children), d_bounds, len(tree.flushed_bounds), pk.data, pk.offsets,
                                pk.stride, pk.n, q, None, 16, nq, keys, None, 16, n_keys, None, keys_result,
                                d_visits, amq.abi.GET_CHECK_PAGE_ID, d_metrics, d_counts)

        def get_values(values, d_visits=None, d_metrics=None, d_counts=None):
            amq.get_values_device(kind, filt, segs, plan.n_segs, d_nodes, len(tree.nodes), d_segs, len(tree.segments),
                                  d_kids, len(tree.children), d_bounds, len(tree.flushed_bounds), pk.data, pk.offsets,
                                  pk.stride, pk.n, q, None, 16, nq, keys, None, 16, n_keys, None, values, None,
                                  values.shape[1], values.numel(), result, d_visits, amq.abi.GET_CHECK_PAGE_ID,
                                  d_metrics, d_counts)

        def gather():
            amq.gather_values_device(result, nq, v_wide, None, 1 + DATA_BYTES, v_wide.numel(), n_keys, slots,
                                     OUT_STRIDE, lengths)

        rec64 = result.view(torch.int64).view(nq, 4)
        rec32 = result.view(torch.int32).view(nq, 8)
        # ---- (1) all values WRITE, against get_keys ----
        with step_limit(lim, f"{name}: check, all WRITE"):
            for c in (pm_k, pm_v, gc, vc):
                c.reset()
            get_keys(visits_k, pm_k.counts, gc.counts)
            get_values(v_write, visits_v, pm_v.counts, vc.counts)
            torch.cuda.synchronize()
            krec = keys_result.view(torch.int64).view(nq, 2)
            klc = keys_result.view(torch.int32).view(nq, 4)
            assert torch.equal(rec64[:, 0], krec[:, 0]) and torch.equal(rec64[:, 1], krec[:, 0]), "key_index differs"
            assert torch.equal(rec32[:, 4], klc[:, 2]) and torch.equal(rec32[:, 5], klc[:, 3]), "leaf or where differs"
            assert torch.equal(visits_v, visits_k), "visits differ"
            found = krec[:, 0] != -1
            assert torch.equal(found, is_hit) and torch.equal(krec[:, 0][is_hit], hit_key[is_hit])
            want_meta = torch.where(found, WRITE | 1 << 16, 0xFF).to(torch.int32)
            assert torch.equal(rec32[:, 7], want_meta) and not bool(rec32[:, 6].any()), "op, flags, n_items or i32"
            mk, mv, ck, cv = pm_k.collect(), pm_v.collect(), gc.collect(), vc.collect()
            assert mk == mv, (mk, mv)
            assert all(cv[n] == ck[n] for n in ck) and cv["item_count"] == ck["found_count"] == n_hits
            assert cv["bad_combine_count"] == 0
            visits_write = int(visits_v.to(torch.int64).sum().item())
            say(log, f"{name}: all WRITE: records, visits, metrics and the six shared counts equal get_keys'; "
                     f"{visits_write / nq:.2f} visits per lookup; {json.dumps(cv)}")
        with step_limit(lim, f"{name}: timing, all WRITE"):
            for _ in range(2):   # warm both
                get_keys()
                get_values(v_write)
            ta, tb = [], []
            for _ in range(args.reps):   # alternate
                ta.append(timed(torch, get_keys))
                tb.append(timed(torch, lambda: get_values(v_write)))
        a, b = spread(ta), spread(tb)
        apart = b["max_ms"] < a["min_ms"] or a["max_ms"] < b["min_ms"]

        # ---- (3) the gather over (1)'s results (they are still in `result`) ----
        with step_limit(lim, f"{name}: check, gather"):
            get_values(v_write)
            slots.fill_(0xEE)
            gather()
            torch.cuda.synchronize()
            assert torch.equal(lengths, torch.where(is_hit, DATA_BYTES, 0).to(torch.int32)), "lengths"
            sl = slots.view(nq, OUT_STRIDE)[pick].cpu().numpy()
            for j in range(len(pick_h)):
                if s_hit[j]:
                    want = (int(s_key[j]) + np.arange(DATA_BYTES)) & 0xFF
                    assert (sl[j, :DATA_BYTES] == want).all() and (sl[j, DATA_BYTES:] == 0xEE).all(), "a gathered value"
                else:
                    assert (sl[j] == 0xEE).all(), "bytes written for a miss"
            out_bytes = n_hits * DATA_BYTES
            say(log, f"{name}: gather: lengths exact, {len(pick_h)} sampled slots exact; {out_bytes / 1e9:.2f} GB of values")
        with step_limit(lim, f"{name}: timing, gather"):
            src = torch.empty(out_bytes, dtype=torch.uint8, device=dev)
            dst = torch.empty(out_bytes, dtype=torch.uint8, device=dev)
            for _ in range(2):
                gather()
                dst.copy_(src)
            tg, tc = [], []
            for _ in range(args.reps):
                tg.append(timed(torch, gather))
                tc.append(timed(torch, lambda: dst.copy_(src)))
            del src, dst
        gsp, csp = spread(tg), spread(tc)

        # ---- (2) with deltas ----
        with step_limit(lim, f"{name}: check, deltas"):
            pm_v.reset()
            vc.reset()
            get_values(v_delta, visits_v, pm_v.counts, vc.counts)
            torch.cuda.synchronize()
            got = result.view(nq, 32)[pick].cpu().numpy().view(amq.abi.VALUE_RESULT_DTYPE).reshape(-1)
            got_visits = visits_v[pick].cpu().numpy()
            for j in range(len(pick_h)):
                entries = [(int(p_leaf[e]), int(p_where[e])) for e in range(int(p_begin[j]), int(p_begin[j + 1]))]
                own = int(s_key[j]) // SEG_KEYS if s_hit[j] else None
                value = (ADD if own is not None and own >= N_BOTTOM else WRITE, int(s_key[j]) & 0x7FFFFFFF)
                op, flags, acc, n_items, leaf_at, where_at, n_vis = mirror(entries, own, value)
                r = got[j]
                want_key = int(s_key[j]) if n_items else (1 << 64) - 1
                assert (int(r["op"]), int(r["flags"]), int(r["i32"]) & 0xFFFFFFFF, int(r["n_items"])) == \
                    (op, flags, acc, n_items), ("record", j)
                assert (int(r["key_index"]), int(r["last_index"])) == (want_key, want_key), ("index", j)
                assert (int(r["leaf"]), int(r["where"])) == (leaf_at & 0xFFFFFFFF, where_at & 0xFFFFFFFF), ("place", j)
                assert int(got_visits[j]) == n_vis, ("visits", j)
            cd = vc.collect()
            visits_delta = int(visits_v.to(torch.int64).sum().item())
            n_pending = int(((rec32[:, 7] & 0xFF) == ADD).sum().item())
            assert cd["found_count"] == n_hits and cd["bad_combine_count"] == 0
            say(log, f"{name}: deltas: {len(pick_h)} sampled records and visit counts equal the host mirror's; "
                     f"{visits_delta / nq:.2f} visits per lookup ({visits_write / nq:.2f} with all WRITE), "
                     f"{cd['item_count'] / max(cd['found_count'], 1):.3f} items per found query, {n_pending} end pending; "
                     f"{json.dumps(cd)}")
        with step_limit(lim, f"{name}: timing, deltas"):
            for _ in range(2):
                get_values(v_delta)
            td = [timed(torch, lambda: get_values(v_delta)) for _ in range(args.reps)]
        dsp = spread(td)

        out = {"kind": name, "bits_per_key": bpk, "leaves": n_leaves, "nodes": len(tree.nodes), "queries": nq,
               "found": n_hits, "visits_per_query_all_write": round(visits_write / nq, 2),
               "get_keys": a, "get_values_all_write": b,
               "get_keys_ms_all": [round(x, 3) for x in ta], "get_values_all_write_ms_all": [round(x, 3) for x in tb],
               "get_values_over_get_keys": round(b["median_ms"] / a["median_ms"], 3), "ranges_apart": apart,
               "m_lookups_per_s_get_values": round(nq / b["median_ms"] / 1e3, 1),
               "get_values_deltas": dsp, "get_values_deltas_ms_all": [round(x, 3) for x in td],
               "visits_per_query_deltas": round(visits_delta / nq, 2),
               "items_per_found_query_deltas": round(cd["item_count"] / max(cd["found_count"], 1), 3),
               "pending_deltas": n_pending,
               "gather": gsp, "gather_ms_all": [round(x, 3) for x in tg], "gather_value_bytes": out_bytes,
               "gather_gb_per_s": round(out_bytes / gsp["median_ms"] / 1e6, 1),
               "copy_same_bytes": csp, "copy_ms_all": [round(x, 3) for x in tc],
               "copy_gb_per_s": round(out_bytes / csp["median_ms"] / 1e6, 1),
               "gather_over_copy": round(gsp["median_ms"] / csp["median_ms"], 2)}
        say(log, json.dumps(out))
        del filt
    if log:
        log.close()


if __name__ == "__main__":
    main()
