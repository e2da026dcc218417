"""Times the leaf update on one GPU: tkv_amq_merge_leaves (records), tkv_amq_gather_merged (bytes) and the
two together, beside the same jobs merged on host threads and a device-to-device copy of the output bytes.

  python tools/merge_leaves.py [--leaves 6104] [--older 16384] [--newer 1024] [--reps 7]
                               [--host-leaves 256] [--step-limit 240] [--log FILE]
  python tools/merge_leaves.py --resources-only [--log FILE]        (no GPU needed)

Workload: the bench's config 2 as leaves -- --leaves leaves of --older sorted keys with 101-byte values (1 op
byte + 100 data bytes, fixed stride) as the older side, and per leaf an update of --newer items (1/16 of the
leaf), every second one a key the leaf holds.  Three runs: 16-byte keys with the update as WRITEs (101-byte
values); 16-byte keys with the update as ADD_I32 deltas (5-byte values, folded into 5-byte WRITEs where the
key exists); 24-byte keys with WRITEs.  A key is zero bytes, then the leaf and the item's number, big-endian.
Per run, after a warm-up and a check of the counts, out_begin and a sample of the gathered items against the
construction: --reps alternating repetitions, each timed between device events, of the merge, the gather, the
two as one chain, and a copy_ of as many bytes as the gather writes (the floor of its byte mover); then
tools/merge_host.cpp, compiled on the spot, over --host-leaves of the same leaves on 16 threads (std::merge and
the compaction loop).  Every step runs under its own time limit.  Prints one JSON line per run.
--resources-only prints the compiler's resource report of the unit's kernels and exits."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from walk_paths import resource_report, say, spread, step_limit, timed  # noqa: E402

WRITE, ADD = 2, 3
VALUE_BYTES = 101


def be_keys(torch, leaf, x, key_bytes):
    """[n, key_bytes] uint8: zero bytes, then `leaf` and `x` (int64 tensors), big-endian."""
    out = torch.zeros((leaf.numel(), key_bytes), dtype=torch.uint8, device=leaf.device)
    for b in range(8):
        out[:, key_bytes - 16 + b] = (leaf >> (56 - 8 * b)) & 0xFF
        out[:, key_bytes - 8 + b] = (x >> (56 - 8 * b)) & 0xFF
    return out


def host_merge(log, leaves, older, newer, key_bytes, deltas, reps, limit):
    src = os.path.join(ROOT, "tools", "merge_host.cpp")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "merge_host")
        subprocess.run(["c++", "-O2", "-std=c++17", "-pthread", "-o", exe, src], check=True, timeout=limit)
        r = subprocess.run([exe, "--leaves", str(leaves), "--older", str(older), "--newer", str(newer), "--key",
                            str(key_bytes), "--value", str(VALUE_BYTES), "--deltas", str(int(deltas)), "--threads", "16",
                            "--reps", str(reps)], capture_output=True, text=True, timeout=limit)
    if r.returncode != 0:
        say(log, "merge_host failed:", r.stdout[-300:], r.stderr[-300:])
        return None
    return json.loads(r.stdout)


def one_run(args, log, torch, amq, dev, key_bytes, deltas):
    L, no, nn, lim = args.leaves, args.older, args.newer, args.step_limit
    name = f"k{key_bytes}_{'deltas' if deltas else 'writes'}"
    step = no // nn
    with step_limit(lim, name + ": inputs"):
        leaf_o = torch.arange(L, device=dev).repeat_interleave(no)
        older = amq.KeyBatch.fixed(be_keys(torch, leaf_o, 2 * torch.arange(no, device=dev).repeat(L), key_bytes))
        del leaf_o
        t = torch.arange(nn, device=dev).repeat(L)
        newer = amq.KeyBatch.fixed(be_keys(torch, torch.arange(L, device=dev).repeat_interleave(nn),
                                           2 * (step * t + 3) + (t & 1), key_bytes))
        ov = torch.full((L * no, VALUE_BYTES), 0x5A, dtype=torch.uint8, device=dev)
        ov[:, 0] = WRITE
        nv = torch.full((L * nn, 5 if deltas else VALUE_BYTES), 0x01, dtype=torch.uint8, device=dev)
        nv[:, 0] = ADD if deltas else WRITE
        older_v, newer_v = amq.KeyBatch.fixed(ov), amq.KeyBatch.fixed(nv)
        nb = torch.arange(L + 1, device=dev) * nn
        ob = torch.arange(L + 1, device=dev) * no
        rn, ro = amq.merge_run(newer, newer_v, nb), amq.merge_run(older, older_v, ob)
        cap = L * (no + nn)
        n_out = L * (no + nn - nn // 2)
        v_cap = amq.merge_values_bound(nv.numel(), ov.numel(), L * nn)
        ws = torch.empty(max(amq.merge_leaves_workspace_bytes(L, L * nn, L * no), amq.gather_merged_workspace_bytes(cap)),
                         dtype=torch.uint8, device=dev)
        out_begin = torch.empty(L + 1, dtype=torch.int64, device=dev)
        items = torch.empty(16 * cap, dtype=torch.uint8, device=dev)
        out_keys = torch.empty(cap * key_bytes, dtype=torch.uint8, device=dev)
        out_vals = torch.empty(v_cap, dtype=torch.uint8, device=dev)
        v_offs = torch.empty(cap + 1, dtype=torch.int64, device=dev)
        needed = torch.zeros(2, dtype=torch.int64, device=dev)
        counts = amq.MergeCounts(dev)
        torch.cuda.synchronize()

    def merge():
        amq.merge_leaves_device(rn, ro, L, out_begin, items, cap, ws, None, 0, counts.counts)

    def gather():
        amq.gather_merged_device(items, out_begin, L, cap, rn, ro, out_keys, key_bytes, None, out_keys.numel(), out_vals,
                                 v_offs, v_cap, ws, needed)

    def both():
        merge()
        gather()

    with step_limit(lim, name + ": warm-up and checks"):
        both()
        torch.cuda.synchronize()
        c = counts.collect()
        assert c == {"newer_count": L * nn, "older_count": L * no, "pair_count": L * (nn // 2),
                     "combined_count": L * (nn // 2) if deltas else 0, "bad_combine_count": 0, "dropped_count": 0,
                     "out_count": n_out}, c
        assert torch.equal(out_begin, torch.arange(L + 1, device=dev) * (no + nn - nn // 2))
        key_total, val_total = (int(x) for x in needed.cpu())
        pair_bytes = 5 if deltas else VALUE_BYTES
        assert key_total == n_out * key_bytes
        assert val_total == L * (no - nn // 2) * VALUE_BYTES + L * (nn // 2) * (pair_bytes + nv.shape[1])
        # the head of leaf 0: older items 0..2 (keys 0, 2, 4), then the update's first item over older item 3
        # (key 6), older item 4 (key 8), ...; keys ascend strictly over the whole sample
        ks = out_keys[:4096 * key_bytes].view(-1, key_bytes)[:, key_bytes - 8:].cpu().numpy()
        nums = [int.from_bytes(bytes(r), "big") for r in ks]
        assert nums[:5] == [0, 2, 4, 6, 8] and all(a < b for a, b in zip(nums, nums[1:]))
        offs = v_offs[:6].cpu().tolist()
        assert [b - a for a, b in zip(offs, offs[1:])] == [VALUE_BYTES] * 3 + [pair_bytes, VALUE_BYTES]
        assert int(out_vals[offs[3]]) == WRITE and int(out_vals[offs[2]]) == WRITE
    copy_src = torch.empty(key_total + val_total, dtype=torch.uint8, device=dev)
    copy_dst = torch.empty_like(copy_src)
    t = {"merge": [], "gather": [], "both": [], "copy": []}
    with step_limit(lim, name + ": timing"):
        for _ in range(args.reps):                                # alternating
            t["merge"].append(timed(torch, merge))
            t["gather"].append(timed(torch, gather))
            t["both"].append(timed(torch, both))
            t["copy"].append(timed(torch, lambda: copy_dst.copy_(copy_src)))
    n_in = L * (no + nn)
    in_bytes = older.data.numel() + newer.data.numel() + ov.numel() + nv.numel()
    res = {"run": name, "leaves": L, "items_in": n_in, "items_out": n_out, "out_key_bytes": key_total,
           "out_value_bytes": val_total,
           # what the gather reads and writes per input item: a record, the source and the destination bytes, offsets
           "gather_bytes_per_item": round((16 * n_out + 2 * (key_total + val_total) + 8 * n_out) / n_in, 1),
           # what the merge reads and writes per input item: keys (searched, not streamed), op bytes, two words of
           # workspace written and read, a record
           "merge_bytes_per_item_streamed": round((older.data.numel() + newer.data.numel() + 16 * n_in + 16 * n_out) / n_in, 1),
           "input_bytes": in_bytes}
    for k, v in t.items():
        res[k] = spread(v)
    for k in ("merge", "gather", "both"):
        res[k]["gitems_per_s"] = round(n_in / res[k]["median_ms"] / 1e6, 2)
    res["gather"]["gbytes_per_s_out"] = round((key_total + val_total) / res["gather"]["median_ms"] / 1e6, 1)
    res["copy"]["gbytes_per_s"] = round((key_total + val_total) / res["copy"]["median_ms"] / 1e6, 1)
    res["gather_over_copy"] = round(res["gather"]["median_ms"] / res["copy"]["median_ms"], 2)
    res["merge_over_gather"] = round(res["merge"]["median_ms"] / res["gather"]["median_ms"], 2)
    del copy_src, copy_dst, items, out_keys, out_vals, ws, ov, nv
    torch.cuda.empty_cache()
    with step_limit(lim, name + ": host merge"):
        host = host_merge(log, min(args.host_leaves, L), no, nn, key_bytes, deltas, args.reps, lim)
    if host:
        res["host"] = host
        res["both_over_host"] = round(res["both"]["gitems_per_s"] / host["gitems_per_s"], 1)
    say(log, json.dumps(res))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leaves", type=int, default=6104)
    ap.add_argument("--older", type=int, default=16384)
    ap.add_argument("--newer", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-leaves", type=int, default=256)
    ap.add_argument("--step-limit", type=int, default=240)
    ap.add_argument("--log", default=None)
    ap.add_argument("--resources-only", action="store_true")
    args = ap.parse_args()
    log = open(args.log, "w") if args.log else None
    if args.resources_only:
        say(log, "merge_leaves: kernel resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage)")
        sys.exit(0 if resource_report(log, "tkv_amq_merge.hip") else 1)
    import torch
    import turtle_kv_amd as amq
    if not torch.cuda.is_available():
        sys.exit("tools/merge_leaves.py needs a GPU")
    assert args.reps >= 7, "at least 7 repetitions"
    assert args.older % args.newer == 0 and args.older // args.newer >= 4 and args.newer % 2 == 0
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    say(log, "merge_leaves:", amq.abi.version(), "|", torch.cuda.get_device_name(0))
    say(log, f"workload: {args.leaves} leaves x ({args.older} older + {args.newer} newer items), {VALUE_BYTES}-byte values, "
             f"every second update key in its leaf; {args.reps} alternating repetitions")
    for key_bytes, deltas in ((16, False), (16, True), (24, False)):
        one_run(args, log, torch, amq, dev, key_bytes, deltas)


if __name__ == "__main__":
    main()
