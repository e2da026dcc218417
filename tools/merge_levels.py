"""Times the K-way merge on one GPU: tkv_amq_merge_levels (records), tkv_amq_gather_levels (bytes) and the
two together, beside the same levels merged pairwise, newest first, by K - 1 rounds of tkv_amq_merge_leaves +
tkv_amq_gather_merged (what a caller paid before the K-way call: every round re-materialises its output so
that it can be the next round's newer run).

  python tools/merge_levels.py [--jobs 6104] [--sizes 1024,2048,4096,16384] [--reps 7] [--step-limit 240] [--log FILE]
  python tools/merge_levels.py --resources-only [--log FILE]        (no GPU needed)

Workload: DESIGN.md section 18's, extended to four levels -- --jobs jobs, 16-byte keys, per job runs of --sizes
items, the newest first, each a multiple of its newer neighbour (powers of two); every second key of a run is
also in the next older run (and so in every older one).  Two runs: every level 101-byte WRITE values in the fixed form; then the
levels above the oldest as 5-byte ADD_I32 deltas, which fold through every level below them.  A key is zero
bytes, then the job and the item's number, big-endian.  Per run, after a warm-up: the counts, out_begin, the byte
totals and the head of the output are checked against the construction, and the chain's final keys, values and
offsets must equal the K-way call's byte for byte; then --reps alternating repetitions, each timed between device
events, of the merge, the gather, the two as one chain of launches, and the pairwise chain.  Every step runs
under its own time limit.  Prints one JSON line per run.
--resources-only prints the compiler's resource report of the unit's kernels and exits."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from merge_leaves import be_keys  # noqa: E402
from walk_paths import resource_report, say, spread, step_limit, timed  # noqa: E402

WRITE, ADD = 2, 3
VALUE_BYTES = 101


def level_numbers(torch, dev, sizes, s):
    """The numbers of level s's keys within a job, ascending: every second one is in level s + 1 too.  The oldest
    level holds the multiples of 2^K; level s item t is t * step (in every older level) for even t, and
    t * step + 2^s (in no other level) for odd t, with step = 2^K * (the oldest level's size / this level's)."""
    k = len(sizes)
    t = torch.arange(sizes[s], device=dev)
    step = (1 << k) * (sizes[-1] // sizes[s])
    return t * step if s == k - 1 else t * step + (t & 1) * (1 << s)


def shadowed(sizes, s):
    """Items of level s (per job) that a newer level holds: those of level s - 1's even items."""
    return 0 if s == 0 else sizes[s - 1] // 2


class Chain:
    """The pairwise route over preallocated buffers: round r merges (the output of round r - 1, or level 0) over
    level r + 1 and gathers the result."""

    def __init__(self, torch, amq, dev, L, levels, begins, sizes):
        self.amq, self.L, self.rounds = amq, L, []
        newer_k, newer_v, newer_b, n_newer, newer_bytes = levels[0][0], levels[0][1], begins[0], L * sizes[0], None
        for r in range(1, len(sizes)):
            older_k, older_v = levels[r]
            n_older = L * sizes[r]
            cap = n_newer + n_older
            nv_bytes = int(newer_v.data.numel()) if newer_bytes is None else newer_bytes
            v_cap = amq.merge_values_bound(nv_bytes, int(older_v.data.numel()), n_newer)
            buf = {"ws": torch.empty(max(amq.merge_leaves_workspace_bytes(L, n_newer, n_older),
                                         amq.gather_merged_workspace_bytes(cap)), dtype=torch.uint8, device=dev),
                   "begin": torch.empty(L + 1, dtype=torch.int64, device=dev),
                   "items": torch.empty(16 * cap, dtype=torch.uint8, device=dev),
                   "keys": torch.empty((cap, 16), dtype=torch.uint8, device=dev),
                   "vals": torch.empty(v_cap, dtype=torch.uint8, device=dev),
                   "voffs": torch.empty(cap + 1, dtype=torch.int64, device=dev), "cap": cap, "v_cap": v_cap,
                   "rn": amq.merge_run(newer_k, newer_v, newer_b), "ro": amq.merge_run(older_k, older_v, begins[r])}
            self.rounds.append(buf)
            # (the next round's newer run: this round's output, all `cap` slots of it addressable)
            newer_k = amq.KeyBatch.fixed(buf["keys"])
            newer_v = amq.KeyBatch.variable(buf["vals"], buf["voffs"])
            newer_b, n_newer, newer_bytes = buf["begin"], cap, v_cap

    def run(self):
        amq, L = self.amq, self.L
        for b in self.rounds:
            amq.merge_leaves_device(b["rn"], b["ro"], L, b["begin"], b["items"], b["cap"], b["ws"])
            amq.gather_merged_device(b["items"], b["begin"], L, b["cap"], b["rn"], b["ro"], b["keys"], 16, None,
                                     16 * b["cap"], b["vals"], b["voffs"], b["v_cap"], b["ws"])


def one_run(args, log, torch, amq, dev, sizes, deltas):
    L, lim, K = args.jobs, args.step_limit, len(sizes)
    name = f"k16_{K}levels_{'deltas' if deltas else 'writes'}"
    with step_limit(lim, name + ": inputs"):
        levels, begins = [], []
        for s, n in enumerate(sizes):
            job = torch.arange(L, device=dev).repeat_interleave(n)
            keys = amq.KeyBatch.fixed(be_keys(torch, job, level_numbers(torch, dev, sizes, s).repeat(L), 16))
            del job
            delta = deltas and s < K - 1
            v = torch.full((L * n, 5 if delta else VALUE_BYTES), 0x01 if delta else 0x5A, dtype=torch.uint8, device=dev)
            v[:, 1:5] = torch.tensor([s + 1, 0, 0, 0], dtype=torch.uint8, device=dev)   # the integer s + 1
            v[:, 0] = ADD if delta else WRITE
            levels.append((keys, amq.KeyBatch.fixed(v)))
            begins.append(torch.arange(L + 1, device=dev) * n)
        table = [amq.merge_run(k, v, b) for (k, v), b in zip(levels, begins)]
        per_job = sum(sizes)
        cap = L * per_job
        kept = [n - shadowed(sizes, s) for s, n in enumerate(sizes)]              # heads per job and level
        n_out = L * sum(kept)
        values_total = sum(int(v.data.numel()) for _, v in levels)
        v_cap = amq.merge_levels_values_bound(values_total, cap - L * sizes[-1])
        ws = torch.empty(max(amq.merge_levels_workspace_bytes(L, K, cap), amq.gather_levels_workspace_bytes(cap)),
                         dtype=torch.uint8, device=dev)
        out_begin = torch.empty(L + 1, dtype=torch.int64, device=dev)
        items = torch.empty(16 * cap, dtype=torch.uint8, device=dev)
        out_keys = torch.empty(cap * 16, dtype=torch.uint8, device=dev)
        out_vals = torch.empty(v_cap, dtype=torch.uint8, device=dev)
        v_offs = torch.empty(cap + 1, dtype=torch.int64, device=dev)
        needed = torch.zeros(2, dtype=torch.int64, device=dev)
        counts = amq.MergeCounts(dev)
        chain = Chain(torch, amq, dev, L, levels, begins, sizes)
        torch.cuda.synchronize()

    def merge():
        amq.merge_levels_device(table, L, out_begin, items, cap, ws, None, 0, counts.counts)

    def gather():
        amq.gather_levels_device(items, out_begin, L, cap, table, out_keys, 16, None, out_keys.numel(), out_vals, v_offs,
                                 v_cap, ws, needed)

    def both():
        merge()
        gather()

    with step_limit(lim, name + ": warm-up and checks"):
        both()
        chain.run()
        torch.cuda.synchronize()
        c = counts.collect()
        # a head of level s < K - 1 with a partner below it: its even items that no newer level holds
        with_partner = [sizes[s] // 2 - shadowed(sizes, s) for s in range(K - 1)]
        assert c == {"newer_count": L * sizes[0], "older_count": L * (per_job - sizes[0]), "pair_count": cap - n_out,
                     "combined_count": L * sum(with_partner) if deltas else 0, "bad_combine_count": 0,
                     "dropped_count": 0, "out_count": n_out}, c
        assert torch.equal(out_begin, torch.arange(L + 1, device=dev) * sum(kept))
        key_total, val_total = (int(x) for x in needed.cpu())
        assert key_total == n_out * 16
        small = 5 if deltas else VALUE_BYTES
        assert val_total == L * (kept[-1] * VALUE_BYTES + sum(kept[:-1]) * small)
        # the head of job 0: key 0 from the newest level (it is in every level), the oldest level's second item, and
        # the numbers ascending
        ks = out_keys[:4096 * 16].view(-1, 16)[:, 8:].cpu().numpy()
        nums = [int.from_bytes(bytes(r), "big") for r in ks]
        assert nums[0] == 0 and nums[1] == 1 << K and all(a < b for a, b in zip(nums, nums[1:]))
        rec = items[:32].cpu().numpy().view(amq.abi.MERGE_ITEM_DTYPE)
        assert int(rec["src"][0]) == 0 and int(rec["src"][1]) == (K - 1) << amq.abi.LEVELS_SRC_SHIFT | 1
        if deltas:                                                   # 1 + 2 + ... + K folded into the oldest WRITE
            assert (int(rec["op"][0]), int(rec["i32"][0]), int(rec["flags"][0])) == (WRITE, K * (K + 1) // 2, 1)
        # the pairwise chain's last round holds the same bytes
        last = chain.rounds[-1]
        assert torch.equal(last["begin"], out_begin)
        assert torch.equal(last["keys"].view(-1)[:key_total], out_keys[:key_total])
        assert torch.equal(last["voffs"][:n_out + 1], v_offs[:n_out + 1])
        assert torch.equal(last["vals"][:val_total], out_vals[:val_total])
    t = {"merge": [], "gather": [], "both": [], "chain": []}
    with step_limit(lim, name + ": timing"):
        for _ in range(args.reps):                                # alternating
            t["merge"].append(timed(torch, merge))
            t["gather"].append(timed(torch, gather))
            t["both"].append(timed(torch, both))
            t["chain"].append(timed(torch, chain.run))
    res = {"run": name, "jobs": L, "sizes": sizes, "items_in": cap, "items_out": n_out, "out_key_bytes": key_total,
           "out_value_bytes": val_total, "workspace_bytes": int(ws.numel()),
           # the items the chain's gathers materialise in all, against the K-way gather's items_out
           "chain_items_gathered": int(sum(int(b["begin"][-1]) for b in chain.rounds))}
    for k, v in t.items():
        res[k] = spread(v)
    for k in ("merge", "gather", "both", "chain"):
        res[k]["gitems_per_s"] = round(cap / res[k]["median_ms"] / 1e6, 2)
    res["chain_over_both"] = round(res["chain"]["median_ms"] / res["both"]["median_ms"], 2)
    say(log, json.dumps(res))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=6104)
    ap.add_argument("--sizes", default="1024,2048,4096,16384")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--step-limit", type=int, default=240)
    ap.add_argument("--log", default=None)
    ap.add_argument("--resources-only", action="store_true")
    args = ap.parse_args()
    log = open(args.log, "w") if args.log else None
    if args.resources_only:
        say(log, "merge_levels: kernel resources (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage)")
        sys.exit(0 if resource_report(log, "tkv_amq_merge.hip", ("levels",)) else 1)
    import torch
    import turtle_kv_amd as amq
    if not torch.cuda.is_available():
        sys.exit("tools/merge_levels.py needs a GPU")
    sizes = [int(x) for x in args.sizes.split(",")]
    assert args.reps >= 7, "at least 7 repetitions"
    assert 2 <= len(sizes) <= amq.abi.MERGE_MAX_RUNS and all(b % a == 0 for a, b in zip(sizes, sizes[1:]))
    assert sizes[0] % 2 == 0 and all(n & (n - 1) == 0 for n in sizes), "powers of two"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    say(log, "merge_levels:", amq.abi.version(), "|", torch.cuda.get_device_name(0))
    say(log, f"workload: {args.jobs} jobs x levels of {sizes} items, newest first, {VALUE_BYTES}-byte values, every second "
             f"key of a level in the next older one; {args.reps} alternating repetitions")
    for deltas in (False, True):
        one_run(args, log, torch, amq, dev, sizes, deltas)


if __name__ == "__main__":
    main()
