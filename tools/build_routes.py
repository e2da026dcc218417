#!/usr/bin/env python3
"""One filter build per build route ("Build routes"), each at about the smallest
shape that reaches it, through tkv_amq_plan / tkv_amq_build(_ex) alone.  Run it under

    rocprofv3 --kernel-trace --output-format csv -d DIR -o run -- python3 tools/build_routes.py

(alone: one traced process, no counters) and reduce the trace to the library's launches with

    python3 tools/build_routes.py --reduce DIR > listing.txt

one line per launch: kernel, grid, workgroup, LDS.  Two versions of the library that take the
same routes give the same listing line for line (profiles/build_routes/).  --big adds the two
routes past kDirectMaxTiles tiles (one filter of ~10 GB of generated 16-byte keys each)."""
import argparse
import csv
import glob
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BLOOM, VQF = 0, 1

# (name, kind, key shape, leaf key counts, bits per key, workspace: True the plan's / False none)
CASES = [
    ("bloom atomics 63 leaves", BLOOM, "k16", [1000] * 63, 10, True),
    ("bloom lds 64 leaves", BLOOM, "k16", [1000] * 64, 10, True),
    ("bloom lds 64 leaves k24", BLOOM, "k24", [1000] * 64, 10, True),
    ("bloom lds 64 leaves var", BLOOM, "var", [1000] * 64, 10, True),
    ("bloom lds 64 leaves of 2560 blocks", BLOOM, "k20", [131_072] * 64 + [1] * 192, 10, True),
    ("bloom lds 2048 leaves, 256 threads", BLOOM, "k24", [300] * 2048, 10, True),
    ("bloom split 100 x 2048", BLOOM, "k16", [2048] * 100, 10, True),
    ("bloom split one leaf k24", BLOOM, "k24", [100_000], 10, True),
    ("bloom split 8 leaves k20", BLOOM, "k20", [40_000] * 8, 12, True),
    ("bloom split 8 leaves var", BLOOM, "var", [40_000] * 8, 12, True),
    ("bloom split refused: no workspace", BLOOM, "k16", [2048] * 100, 10, False),
    ("bloom window 12 x 2 windows", BLOOM, "k16", [140_000] * 12, 10, True),
    ("bloom window k24", BLOOM, "k24", [140_000] * 12, 10, True),
    ("bloom window k20", BLOOM, "k20", [140_000] * 12, 10, True),
    ("bloom window var", BLOOM, "var", [140_000] * 12, 10, True),
    ("bloom window 300 leaves, one part", BLOOM, "k16", [131_073] * 300, 10, True),
    ("bloom window no workspace", BLOOM, "k16", [250_000, 3000, 90_000], 10, False),
    ("bloom window one filter var", BLOOM, "var", [200_000], 10, True),
    ("bloom window 16 windows var", BLOOM, "var", [2_097_152, 3000, 2_097_152], 10, True),
    ("bloom tiled keys one filter k16", BLOOM, "k16", [200_000], 10, True),
    ("bloom tiled keys one filter k24", BLOOM, "k24", [200_000], 10, True),
    ("bloom tiled keys 17 windows", BLOOM, "k16", [2_097_153], 10, True),
    ("bloom tiled keys 129 tiles (no tile split)", BLOOM, "k16", [27_000_000], 10, True),
    ("bloom tiled records var", BLOOM, "var", [2_097_153], 10, True),
    ("bloom tiled records k20", BLOOM, "k20", [2_097_153], 10, True),
    ("bloom tiled records k = 16 var", BLOOM, "var", [2_000_000], 23, True),
    ("bloom atomics k = 17 var", BLOOM, "var", [2_000_000], 24, True),
    ("bloom atomics one filter, no workspace", BLOOM, "k16", [2_097_153], 10, False),
    ("bloom batch: multi-leaf past 5 windows k16", BLOOM, "k16", [655_360, 3000, 655_361, 655_360, 900_000], 10, True),
    ("bloom batch: multi-leaf k24", BLOOM, "k24", [655_360, 3000, 655_361], 10, True),
    ("bloom batch: records leaf past 16 windows var", BLOOM, "var", [2_097_152, 3000, 2_097_153], 10, True),
    ("bloom batch: atomics leaf k = 17 var", BLOOM, "var", [900_000, 3000], 24, True),
    ("vqf ring place one leaf", VQF, "k16", [20_000], 12, True),
    ("vqf ring place k24", VQF, "k24", [20_000] * 3, 12, True),
    ("vqf ring place located k20", VQF, "k20", [20_000] * 8, 12, True),
    ("vqf ring place located var", VQF, "var", [20_000] * 8, 12, True),
    ("vqf ring place direct var, 65 leaves", VQF, "var", [5000] * 65, 12, True),
    ("vqf ring place 600 blocks (no match tables)", VQF, "k16", [24_000] * 4, 12, True),
    ("vqf ring place 2 per CU", VQF, "k16", [10_000] * 300, 12, True),
    ("vqf ring decide + fused 512", VQF, "k16", [30_000] * 600, 12, True),
    ("vqf ring decide k20", VQF, "k20", [30_000] * 600, 12, True),
    ("vqf decide + fused 512", VQF, "k16", [30_000] * 800, 12, True),
    ("vqf decide + fused 256", VQF, "k16", [15_000] * 800, 12, True),
    ("vqf decide var + fused 256", VQF, "var", [3000] * 4200, 12, True),
    ("vqf decide + fused, 4 parts", VQF, "k16", [200_000] * 3, 12, True),
    ("vqf decide + scatter + place", VQF, "k16", [250_000] * 3, 12, True),
    ("vqf decide big, u8 counts", VQF, "k24", [700_000, 1000], 12, True),
    ("vqf decide big, workspace counts", VQF, "k16", [7_000_000], 12, True),
]
BIG_CASES = [
    ("bloom tiled keys routed as bit records (k = 7)", BLOOM, "k16", [671_088_641], 10, True),
    ("bloom tiled keys routed as keys (k = 9)", BLOOM, "k16", [560_000_000], 13, True),
]


def make_keys(amq, torch, shape, n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    if shape == "k16":
        return amq.KeyBatch.fixed(amq.gen_keys16(seed, 0, n))
    if shape in ("k24", "k20"):
        w = int(shape[1:])
        return amq.KeyBatch.fixed(torch.randint(0, 256, (n, w), dtype=torch.uint8, device="cuda", generator=g))
    lens = torch.randint(8, 32, (n,), device="cuda", generator=g)
    offs = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    offs[1:] = torch.cumsum(lens, 0)
    data = torch.randint(0, 256, (int(offs[-1]),), dtype=torch.uint8, device="cuda", generator=g)
    return amq.KeyBatch.variable(data, offs)


def run(big, only):
    import torch

    import turtle_kv_amd as amq
    from turtle_kv_amd.filters import _ptr, _stream_handle
    assert torch.cuda.is_available(), "needs a GPU"
    L = amq.abi.lib()
    for i, (name, kind, shape, counts, bpk, with_ws) in enumerate(CASES + (BIG_CASES if big else [])):
        if only and only not in name:
            continue
        plan = amq.plan_filters(kind, counts, bpk, payload_capacity=(1 << 28) if kind == VQF else 0)
        keys = make_keys(amq, torch, shape, plan.n_keys, 100 + i)
        if with_ws:
            amq.build_all_filters(plan, keys)
        else:  # tkv_amq_build without a workspace pointer
            out = torch.empty(max(plan.total_out_bytes, 1), dtype=torch.uint8, device="cuda")
            amq.abi.check(L.tkv_amq_build(kind, _ptr(keys.data), _ptr(keys.offsets), keys.stride, keys.n,
                                          _ptr(plan.device_segs()), plan.n_segs, plan.max_seg_blocks,
                                          _ptr(out), None, 0, _stream_handle()), "tkv_amq_build")
        torch.cuda.synchronize()
        print(f"{i:3d} {name}: ok ({plan.n_segs} leaves, {plan.n_keys} keys, {plan.max_seg_blocks} blocks)",
              flush=True)
        del keys
        torch.cuda.empty_cache()


def reduce(path):
    files = sorted(glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True))
    assert files, f"no kernel trace under {path}"
    rows = []
    for f in files:
        with open(f, newline="") as fh:
            rows += list(csv.DictReader(fh))
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    dims = lambda r, what: "x".join(r[c] for c in sorted(r) if c.startswith(what))
    for r in rows:
        name = r["Kernel_Name"]
        # the library's kernels only (the key generators and torch's own are set-up)
        if ("tkv::" not in name and "bloom_compact_segs" not in name) or "gen_keys16" in name:
            continue
        name = re.sub(r"\(.*$", "", name.replace("(anonymous namespace)::", "")).replace("void ", "").strip()
        print(name, dims(r, "Grid_Size"), dims(r, "Workgroup_Size"), r["LDS_Block_Size"])


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--big", action="store_true", help="also the two routes past kDirectMaxTiles tiles")
    ap.add_argument("--reduce", metavar="DIR", help="reduce a rocprofv3 kernel trace under DIR to the listing")
    ap.add_argument("--cases", metavar="TEXT", help="only the cases whose name contains TEXT")
    a = ap.parse_args()
    reduce(a.reduce) if a.reduce else run(a.big, a.cases)
