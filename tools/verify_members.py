"""Times tkv_amq_verify_members against the composed route it replaces, on one GPU.

  python tools/verify_members.py [--total-keys 100000000] [--reps 7] [--step-limit 120] [--log FILE]
                                 [--no-resources]

Shapes (the bench's, bench.segment_counts): config 2 (--total-keys 16-byte keys in 16,384-key
leaves, Bloom at 10 bits/key: 6,104 leaves at 100M), config 3 (the same leaves as VQF at 12
bits/key in 32,704-byte payloads) and bloom10k24 (config 2's leaves of 24-byte keys).  In one
process, every variant warmed first, then --reps alternating repetitions of ten-call windows
between device events, per-call time reported:
  (a) tkv_amq_verify_members (its three launches);
  (b) the composed route: tkv_amq_probe over a PRECOMPUTED 4-byte segment index per key, then a
      count of the zero answers.  The index expansion (repeat_interleave) is not charged to it;
  (c) the build of the same plan, for scale.
The bar: (a) faster than (b) by more than the spread of the repetitions, for both kinds;
(a) / (c) is reported.  Before timing, (a)'s per-leaf counts are checked against (b)'s answers on a
damaged copy of the filters.  One more line times an uneven batch (one 3M-key leaf, one 150K-key
leaf and 300 small ones: no bar; the large leaves are split over workgroups).  Every step runs
under its own time limit (--step-limit seconds; the process exits if one overruns).  Prints one
JSON line per shape, and the compiler's resource report of the kernels.  Needs a GPU."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench import segment_counts  # noqa: E402
from open_scan import say, spread, step_limit, timed, INNER  # noqa: E402
from walk_paths import resource_report  # noqa: E402

VQF_CAP = 32704


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--total-keys", type=int, default=100_000_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--step-limit", type=int, default=120)
    ap.add_argument("--log", default=None)
    ap.add_argument("--no-resources", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch
    import turtle_kv_amd as amq
    if not torch.cuda.is_available():
        sys.exit("tools/verify_members.py needs a GPU")
    assert args.reps >= 7, "at least 7 repetitions of each leg"
    log = open(args.log, "w") if args.log else None
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lim = args.step_limit
    say(log, "verify_members:", amq.abi.version(), "|", torch.cuda.get_device_name(0))
    if not args.no_resources:
        with step_limit(1200, "resource report"):
            # (tkv_amq_verify.h is compiled with the builds, in tkv_amq_kernels.hip)
            resource_report(log, "tkv_amq_kernels.hip", ("verify_",), timeout=1200)

    n_all = args.total_keys // 2 * 2
    counts = segment_counts(n_all)
    shapes = [("config2_bloom10", amq.BLOOM, 10, 0, 16), ("config3_vqf12", amq.VQF, 12, VQF_CAP, 16),
              ("bloom10k24", amq.BLOOM, 10, 0, 24)]
    results = {}
    kb, stride_have = None, 0
    for name, kind, bpk, cap, stride in shapes:
        if stride != stride_have:
            with step_limit(lim, f"keys ({stride} bytes)"):
                kb = None
                raw = amq.gen_keys16(42, 0, n_all * stride // 16, device=dev)
                kb = amq.KeyBatch.fixed(raw.view(n_all, stride))
                stride_have = stride
                torch.cuda.synchronize()
        with step_limit(lim, f"{name}: build"):
            plan = amq.plan_filters(kind, counts, bpk, payload_capacity=cap)
            bws = torch.empty(max(plan.workspace_bytes, 16), dtype=torch.uint8, device=dev)
            filt = amq.build_all_filters(plan, kb, workspace=bws)
            scratch = torch.empty_like(filt)   # (c) builds here
            torch.cuda.synchronize()
        n = plan.n_segs
        segs = plan.device_segs(dev)
        d_res = torch.empty(16 * n, dtype=torch.uint8, device=dev)
        d_tot = torch.empty(1, dtype=torch.int64, device=dev)
        ws = torch.empty(amq.verify_members_workspace_bytes(n), dtype=torch.uint8, device=dev)
        with step_limit(lim, f"{name}: segment index"):
            qseg = torch.repeat_interleave(torch.arange(n, dtype=torch.int32, device=dev),
                                           torch.from_numpy(np.asarray(counts, dtype=np.int64)).to(dev))
            answers = torch.empty(n_all, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()

        def verify(f=filt):
            amq.verify_members_device(kind, f, segs, n, plan.max_seg_blocks, kb.data, None, stride, n_all, None,
                                      d_res, d_tot, ws)

        def composed(f=filt):
            amq.probe_filters(plan, f, kb, qseg, out=answers)
            return n_all - torch.count_nonzero(answers)

        def build():
            amq.build_all_filters(plan, kb, out=scratch, workspace=bws, check=False)

        with step_limit(lim, f"{name}: check on a damaged copy"):
            verify()
            torch.cuda.synchronize()
            assert int(d_tot.item()) == 0 and int(composed().item()) == 0, "a clean build has no false negative"
            bad = filt.clone()
            hdr = 64 if kind == amq.BLOOM else 80
            for s in (0, n // 2, n - 1):   # the first third of three leaves' blocks zeroed
                o = int(plan.segs["out_offset"][s]) + hdr
                bad[o:o + 64 * (int(plan.segs["n_blocks"][s]) // 3)] = 0
            verify(bad)
            got = d_res.cpu().numpy().view(amq.abi.MEMBER_CHECK_DTYPE).copy()
            total = int(d_tot.item())
            zeros = int(composed(bad).item())
            per_leaf = torch.bincount(qseg[answers == 0].to(torch.int64), minlength=n).cpu().numpy()
            assert total == zeros > 0 and np.array_equal(got["missing"], per_leaf), (total, zeros)
            assert sorted(np.flatnonzero(got["missing"]).tolist()) == sorted({0, n // 2, n - 1})
            del bad
        with step_limit(lim, f"{name}: warm"):
            for _ in range(3):
                verify()
                composed()
                build()
            torch.cuda.synchronize()
        ta, tb, tc = [], [], []
        with step_limit(lim, f"{name}: timed"):
            for _ in range(args.reps):   # alternate
                ta.append(timed(torch, verify))
                tb.append(timed(torch, composed))
                tc.append(timed(torch, build))
        a, b, c = spread(ta), spread(tb), spread(tc)
        gap = b["median_ms"] - a["median_ms"]
        noise = max(a["max_ms"] - a["min_ms"], b["max_ms"] - b["min_ms"])
        res = {"shape": name, "leaves": n, "keys": n_all, "key_bytes": stride,
               "filter_bytes": int(filt.numel()), "max_seg_blocks": plan.max_seg_blocks,
               "verify_members": {**a, "gkeys_per_s": round(n_all / a["median_ms"] / 1e6, 1)},
               "probe_plus_count": {**b, "gkeys_per_s": round(n_all / b["median_ms"] / 1e6, 1)},
               "build": {**c, "gkeys_per_s": round(n_all / c["median_ms"] / 1e6, 1)},
               "verify_ms_all": [round(x, 4) for x in ta], "composed_ms_all": [round(x, 4) for x in tb],
               "build_ms_all": [round(x, 4) for x in tc], "calls_per_window": INNER,
               "composed_over_verify": round(b["median_ms"] / a["median_ms"], 3),
               "verify_over_build": round(a["median_ms"] / c["median_ms"], 3),
               "gap_ms": round(gap, 4), "spread_ms": round(noise, 4), "verify_faster_by_more_than_spread": gap > noise}
        results[name] = res
        say(log, json.dumps(res))
        del filt, scratch, qseg, answers, d_res, ws, bws

    # the uneven batch: no leaf is walked by one workgroup
    with step_limit(lim, "uneven: build"):
        ucounts = [3_000_000, 150_000] + [1 + (37 * i) % 600 for i in range(300)]
        un = sum(ucounts)
        ukb = amq.KeyBatch.fixed(kb.data.view(-1)[:un * 16].view(un, 16))
        plan = amq.plan_filters(amq.BLOOM, ucounts, 10)
        bws = torch.empty(max(plan.workspace_bytes, 16), dtype=torch.uint8, device=dev)
        filt = amq.build_all_filters(plan, ukb, workspace=bws)
        n = plan.n_segs
        segs = plan.device_segs(dev)
        d_res = torch.empty(16 * n, dtype=torch.uint8, device=dev)
        d_tot = torch.empty(1, dtype=torch.int64, device=dev)
        ws = torch.empty(amq.verify_members_workspace_bytes(n), dtype=torch.uint8, device=dev)
        qseg = torch.repeat_interleave(torch.arange(n, dtype=torch.int32, device=dev),
                                       torch.from_numpy(np.asarray(ucounts, dtype=np.int64)).to(dev))
        answers = torch.empty(un, dtype=torch.uint8, device=dev)

        def uverify():
            amq.verify_members_device(amq.BLOOM, filt, segs, n, plan.max_seg_blocks, ukb.data, None, 16, un, None,
                                      d_res, d_tot, ws)

        def ucomposed():
            amq.probe_filters(plan, filt, ukb, qseg, out=answers)
            return un - torch.count_nonzero(answers)

        for _ in range(3):
            uverify()
            ucomposed()
        torch.cuda.synchronize()
        assert int(d_tot.item()) == 0
    with step_limit(lim, "uneven: timed"):
        ta, tb = [], []
        for _ in range(args.reps):
            ta.append(timed(torch, uverify))
            tb.append(timed(torch, ucomposed))
    say(log, json.dumps({"shape": "uneven_3M_150K_300small", "leaves": n, "keys": un,
                         "verify_members": spread(ta), "probe_plus_count": spread(tb)}))
    say(log, json.dumps({"verify_faster_by_more_than_spread":
                         {k: v["verify_faster_by_more_than_spread"] for k, v in results.items()}}))
    if log:
        log.close()


if __name__ == "__main__":
    main()
