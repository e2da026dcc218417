"""Rate of the hash-range route for keys of any shape (tkv_amq_bloom_route_records_any: bit
records, two per key above 12 bits/key) beside tkv_amq_bloom_route_records_ex on the same
24-byte keys, HIP events, 3 warm-ups and 20 reps.  --n keys per case, --parts the route's parts."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def timed(torch, fn):
    for _ in range(3):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(20)]
    torch.cuda.synchronize()
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev]))


def main():
    import argparse

    import torch

    import turtle_kv_amd as amq
    from oversize_batch import make_keys
    from turtle_kv_amd.filters import _ptr, _stream_handle
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=50_000_000)
    ap.add_argument("--parts", type=int, default=8)
    args = ap.parse_args()
    L = amq.abi.lib()
    n, P = args.n, args.parts
    for shape, bpk, ex in (("k24", 12, True), ("k24", 12, False), ("var", 12, False), ("var", 16, False)):
        kb = make_keys(torch, amq, shape, n)
        plan = amq.plan_filters(amq.BLOOM, [n], bpk)
        seg = plan.segs[0]
        nb, k = int(seg["n_blocks"]), int(seg["hash_count"])
        rpk = int(L.tkv_amq_bloom_records_per_key(k))
        recs = torch.empty(12 * rpk * n, dtype=torch.uint8, device="cuda")
        counts = torch.zeros(P, dtype=torch.int32, device="cuda")
        d_seg = plan.device_segs()
        if ex:
            ws = torch.empty(int(L.tkv_amq_bloom_route_records_ws_bytes(n, P)), dtype=torch.uint8, device="cuda")
            name = "tkv_amq_bloom_route_records_ex"

            def fn():
                amq.abi.check(L.tkv_amq_bloom_route_records_ex(_ptr(kb.data), 24, n, _ptr(d_seg), nb, k, P, _ptr(recs),
                                                               _ptr(counts), _ptr(ws), ws.numel(), _stream_handle()),
                              name)
        else:
            ws = torch.empty(int(L.tkv_amq_bloom_route_records_any_ws_bytes(n, P, k)), dtype=torch.uint8,
                             device="cuda")
            name = "tkv_amq_bloom_route_records_any"

            def fn():
                amq.abi.check(L.tkv_amq_bloom_route_records_any(_ptr(kb.data), _ptr(kb.offsets), kb.stride, n,
                                                                _ptr(d_seg), nb, k, P, _ptr(recs), _ptr(counts),
                                                                _ptr(ws), ws.numel(), _stream_handle()), name)
        ms = timed(torch, fn)
        assert int(counts.sum()) == rpk * n
        print(f"{name} {shape} @{bpk} (k = {k}, {rpk} records per key), {P} parts: {n} keys, {ms * 1e3:.1f} us, "
              f"{n / ms / 1e6:.1f} Gkeys/s", flush=True)
        del kb, recs, ws
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
