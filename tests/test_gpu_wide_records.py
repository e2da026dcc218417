"""Wide bit records (9 <= k <= 16: two 12-byte records per key) and the route for keys of any
shape: tkv_amq_bloom_route_records_any + tkv_amq_bloom_build_range_records through the C ABI,
the hash-range builders on variable-length and other fixed-size keys, and oversize leaves of
such keys above 12 bits/key in a tkv_amq_build_ex batch.  Every filter is compared byte for
byte with the CPU oracle."""
import numpy as np
import pytest

from test_gpu_hash_shard import _free_port
from test_gpu_parity import assert_same, oracle_per_segment

pytestmark = pytest.mark.gpu

GUARD = 4096


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need a visible MI355X"
    return t


def make_keys(shape, n, seed, dup=0):
    """(bytes, int64 offsets or None, stride).  "var": lengths 1..31, every 97th key 32..70
    bytes (both hash branches); "kN": N-byte keys (k40: the per-seed long hash).  dup: the last
    `dup` keys are copies of one key."""
    rng = np.random.default_rng(seed)
    if shape != "var":
        stride = int(shape[1:])
        keys = rng.integers(0, 256, (n, stride), dtype=np.uint8)
        if dup:
            keys[n - dup:] = keys[n // 3]
        return keys, None, stride
    lens = rng.integers(1, 32, n)
    lens[::97] = rng.integers(32, 71, lens[::97].size)
    if dup:
        lens[n - dup:] = 19
    offs = np.zeros(n + 1, np.int64)
    offs[1:] = np.cumsum(lens)
    keys = rng.integers(0, 256, int(offs[-1]), dtype=np.uint8)
    if dup:
        keys[offs[n - dup]:] = np.tile(keys[offs[n - dup]:offs[n - dup] + 19], dup)
    return keys, offs, 0


def oracle_filter(oracle, keys, offs, stride, n, bpk):
    st, ref = oracle.bloom_build(keys, n, bpk, src_page_id=0,
                                 offsets=None if offs is None else offs.astype(np.uint64), stride=stride)
    assert st == 0
    return ref.tobytes()


def route_any(amq, torch, keys_t, offs_t, stride, n, plan, n_parts, ws_short=0, k=None):
    """-> (status, records [rpk * n, 12] on the device, counts in records)."""
    from turtle_kv_amd.filters import _ptr, _stream_handle
    L = amq.abi.lib()
    seg = plan.segs[0]
    k = int(seg["hash_count"]) if k is None else k
    rpk = max(1, int(L.tkv_amq_bloom_records_per_key(k)))
    buf = torch.full((12 * rpk * n + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    counts = torch.full((max(n_parts, 1),), -1, dtype=torch.int32, device="cuda")
    need = int(L.tkv_amq_bloom_route_records_any_ws_bytes(n, n_parts, k))
    ws = torch.empty(max(need, 4096), dtype=torch.uint8, device="cuda")
    st = L.tkv_amq_bloom_route_records_any(_ptr(keys_t) if n else None, _ptr(offs_t), stride, n,
                                           _ptr(plan.device_segs()), int(seg["n_blocks"]), k, n_parts,
                                           _ptr(buf), _ptr(counts), _ptr(ws), need - ws_short, _stream_handle())
    torch.cuda.synchronize()
    assert bool((buf[12 * rpk * n:] == 0xA5).all()), "the guard after the record buffer was written"
    return st, buf[:12 * rpk * n].view(rpk * n, 12), counts.cpu().numpy().astype(np.int64)


def build_range_records(amq, torch, recs, plan, t0, t1, out, k=None):
    from turtle_kv_amd.filters import _ptr, _stream_handle
    L = amq.abi.lib()
    seg = plan.segs[0]
    m = recs.shape[0]
    ws = torch.empty(max(1, int(L.tkv_amq_bloom_build_range_records_ws_bytes(m, t0, t1))), dtype=torch.uint8,
                     device="cuda")
    return L.tkv_amq_bloom_build_range_records(_ptr(recs) if m else None, m, _ptr(plan.device_segs()),
                                               int(seg["n_blocks"]), int(seg["hash_count"]) if k is None else k,
                                               t0, t1, _ptr(out), _ptr(ws), ws.numel(), _stream_handle())


# shape, n, bits/key (k), parts, copies of one key
ROUTE_CASES = [
    ("k24", 300_000, 16, 3, 0),      # k = 11; 9,375 blocks = 5 tiles, parts of 2/2/1, partial last tile
    ("var", 300_000, 13, 8, 0),      # k = 9: one real index in the second record; parts 4..7 empty
    ("var", 300_000, 23, 2, 0),      # k = 16: a full second record; 7 tiles, parts of 4/3
    ("k20", 200_000, 16, 1, 0),      # one part; last tile of 106 blocks
    ("k40", 150_000, 14, 2, 0),      # k = 10, long keys; last tile of 6 blocks
    ("var", 400_000, 16, 3, 150_000),  # wide records through the overflow lists
    ("k24", 300_000, 12, 3, 0),      # k = 8, one record per key: counts equal route_records_ex's
    ("k16", 300_000, 16, 2, 0),      # also equal to tkv_amq_bloom_route + tkv_amq_bloom_build_range
]


@pytest.mark.parametrize("shape,n,bpk,n_parts,dup", ROUTE_CASES)
def test_route_any_and_range_builds_equal_oracle(oracle, amq, torch, shape, n, bpk, n_parts, dup):
    from turtle_kv_amd.dist import hash_shard_tiles
    from turtle_kv_amd.filters import _ptr, _stream_handle
    L = amq.abi.lib()
    keys, offs, stride = make_keys(shape, n, 1000 + bpk, dup)
    ref = oracle_filter(oracle, keys, offs, stride, n, bpk)
    plan = amq.plan_filters(0, [n], bpk)
    nb, k = int(plan.segs[0]["n_blocks"]), int(plan.segs[0]["hash_count"])
    rpk = int(L.tkv_amq_bloom_records_per_key(k))
    assert rpk == (1 if bpk <= 12 else 2)
    keys_t = torch.from_numpy(keys).cuda()
    offs_t = None if offs is None else torch.from_numpy(offs).cuda()
    st, recs, counts = route_any(amq, torch, keys_t, offs_t, stride, n, plan, n_parts)
    assert st == 0
    assert counts.sum() == rpk * n and (counts % rpk == 0).all()
    T, q = hash_shard_tiles(nb, n_parts)
    base = np.concatenate([[0], np.cumsum(counts)])
    out = torch.zeros(plan.total_out_bytes, dtype=torch.uint8, device="cuda")
    for p in range(n_parts):
        t0, t1 = min(T, p * q), min(T, (p + 1) * q)
        if t0 == t1:
            assert counts[p] == 0
        st = build_range_records(amq, torch, recs[int(base[p]):int(base[p + 1])], plan, t0, t1, out)
        assert st == 0
    torch.cuda.synchronize()
    assert out.cpu().numpy().tobytes() == ref
    if shape == "k24" and bpk == 12:
        routed = torch.empty(12 * n, dtype=torch.uint8, device="cuda")
        c2 = torch.zeros(n_parts, dtype=torch.int32, device="cuda")
        ws = torch.empty(int(L.tkv_amq_bloom_route_records_ws_bytes(n, n_parts)), dtype=torch.uint8, device="cuda")
        amq.abi.check(L.tkv_amq_bloom_route_records_ex(_ptr(keys_t), 24, n, _ptr(plan.device_segs()), nb, k,
                                                       n_parts, _ptr(routed), _ptr(c2), _ptr(ws), ws.numel(),
                                                       _stream_handle()), "route_records_ex")
        torch.cuda.synchronize()
        assert np.array_equal(c2.cpu().numpy(), counts)
    if shape == "k16":
        routed = torch.empty_like(keys_t)
        c2 = torch.zeros(n_parts, dtype=torch.int32, device="cuda")
        ws = torch.empty(int(L.tkv_amq_bloom_route_ws_bytes(n, n_parts)), dtype=torch.uint8, device="cuda")
        amq.abi.check(L.tkv_amq_bloom_route(_ptr(keys_t), n, _ptr(plan.device_segs()), nb, n_parts, _ptr(routed),
                                            _ptr(c2), _ptr(ws), ws.numel(), _stream_handle()), "route")
        torch.cuda.synchronize()
        c2 = c2.cpu().numpy().astype(np.int64)
        assert np.array_equal(rpk * c2, counts)
        b2 = np.concatenate([[0], np.cumsum(c2)])
        out2 = torch.zeros_like(out)
        for p in range(n_parts):
            part = routed[int(b2[p]):int(b2[p + 1])]
            ws = torch.empty(max(1, int(L.tkv_amq_bloom_build_range_ws_bytes(part.shape[0], p * q, min(T, (p + 1) * q)))),
                             dtype=torch.uint8, device="cuda")
            amq.abi.check(L.tkv_amq_bloom_build_range(_ptr(part), part.shape[0], _ptr(plan.device_segs()), nb,
                                                      p * q, min(T, (p + 1) * q), _ptr(out2), _ptr(ws), ws.numel(),
                                                      _stream_handle()), "build_range")
        torch.cuda.synchronize()
        assert torch.equal(out2, out)


def test_route_any_refusals(amq, torch):
    INVALID = amq.abi.INVALID_ARGUMENT
    n = 5000
    keys, offs, stride = make_keys("var", n, 5)
    plan = amq.plan_filters(0, [n], 16)
    keys_t, offs_t = torch.from_numpy(keys).cuda(), torch.from_numpy(offs).cuda()
    assert route_any(amq, torch, keys_t, offs_t, 0, n, plan, 2)[0] == 0
    assert route_any(amq, torch, keys_t, offs_t, 0, n, plan, 2, k=17)[0] == INVALID
    assert route_any(amq, torch, keys_t, offs_t, 0, n, plan, 2, k=0)[0] == INVALID
    assert route_any(amq, torch, keys_t, offs_t, 0, n, plan, 0)[0] == INVALID
    assert route_any(amq, torch, keys_t, offs_t, 0, n, plan, 2049)[0] == INVALID
    assert route_any(amq, torch, keys_t, None, 0, n, plan, 2)[0] == INVALID      # stride 0, no offsets
    assert route_any(amq, torch, keys_t, offs_t, 0, n, plan, 2, ws_short=256)[0] == INVALID
    recs = torch.zeros((16, 12), dtype=torch.uint8, device="cuda")
    out = torch.zeros(plan.total_out_bytes, dtype=torch.uint8, device="cuda")
    assert build_range_records(amq, torch, recs, plan, 0, 1, out, k=17) == INVALID
    st, _, counts = route_any(amq, torch, keys_t, offs_t, 0, 0, plan, 3)
    assert st == 0 and counts.tolist() == [0, 0, 0]
    st, _, counts = route_any(amq, torch, None, None, 20, 0, plan, 3)
    assert st == 0 and counts.tolist() == [0, 0, 0]


def _batch(amq, torch, keys, offs):
    keys_t = torch.from_numpy(keys).cuda()
    if offs is None:
        return amq.KeyBatch.fixed(keys_t)
    return amq.KeyBatch.variable(keys_t, torch.from_numpy(offs).cuda())


def test_hash_sharded_takes_24_byte_keys_above_12_bits(oracle, amq, torch):
    from turtle_kv_amd.dist import HashShardedBloom
    n = 300_000
    keys, _, _ = make_keys("k24", n, 31)
    filt = HashShardedBloom(n, 16, 1, 0, "cuda").build(torch.from_numpy(keys).cuda())
    assert filt.cpu().numpy().tobytes() == oracle_filter(oracle, keys, None, 24, n, 16)


@pytest.mark.parametrize("bpk", [10, 16])
def test_exact_hash_sharded_takes_variable_length_keys(oracle, amq, torch, bpk):
    from turtle_kv_amd.dist import ExactHashShardedBloom
    n = 300_000
    keys, offs, _ = make_keys("var", n, 32)
    ex = ExactHashShardedBloom(n, bpk, 1, 0, "cuda")
    filt = ex.build(_batch(amq, torch, keys, offs))
    assert ex.route_records and ex.route_unit == 12
    assert filt.cpu().numpy().tobytes() == oracle_filter(oracle, keys, offs, 0, n, bpk)


def test_key_shape_fallback_does_not_latch(oracle, amq, torch):
    from turtle_kv_amd.dist import HashShardedBloom
    n = 700_000
    hs = HashShardedBloom(n, 12, 1, 0, "cuda")
    keys, offs, _ = make_keys("var", n, 33)
    filt = hs.build(_batch(amq, torch, keys, offs))
    assert hs.last_fallback == "key_shape"
    assert filt.cpu().numpy().tobytes() == oracle_filter(oracle, keys, offs, 0, n, 12)
    k16 = amq.gen_keys16(34, 0, n)
    filt = hs.build(k16)
    assert hs.last_fallback is None
    assert filt.cpu().numpy().tobytes() == oracle_filter(oracle, k16.cpu().numpy(), None, 16, n, 12)


def _wide_worker(rank, world, port, n_total, bpk, split, q):
    """One gloo rank on the box's one GPU: HashShardedBloom.build over this rank's share of
    variable-length keys regenerated from a seed; rank 0 checks the filter against the oracle."""
    import os
    import sys

    import torch
    import torch.distributed as dist
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tests"))
    import turtle_kv_amd as amq
    from turtle_kv_amd.dist import HashShardedBloom
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    keys, offs, _ = make_keys("var", n_total, 99)
    bounds = [0] + [int(n_total * f) for f in split] + [n_total]
    k0, k1 = bounds[rank], bounds[rank + 1]
    mine = amq.KeyBatch.variable(torch.from_numpy(keys[offs[k0]:offs[k1]]).cuda(),
                                 torch.from_numpy(offs[k0:k1 + 1] - offs[k0]).cuda())
    hs = HashShardedBloom(n_total, bpk, world, rank, "cuda")
    filt = hs.build(mine)
    res = None
    if rank == 0:
        from oracle import oracle as O
        O.build_oracle()
        res = filt.cpu().numpy().tobytes() == oracle_filter(O, keys, offs, 0, n_total, bpk)
    dist.barrier()
    dist.destroy_process_group()
    if rank == 0:
        q.put(res)


def test_wide_records_two_gloo_ranks():
    """Variable-length keys at 16 bits/key (k = 11) over two ranks holding 0.6 / 0.4 of them:
    wide records routed, exchanged (counts in records) and built by their owners."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_wide_worker, args=(r, 2, port, 500_000, 16, (0.6,), q)) for r in range(2)]
    for p in ps:
        p.start()
    for p in ps:
        p.join(300)
    assert all(p.exitcode == 0 for p in ps), [p.exitcode for p in ps]
    assert q.get(timeout=5), "filter differs from the oracle"


@pytest.mark.parametrize("shape,bpk,counts", [
    ("var", 13, [1_620_000, 500, 16384]),   # k = 9
    ("k20", 23, [920_000, 3]),              # k = 16
    ("var", 24, [880_000, 500]),            # k = 17: stays on device atomics
])
def test_oversize_other_shapes_above_12_bits(oracle, amq, torch, shape, bpk, counts):
    """Leaves just past 16 LDS windows (40,960 blocks) of variable-length and 20-byte keys at
    13 to 24 bits/key in a tkv_amq_build_ex batch: up to k = 16 hashed into wide records and
    built by the tiled build, which the plan's workspace must hold."""
    n = sum(counts)
    keys, offs, stride = make_keys(shape, n, 7 * bpk)
    ref = oracle_per_segment(oracle, 0, keys, counts, bpk, stride=stride,
                             offsets=None if offs is None else offs.astype(np.uint64))
    plan = amq.plan_filters(amq.BLOOM, counts, bpk)
    assert plan.max_seg_blocks > 40960
    if bpk <= 23:
        assert plan.workspace_bytes >= 2 * 12 * counts[0]
    _, leaves = amq.filters.build_route(plan, stride, offs is not None)
    want = amq.abi.LEAF_TILED_RECORDS if bpk <= 23 else amq.abi.LEAF_ATOMICS
    assert list(leaves) == [want] + [amq.abi.LEAF_BATCH] * (len(counts) - 1)
    kb = _batch(amq, torch, keys, offs)
    out = torch.full((plan.total_out_bytes,), 0xA5, dtype=torch.uint8, device="cuda")
    amq.build_all_filters(plan, kb, out=out)
    torch.cuda.synchronize()
    assert_same(plan, out.cpu().numpy(), ref)
    if bpk != 13:
        return
    # a workspace 256 bytes short of the plan's: the library falls back and still builds it
    _, leaves = amq.filters.build_route(plan, stride, True, workspace_bytes=plan.workspace_bytes - 256)
    assert leaves[0] == amq.abi.LEAF_ATOMICS
    ws = torch.full((plan.workspace_bytes,), 0xFF, dtype=torch.uint8, device="cuda")
    out2 = torch.full((plan.total_out_bytes,), 0x5A, dtype=torch.uint8, device="cuda")
    st = amq.abi.lib().tkv_amq_build_ex(plan.kind, kb.data.data_ptr(), kb.offsets.data_ptr(), 0, n,
                                        plan.device_segs(kb.data.device).data_ptr(), plan.segs.ctypes.data,
                                        plan.n_segs, plan.max_seg_blocks, out2.data_ptr(), ws.data_ptr(),
                                        plan.workspace_bytes - 256, None)
    amq.abi.check(st, "tkv_amq_build_ex")
    torch.cuda.synchronize()
    assert_same(plan, out2.cpu().numpy(), ref)
