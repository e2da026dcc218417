"""The device hash computes `h ^= h >> 29` of every XXH64 avalanche with one 64-bit shift
(dshr<29>, turtle_kv_amd/csrc/tkv_amq_device.h).  Every kernel that hashes changed with it, so
every leaf built here is byte-compared with the CPU oracle, every probe answer with the oracle's,
and every batch asserts its route, so that the kernel meant is the kernel run.

  batch                                          route asserted
  3 leaves of 1 / 63 / 64 / 65 / 1,025 keys      ROUTE_ATOMICS (bloom_global_set: under 64 leaves
                                                 of under 2,048 keys nothing is split)
  3 leaves of 2,048 keys                         ROUTE_SPLIT (bloom_build_split + merge)
  300 leaves of 1 / 63 / 64 / 65 / 1,025 keys    ROUTE_LDS, 1,024 threads (one workgroup a leaf)
  2,048 leaves of 65 keys                        ROUTE_LDS, 256 threads (the flagship's kernel)
  one 200,000-key leaf at 12 bits per key        ROUTE_WINDOW, two windows
  one filter of the fewest keys that are tiled   ROUTE_TILED_KEYS (the size is searched through
                                                 build_route, not written down)
  VQF, one leaf of 64 and one of 1,025 keys      ROUTE_VQF_RING_PLACE

each at 6, 10, 12 and 20 bits per key (k = 4, 7, 8 and 14: the run-time ladder and the unrolled
7 and 8), for 16-byte, 24-byte and 20-byte keys, variable keys of 8..31 bytes (BloomShort) and
variable keys of 32..40 bytes (BloomLong, xxh64_bytes).  The 16-byte and variable batches are
probed with every member and as many non-members.

What separates a right `h >> 29` from a wrong one is the top three bits of h: they are all that
the high word of the shifted value holds.  The 16-byte tests restate XXH64 in Python integers and
assert that, for every seed they use, their keys hold a value with those bits zero and one with
them non-zero at that point of the hash."""
import numpy as np
import pytest

from test_gpu_parity import assert_same, gpu_build, oracle_per_segment, sorted_keys

pytestmark = pytest.mark.gpu

LEAF_KEYS = [1, 63, 64, 65, 1025]
BPKS = [6, 10, 12, 20]
HASHES = {6: 4, 10: 7, 12: 8, 20: 14}
SHAPES = ["k16", "k24", "k20", "var", "long"]
PROBED = ("k16", "var", "long")
VQF_SEED = 0x9D0924DC03E79A75
M = (1 << 64) - 1
P1, P2, P3, P4, P5 = (0x9E3779B185EBCA87, 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9,
                      0x85EBCA77C2B2AE63, 0x27D4EB2F165667C5)


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need a visible MI355X"
    return t


# ---- XXH64 of a 16-byte key in Python integers (xxHash spec, the short-input path) ----
def rotl(x, r):
    return ((x << r) | (x >> (64 - r))) & M


def xxh_round0(v):
    return (rotl((v * P2) & M, 31) * P1) & M


def xxh16_before_shift29(key: bytes, seed: int) -> int:
    """h as it enters `h ^= h >> 29`"""
    h = (seed + P5 + 16) & M
    for i in (0, 8):
        h ^= xxh_round0(int.from_bytes(key[i:i + 8], "little"))
        h = (rotl(h, 27) * P1 + P4) & M
    h ^= h >> 33
    return (h * P2) & M


def xxh16(key: bytes, seed: int) -> int:
    h = xxh16_before_shift29(key, seed)
    h ^= h >> 29
    h = (h * P3) & M
    return h ^ (h >> 32)


def bloom_seed(i):
    z = (0x243F6A8885A308D3 + i * 0x9E3779B97F4A7C15) & M
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
    return z ^ (z >> 31)


def assert_keys_separate_the_shift(oracle, keys16, seeds):
    """For every seed: a key whose h has its top three bits zero where `h >> 29` is taken, and one
    with them non-zero.  The restated hash is checked against the oracle's on the way."""
    rows = [k.tobytes() for k in keys16.reshape(-1, 16)]
    for seed in seeds:
        assert xxh16(rows[0], seed) == oracle.xxh64(rows[0], seed), hex(seed)
        top = {xxh16_before_shift29(k, seed) >> 61 != 0 for k in rows}
        assert top == {False, True}, (hex(seed), top, len(rows))


# ---- keys ----
def make_keys(oracle, shape, seed, n):
    """(key bytes, stride, offsets or None) of n keys"""
    rng = np.random.default_rng(seed)
    if shape == "k16":
        return oracle.gen_keys16(seed, 0, n), 16, None
    if shape in ("k24", "k20"):
        stride = int(shape[1:])
        return rng.integers(0, 256, (n, stride), dtype=np.uint8), stride, None
    lens = rng.integers(8, 32, n) if shape == "var" else rng.integers(32, 41, n)
    offs = np.zeros(n + 1, np.int64)
    offs[1:] = np.cumsum(lens)
    return rng.integers(0, 256, max(int(lens.sum()), 1), dtype=np.uint8), 0, offs


def key_batch(amq, torch, keys, offs):
    if offs is None:
        return amq.KeyBatch.fixed(torch.from_numpy(keys).cuda())
    return amq.KeyBatch.variable(torch.from_numpy(keys).cuda(), torch.from_numpy(offs).cuda())


def build_and_compare(oracle, amq, torch, shape, counts, bpk, seed):
    """Builds the batch and compares every leaf with the oracle.
    Returns (route, plan, filter bytes, keys, offsets, oracle payloads)."""
    keys, stride, offs = make_keys(oracle, shape, seed, sum(counts))
    plan, out = gpu_build(amq, torch, 0, torch.from_numpy(keys).cuda(), counts, bpk,
                          offsets_t=None if offs is None else torch.from_numpy(offs).cuda())
    r, _ = amq.filters.build_route(plan, stride, offs is not None)
    ref = oracle_per_segment(oracle, 0, keys, counts, bpk, stride=stride,
                             offsets=None if offs is None else offs.astype(np.uint64))
    assert_same(plan, out, ref)
    return r, plan, out, keys, offs, ref


def oracle_answers(oracle, plan, out, ref, q, q_offs, qseg):
    """the oracle's answer to every lookup, over the filters just compared with its own"""
    if q_offs is None:
        st, want = oracle.probe_segments(0, out, plan.segs["out_offset"], q, qseg.astype(np.uint32))
        assert st == 0
        return want
    query = oracle.lib().tkvo_bloom_query_payload
    payload = [np.frombuffer(r, np.uint8) for r in ref]
    base = [p.ctypes.data for p in payload]
    q = np.ascontiguousarray(q)
    qp = q.ctypes.data
    return np.array([query(base[s], qp + int(a), int(b - a))
                     for s, a, b in zip(qseg.tolist(), q_offs[:-1].tolist(), q_offs[1:].tolist())],
                    dtype=np.uint8)


def probe_and_compare(oracle, amq, torch, shape, plan, out, ref, keys, offs, counts, seed):
    """every member and as many non-members of the same shape, answer for answer"""
    n = sum(counts)
    miss, _, miss_offs = make_keys(oracle, shape, seed + 1000, n)
    seg_of = np.repeat(np.arange(len(counts)), counts)
    qseg = np.concatenate([seg_of, np.random.default_rng(seed).integers(0, len(counts), n)]).astype(np.int32)
    if offs is None:
        q, q_offs = np.concatenate([keys, miss]), None
    else:
        q = np.concatenate([keys[:offs[n]], miss[:miss_offs[n]]])
        q_offs = np.concatenate([offs[:n], offs[n] + miss_offs[:n + 1]])
    got = amq.probe_filters(plan, torch.from_numpy(out).cuda(), key_batch(amq, torch, q, q_offs),
                            torch.from_numpy(qseg).cuda()).cpu().numpy()
    want = oracle_answers(oracle, plan, out, ref, q, q_offs, qseg)
    assert np.array_equal(got.astype(np.uint8), want.astype(np.uint8)), np.nonzero(got != want)[0][:8]
    assert got[:n].all(), "false negative"


@pytest.mark.parametrize("n_leaves", [3, 300])
@pytest.mark.parametrize("bpk", BPKS)
@pytest.mark.parametrize("shape", SHAPES)
def test_bloom_leaves(oracle, amq, torch, shape, bpk, n_leaves):
    A = amq.abi
    seen16 = []
    for per_leaf in LEAF_KEYS:
        counts = [per_leaf] * n_leaves
        seed = 900 + per_leaf
        r, plan, out, keys, offs, ref = build_and_compare(oracle, amq, torch, shape, counts, bpk, seed)
        assert int(plan.segs["hash_count"][0]) == HASHES[bpk]
        if n_leaves == 3:
            assert r.route == A.ROUTE_ATOMICS, r.route
        else:
            assert r.route == A.ROUTE_LDS and r.threads == 1024, (r.route, r.threads)
        if shape in PROBED:
            probe_and_compare(oracle, amq, torch, shape, plan, out, ref, keys, offs, counts, seed)
        if shape == "k16":
            seen16.append(keys)
    if shape == "k16":
        assert_keys_separate_the_shift(oracle, np.concatenate(seen16)[:4096],
                                       [bloom_seed(j) for j in range(HASHES[bpk])])


@pytest.mark.parametrize("bpk", BPKS)
@pytest.mark.parametrize("shape", SHAPES)
def test_bloom_split_of_three(oracle, amq, torch, shape, bpk):
    """Three leaves are split from 2,048 keys a leaf on: bloom_build_split and bloom_split_merge."""
    counts = [2048] * 3
    r, plan, out, keys, offs, ref = build_and_compare(oracle, amq, torch, shape, counts, bpk, 31)
    assert r.route == amq.abi.ROUTE_SPLIT and r.parts >= 2, (r.route, r.parts)
    if shape in PROBED:
        probe_and_compare(oracle, amq, torch, shape, plan, out, ref, keys, offs, counts, 31)
    if shape == "k16":
        assert_keys_separate_the_shift(oracle, keys[:4096], [bloom_seed(j) for j in range(HASHES[bpk])])


@pytest.mark.parametrize("bpk", BPKS)
@pytest.mark.parametrize("shape", SHAPES)
def test_bloom_256_thread_leaves(oracle, amq, torch, shape, bpk):
    """2,048 leaves: the 256-thread bloom_build_lds, whose 16- and 24-byte loops the flagship runs."""
    counts = [65] * 2048
    r, *_ = build_and_compare(oracle, amq, torch, shape, counts, bpk, 32)
    assert r.route == amq.abi.ROUTE_LDS and r.threads == 256, (r.route, r.threads)


@pytest.mark.parametrize("shape", SHAPES)
def test_bloom_window_leaf(oracle, amq, torch, shape):
    """One 200,000-key leaf at 12 bits per key is 4,688 blocks, two LDS windows.  Alone, a leaf of
    16- or 24-byte keys would be tiled, so it stands beside small leaves, which keep it in the
    batch's window build."""
    counts = [200_000] + [65] * 70
    r, plan, *_ = build_and_compare(oracle, amq, torch, shape, counts, 12, 33)
    assert plan.max_seg_blocks == 4688
    assert r.route == amq.abi.ROUTE_WINDOW and r.windows == 2, (r.route, r.windows)


def one_filter_route(amq, n, bpk, stride):
    plan = amq.plan_filters(0, [n], bpk)
    return amq.filters.build_route(plan, stride, False)[0].route


@pytest.mark.parametrize("shape,bpk", [("k16", 10), ("k24", 10), ("k16", 12), ("k16", 20), ("k16", 6)])
def test_bloom_monolithic_smallest_tiled(oracle, amq, torch, shape, bpk):
    """One filter of the fewest keys that build_route sends to the tiled build (the route depends
    on the block count alone, which grows with the keys: a bisection finds the step)."""
    TK = amq.abi.ROUTE_TILED_KEYS
    stride = int(shape[1:])
    lo, hi = 1, 1 << 22
    assert one_filter_route(amq, lo, bpk, stride) != TK and one_filter_route(amq, hi, bpk, stride) == TK
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if one_filter_route(amq, mid, bpk, stride) == TK:
            hi = mid
        else:
            lo = mid
    n = hi
    assert one_filter_route(amq, n - 1, bpk, stride) != TK
    r, plan, out, keys, offs, ref = build_and_compare(oracle, amq, torch, shape, [n], bpk, 34)
    assert r.route == TK, r.route
    assert plan.max_seg_blocks * 64 > 160 * 1024   # past one LDS image
    if shape == "k16":
        assert_keys_separate_the_shift(oracle, keys[:4096], [bloom_seed(j) for j in range(HASHES[bpk])])


@pytest.mark.parametrize("n", [64, 1025])
def test_vqf_leaf(oracle, amq, torch, n):
    keys = sorted_keys(oracle, 35, [n])
    ref = oracle_per_segment(oracle, 1, keys, [n], 12)
    plan, out = gpu_build(amq, torch, 1, torch.from_numpy(keys).cuda(), [n], 12)
    r, _ = amq.filters.build_route(plan, 16, False)
    assert r.route == amq.abi.ROUTE_VQF_RING_PLACE, r.route
    assert_same(plan, out, ref)
    hv = amq.vqf_hash_val(amq.KeyBatch.fixed(torch.from_numpy(keys).cuda())).cpu().numpy().view(np.uint64)
    assert [int(x) for x in hv] == [xxh16(k.tobytes(), VQF_SEED) for k in keys]
    if n >= 64:
        assert_keys_separate_the_shift(oracle, keys, [VQF_SEED])
