"""GPU: tkv_amq_verify_members against the CPU oracle -- never against the code under test.

Expected values: for 16-byte keys oracle.probe_segments over the same (possibly damaged) filter
bytes; for other key shapes oracle.bloom_query / oracle.vqf_is_present(oracle.xxh64(key)) per
key.  Everywhere the existing tkv_amq_probe is asked the same (key, leaf) pairs as a cross-check.
Every damage case first asserts that the oracle itself expects missing keys in the damaged leaf.

Shapes: leaves of 0 .. 16,384 keys around the wave and workgroup edges in one batch; one
100,001-key Bloom leaf (its 125 KB image fits LDS, its keys are split over many units); one
150,000-key leaf (187 KB: the global-memory route) beside 300 small ones; the LDS hint as the
plan's value, 0 and 1."""
import numpy as np
import pytest

from turtle_kv_amd import abi

pytestmark = pytest.mark.gpu

BLOOM, VQF = 0, 1
U64 = (1 << 64) - 1
LEAVES = [0, 1, 63, 64, 65, 255, 256, 257, 1000, 16384, 8448]
# (kind, bits/key, payload capacity): Bloom k = 3, 7, 8, 11, 17; VQF 8-bit tags, 16-bit tags, and a
# capacity so small that hash_val_shift > 0
SETTINGS = [(BLOOM, 4, 0), (BLOOM, 10, 0), (BLOOM, 12, 0), (BLOOM, 16, 0), (BLOOM, 24, 0),
            (VQF, 12, 32704), (VQF, 22, 65472), (VQF, 12, 80 + 64 * 16)]
BLOOM_K = {4: 3, 10: 7, 12: 8, 16: 11, 24: 17}
SHAPES = ("k16", "k24", "k24off4", "s20", "var")
HINTS = ("plan", 0, 1)


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available()
    return t


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------------------------------
# keys of every shape (host rows / bytes, built once per (shape, n))
# ---------------------------------------------------------------------------------------
_host_keys = {}


def host_keys(oracle, shape, n):
    """(host array, offsets or None): k16 [n,16]; k24 / k24off4 [n,24]; s20 [n,20]; var: bytes of
    n keys of 8..40 bytes (both sides of XXH64's 32-byte split) and their n + 1 offsets."""
    key = (shape, n)
    if key not in _host_keys:
        a = oracle.gen_keys16(77, 0, max(n, 1))[:n]
        if shape == "k16":
            v = (a, None)
        else:
            b = oracle.gen_keys16(78, 0, max(n, 1))[:n]
            c = oracle.gen_keys16(79, 0, max(n, 1))[:n]
            wide = np.ascontiguousarray(np.concatenate([a, b, c], axis=1))  # [n, 48], unique rows
            if shape in ("k24", "k24off4"):
                v = (np.ascontiguousarray(wide[:, :24]), None)
            elif shape == "s20":
                v = (np.ascontiguousarray(wide[:, :20]), None)
            else:
                lens = np.random.default_rng(5).integers(8, 41, n)
                offs = np.zeros(n + 1, dtype=np.int64)
                np.cumsum(lens, out=offs[1:])
                mask = np.arange(48)[None, :] < lens[:, None]
                v = (np.ascontiguousarray(wide[mask]) if n else np.zeros(1, np.uint8), offs)
        _host_keys[key] = v
    return _host_keys[key]


def key_bytes(shape, hk, offs, i):
    return hk[i].tobytes() if offs is None else hk[int(offs[i]):int(offs[i + 1])].tobytes()


def key_batch(amq, torch, shape, hk, offs):
    if shape == "var":
        return amq.KeyBatch.variable(dev(torch, hk), dev(torch, offs))
    if shape == "k24off4":  # the rows at a base pointer 4 bytes past an aligned one: not the 24-byte fast mode
        buf = torch.zeros(hk.size + 16, dtype=torch.uint8, device="cuda")
        rows = buf[4:4 + hk.size].view(hk.shape[0], 24)
        rows.copy_(torch.from_numpy(hk))
        assert rows.data_ptr() % 8 == 4 and rows.is_contiguous()
        return amq.KeyBatch.fixed(rows)
    return amq.KeyBatch.fixed(dev(torch, hk))


# ---------------------------------------------------------------------------------------
# the call, and the expectations
# ---------------------------------------------------------------------------------------
def run(amq, torch, plan, filt, kb, key_begin=None, hint="plan"):
    """tkv_amq_verify_members through the raw launch: (MEMBER_CHECK_DTYPE[n_segs], total)."""
    n = plan.n_segs
    res = torch.full((max(n, 1) * 16,), 0xAB, dtype=torch.uint8, device="cuda")   # (the call initialises)
    tot = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    ws = torch.empty(amq.verify_members_workspace_bytes(n), dtype=torch.uint8, device="cuda")
    d_kb = None if key_begin is None else dev(torch, np.asarray(key_begin, dtype=np.uint64).view(np.int64))
    amq.verify_members_device(plan.kind, filt, plan.device_segs(), n, plan.max_seg_blocks if hint == "plan" else hint,
                              kb.data, kb.offsets, kb.stride, kb.n, d_kb, res, tot, ws)
    torch.cuda.synchronize()
    return res[:16 * n].cpu().numpy().view(abi.MEMBER_CHECK_DTYPE).copy(), int(tot.item())


def clamped_ranges(plan, n_keys, key_begin=None):
    """include/tkv_amq.h: both ends clamped to n_keys, an end below its begin reads as empty."""
    if key_begin is None:
        lo = plan.segs["key_begin"].astype(object)
        hi = lo + plan.segs["n_keys"].astype(object)
    else:
        kb = [int(x) for x in key_begin]
        lo, hi = np.array(kb[:-1], dtype=object), np.array(kb[1:], dtype=object)
    out = []
    for b, e in zip(lo, hi):
        b, e = min(int(b), n_keys), min(int(e), n_keys)
        out.append((b, max(b, e)))
    return out


def pairs(ranges):
    idx = np.concatenate([np.arange(b, e, dtype=np.int64) for b, e in ranges] + [np.zeros(0, np.int64)])
    seg = np.repeat(np.arange(len(ranges)), [e - b for b, e in ranges]).astype(np.uint32)
    return idx, seg


def fold(n_segs, idx, seg, present):
    """Per-leaf (missing, first_missing) from the answer of every (key idx[i], leaf seg[i]) pair."""
    rej = np.asarray(present) == 0
    missing = np.bincount(seg[rej], minlength=n_segs).astype(np.uint32)
    first = np.full(n_segs, U64, dtype=np.uint64)
    np.minimum.at(first, seg[rej], idx[rej].astype(np.uint64))
    return missing, first


def expect16(oracle, plan, host, keys16, ranges):
    idx, seg = pairs(ranges)
    st, res = oracle.probe_segments(plan.kind, host, plan.segs["out_offset"], np.ascontiguousarray(keys16[idx]), seg)
    assert st == 0
    return fold(plan.n_segs, idx, seg, res)


def expect_per_key(oracle, plan, host, shape, hk, offs, ranges, leaves):
    """The oracle's per-key answer, on the leaves listed (the small ones)."""
    idx, seg, res = [], [], []
    for s in leaves:
        sg = plan.segs[s]
        payload = np.ascontiguousarray(host[int(sg["out_offset"]):int(sg["out_offset"]) + int(sg["payload_bytes"])])
        for i in range(*ranges[s]):
            k = key_bytes(shape, hk, offs, i)
            r = oracle.bloom_query(payload, k) if plan.kind == BLOOM else \
                oracle.vqf_is_present(payload, oracle.xxh64(k, oracle.VQF_HASH_SEED))
            idx.append(i), seg.append(s), res.append(r)
    return fold(plan.n_segs, np.asarray(idx, np.int64), np.asarray(seg, np.uint32), np.asarray(res))


def probe_fold(amq, torch, plan, filt, kb, ranges):
    """The existing tkv_amq_probe over the same pairs (fixed-stride keys, or every key in order)."""
    idx, seg = pairs(ranges)
    if len(idx) == 0:
        return fold(plan.n_segs, idx, seg, np.zeros(0))
    if kb.offsets is None:
        q = amq.KeyBatch.fixed(kb.data[dev(torch, idx)].contiguous())
    else:
        assert np.array_equal(idx, np.arange(kb.n))
        q = kb
    res = amq.probe_filters(plan, filt, q, dev(torch, seg.astype(np.int32))).cpu().numpy()
    return fold(plan.n_segs, idx, seg, res)


def assert_result(got, total, missing, first, flags=0, leaves=None):
    sel = slice(None) if leaves is None else list(leaves)
    assert np.array_equal(got["missing"][sel], missing[sel])
    assert np.array_equal(got["first_missing"][sel], first[sel])
    if flags is not None:
        assert np.array_equal(got["flags"][sel], np.broadcast_to(np.asarray(flags, np.uint32), got["flags"].shape)[sel])
    if leaves is None:
        assert total == int(missing.sum())


def build(amq, torch, kind, bpk, cap, counts, kb, pages=False, src0=900):
    src = np.arange(src0, src0 + len(counts), dtype=np.uint64)
    if pages:
        packed = amq.plan_filters(kind, counts, bpk, payload_capacity=cap, src_page_ids=src)
        log2 = int(64 + (cap if kind == VQF else int(packed.segs["payload_bytes"].max())) - 1).bit_length()
        plan = amq.plan_filter_pages(kind, counts, bpk, log2, src_page_ids=src)
    else:
        plan = amq.plan_filters(kind, counts, bpk, payload_capacity=cap, src_page_ids=src)
    filt = torch.zeros(max(plan.total_out_bytes, 16), dtype=torch.uint8, device="cuda")
    amq.build_all_filters(plan, kb, out=filt)
    torch.cuda.synchronize()
    return plan, filt


_built16 = {}


def built16(oracle, amq, torch, kind, bpk, cap, counts=None):
    """One clean build of 16-byte keys per setting, shared (and left unchanged) by the damage,
    CSR and capture tests: (plan, device filters, host copy, host keys, KeyBatch)."""
    counts = LEAVES if counts is None else counts
    key = (kind, bpk, cap, tuple(counts))
    if key not in _built16:
        hk, _ = host_keys(oracle, "k16", sum(counts))
        kb = key_batch(amq, torch, "k16", hk, None)
        plan, filt = build(amq, torch, kind, bpk, cap, counts, kb)
        _built16[key] = (plan, filt, filt.cpu().numpy(), hk, kb)
    return _built16[key]


# ---------------------------------------------------------------------------------------
# 1. clean builds -> all zero
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("kind,bpk,cap", SETTINGS)
def test_clean_build_is_all_zero(oracle, amq, torch, kind, bpk, cap, shape):
    hk, offs = host_keys(oracle, shape, sum(LEAVES))
    kb = key_batch(amq, torch, shape, hk, offs)
    plan, filt = build(amq, torch, kind, bpk, cap, LEAVES, kb)
    if kind == BLOOM:
        assert int(plan.segs["hash_count"][-1]) == BLOOM_K[bpk]
    else:
        assert int(plan.segs["tag_bits"][-1]) == (16 if bpk == 22 else 8)
        assert (int(plan.segs["hash_val_shift"].max()) > 0) == (cap < 32704)
    zero_m, none = np.zeros(len(LEAVES), np.uint32), np.full(len(LEAVES), U64, np.uint64)
    for hint in HINTS:
        got, total = run(amq, torch, plan, filt, kb, hint=hint)
        assert_result(got, total, zero_m, none, flags=0)
    # the existing probe agrees, and so does the oracle's per-key answer on the small leaves
    ranges = clamped_ranges(plan, kb.n)
    pm, pf = probe_fold(amq, torch, plan, filt, kb, ranges)
    assert not pm.any() and (pf == U64).all()
    small = [s for s, c in enumerate(LEAVES) if c <= 257]
    em, ef = expect_per_key(oracle, plan, filt.cpu().numpy(), shape, hk, offs, ranges, small)
    assert not em.any() and (ef == U64).all()
    # the host mirror returns the same records
    assert np.array_equal(amq.verify_members(plan, filt, kb), got)


@pytest.mark.parametrize("kind,bpk,cap", [(BLOOM, 10, 0), (VQF, 12, 32704)])
def test_page_image_plan_is_all_zero(oracle, amq, torch, kind, bpk, cap):
    hk, _ = host_keys(oracle, "k16", sum(LEAVES))
    kb = key_batch(amq, torch, "k16", hk, None)
    plan, filt = build(amq, torch, kind, bpk, cap, LEAVES, kb, pages=True)
    assert (plan.segs["page_flags"] & abi.PAGE_IMAGE).all()
    got, total = run(amq, torch, plan, filt, kb)
    assert_result(got, total, np.zeros(len(LEAVES), np.uint32), np.full(len(LEAVES), U64, np.uint64), flags=0)


@pytest.mark.parametrize("kind", [BLOOM, VQF])
def test_no_filter_plan(oracle, amq, torch, kind):
    hk, _ = host_keys(oracle, "k16", sum(LEAVES))
    kb = key_batch(amq, torch, "k16", hk, None)
    plan, filt = build(amq, torch, kind, 0, 32704 if kind == VQF else 0, LEAVES, kb)
    got, total = run(amq, torch, plan, filt, kb)
    assert_result(got, total, np.zeros(len(LEAVES), np.uint32), np.full(len(LEAVES), U64, np.uint64),
                  flags=abi.VERIFY_NO_FILTER)


def test_empty_batch(amq, torch):
    tot = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    amq.verify_members_device(BLOOM, None, None, 0, 0, None, None, 16, 0, None, None, tot, None)
    torch.cuda.synchronize()
    assert int(tot.item()) == 0
    amq.verify_members_device(VQF, None, None, 0, 0, None, None, 16, 0, None, None, None, None)


# ---------------------------------------------------------------------------------------
# 2. Bloom damage
# ---------------------------------------------------------------------------------------
def check_damaged16(oracle, amq, torch, plan, filt, hk, kb, damaged, key_begin=None, flags=0, hints=HINTS):
    ranges = clamped_ranges(plan, kb.n, key_begin)
    em, ef = expect16(oracle, plan, filt.cpu().numpy(), hk, ranges)
    for s in damaged:
        assert em[s] > 0, f"the oracle expects missing keys in damaged leaf {s}"
    pm, pf = probe_fold(amq, torch, plan, filt, kb, ranges)
    assert np.array_equal(pm, em) and np.array_equal(pf, ef), "tkv_amq_probe and the oracle agree"
    first = None
    for hint in hints:
        got, total = run(amq, torch, plan, filt, kb, key_begin=key_begin, hint=hint)
        assert_result(got, total, em, ef, flags=flags)
        assert first is None or first == got.tobytes(), "the LDS hint does not change the result"
        first = got.tobytes()
    return em, ef


@pytest.mark.parametrize("bpk", [10, 12, 16])
def test_bloom_damage(oracle, amq, torch, bpk):
    plan, clean, host, hk, kb = built16(oracle, amq, torch, BLOOM, bpk, 0)
    bad = host.copy()
    a, b = LEAVES.index(16384), LEAVES.index(1000)
    sa, sb = plan.segs[a], plan.segs[b]
    # leaf a: the first half of its blocks zeroed
    o = int(sa["out_offset"]) + 64
    bad[o:o + 64 * (int(sa["n_blocks"]) // 2)] = 0
    # leaf b: one set bit cleared
    blocks = bad[int(sb["out_offset"]) + 64:int(sb["out_offset"]) + 64 + 64 * int(sb["n_blocks"])]
    byte = int(np.flatnonzero(blocks)[7])
    blocks[byte] &= np.uint8(~(1 << (int(blocks[byte]).bit_length() - 1)) & 0xFF)
    em, _ = check_damaged16(oracle, amq, torch, plan, dev(torch, bad), hk, kb, damaged=[a, b])
    assert not em[[s for s in range(len(LEAVES)) if s not in (a, b)]].any()     # untouched leaves are zero
    assert 0.3 * 16384 < em[a] < 0.7 * 16384


# ---------------------------------------------------------------------------------------
# 3. VQF damage
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("bpk,cap", [(12, 32704), (22, 65472)])
def test_vqf_damage(oracle, amq, torch, bpk, cap):
    plan, clean, host, hk, kb = built16(oracle, amq, torch, VQF, bpk, cap)
    bad = host.copy()
    a, b = LEAVES.index(16384), LEAVES.index(8448)
    md = 16 if bpk == 12 else 8
    # leaf a: the tag bytes of one block zeroed; leaf b: the metadata of one block (in mid-filter)
    blk_a = int(plan.segs[a]["out_offset"]) + 80 + 64 * (int(plan.segs[a]["n_blocks"]) // 3)
    bad[blk_a + md:blk_a + 64] = 0
    blk_b = int(plan.segs[b]["out_offset"]) + 80 + 64 * (int(plan.segs[b]["n_blocks"]) // 2)
    bad[blk_b:blk_b + md] = 0
    em, _ = check_damaged16(oracle, amq, torch, plan, dev(torch, bad), hk, kb, damaged=[a, b])
    assert not em[[s for s in range(len(LEAVES)) if s not in (a, b)]].any()


# ---------------------------------------------------------------------------------------
# 4. swapped leaves
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,bpk,cap", [(BLOOM, 10, 0), (VQF, 12, 32704)])
def test_swapped_leaves(oracle, amq, torch, kind, bpk, cap):
    counts = [3000, 500, 3000, 77]
    plan, clean, host, hk, kb = built16(oracle, amq, torch, kind, bpk, cap, counts)
    s0, s2 = plan.segs[0], plan.segs[2]
    assert s0["n_blocks"] == s2["n_blocks"] and s0["payload_bytes"] == s2["payload_bytes"]
    n = int(s0["payload_bytes"])
    bad = host.copy()
    o0, o2 = int(s0["out_offset"]), int(s2["out_offset"])
    bad[o0:o0 + n], bad[o2:o2 + n] = host[o2:o2 + n], host[o0:o0 + n]
    flags = np.array([abi.VERIFY_ID_MISMATCH, 0, abi.VERIFY_ID_MISMATCH, 0], np.uint32)
    em, _ = check_damaged16(oracle, amq, torch, plan, dev(torch, bad), hk, kb, damaged=[0, 2], flags=flags)
    assert em[0] > 0.9 * 3000 and em[2] > 0.9 * 3000 and em[1] == 0 and em[3] == 0


# ---------------------------------------------------------------------------------------
# 5. d_key_begin
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,bpk,cap", [(BLOOM, 10, 0), (VQF, 12, 32704)])
def test_opened_filters_with_key_begin(oracle, amq, torch, kind, bpk, cap):
    plan, filt, host, hk, kb = built16(oracle, amq, torch, kind, bpk, cap)
    opened = amq.open_filters(kind, filt, offsets=plan.segs["out_offset"])
    assert opened.all_ok and not opened.plan.segs["key_begin"].any()
    n_keys, n = kb.n, len(LEAVES)
    csr = np.concatenate([[0], np.cumsum(LEAVES)]).astype(np.uint64)
    # the true CSR: all zero (through the host mirror too, which takes the OpenedFilters)
    got, total = run(amq, torch, opened.plan, filt, kb, key_begin=csr)
    assert_result(got, total, np.zeros(n, np.uint32), np.full(n, U64, np.uint64), flags=0)
    assert np.array_equal(amq.verify_members(opened, filt, kb, key_begin=csr), got)
    # shifted by one leaf: leaf s is asked about its neighbour's keys
    shifted = np.concatenate([csr[1:], [n_keys]]).astype(np.uint64)
    big = LEAVES.index(16384) - 1   # (the leaf that is now asked about the 16,384-key leaf's keys)
    em, _ = check_damaged16(oracle, amq, torch, opened.plan, filt, hk, kb, damaged=[big], key_begin=shifted)
    assert em[big] > 0.5 * 16384
    # malformed: an end below its begin, entries past n_keys
    bad = csr.copy()
    bad[3] = bad[5] + 10            # leaf 2's end > leaf 3's begin .. leaf 3: end below begin (empty)
    bad[-1] = n_keys + 12345        # the last leaf's end is clamped
    bad[-2] = U64                   # its begin too: empty; the leaf before it runs to n_keys
    ranges = clamped_ranges(opened.plan, n_keys, bad)
    assert ranges[3][0] == ranges[3][1] and ranges[-1] == (n_keys, n_keys) and ranges[-2][1] == n_keys
    check_damaged16(oracle, amq, torch, opened.plan, filt, hk, kb, damaged=[], key_begin=bad)


def test_plan_ranges_are_clamped(oracle, amq, torch):
    """Without d_key_begin the segments' own ranges are clamped to n_keys the same way."""
    plan, filt, host, hk, kb = built16(oracle, amq, torch, BLOOM, 10, 0)
    short = amq.KeyBatch.fixed(kb.data[:10000].contiguous())
    ranges = clamped_ranges(plan, 10000)    # the 16,384-key leaf is cut short, the last leaf is empty
    assert ranges[-1] == (10000, 10000) and ranges[-2] == (int(plan.segs["key_begin"][-2]), 10000)
    em, ef = expect16(oracle, plan, host, hk, ranges)
    got, total = run(amq, torch, plan, filt, short)
    assert_result(got, total, em, ef, flags=0)
    assert total == 0


# ---------------------------------------------------------------------------------------
# large and uneven batches: units of one leaf over many workgroups, the global-memory route
# ---------------------------------------------------------------------------------------
BIG = [("lds", [100_001]), ("global_uneven", [150_000] + [1 + (37 * i) % 600 for i in range(300)])]


@pytest.mark.parametrize("name,counts", BIG, ids=[b[0] for b in BIG])
@pytest.mark.parametrize("shape", ["k16", "k24"])
def test_big_bloom_leaf(oracle, amq, torch, name, counts, shape):
    hk, offs = host_keys(oracle, shape, sum(counts))
    kb = key_batch(amq, torch, shape, hk, offs)
    plan, filt = build(amq, torch, BLOOM, 10, 0, counts, kb)
    assert (64 * int(plan.segs["n_blocks"][0]) <= 160 * 1024) == (name == "lds")
    n = len(counts)
    for hint in HINTS:
        got, total = run(amq, torch, plan, filt, kb, hint=hint)
        assert_result(got, total, np.zeros(n, np.uint32), np.full(n, U64, np.uint64), flags=0)
    # damage: the big leaf's second half zeroed, one small leaf's blocks zeroed
    bad = filt.cpu().numpy().copy()
    o, nb = int(plan.segs[0]["out_offset"]) + 64, int(plan.segs[0]["n_blocks"])
    bad[o + 64 * (nb // 2):o + 64 * nb] = 0
    damaged = [0]
    if n > 1:
        sg = plan.segs[n - 1]
        bad[int(sg["out_offset"]) + 64:int(sg["out_offset"]) + int(sg["payload_bytes"])] = 0
        damaged.append(n - 1)
    d_bad = dev(torch, bad)
    ranges = clamped_ranges(plan, kb.n)
    if shape == "k16":
        em, ef = check_damaged16(oracle, amq, torch, plan, d_bad, hk, kb, damaged=damaged)
    else:
        # 24-byte keys: the oracle per key on the small damaged leaf and on a slice of the big one
        probe_m, probe_f = probe_fold(amq, torch, plan, d_bad, kb, ranges)
        got, total = run(amq, torch, plan, d_bad, kb)
        assert_result(got, total, probe_m, probe_f, flags=0)
        em = probe_m
        if n > 1:
            om, of = expect_per_key(oracle, plan, bad, shape, hk, offs, ranges, [n - 1])
            assert om[n - 1] > 0
            assert_result(got, total, om, of, flags=0, leaves=[n - 1])
        sl = [(0, 0)] * n
        sl[0] = (40_000, 41_000)
        om, _ = expect_per_key(oracle, plan, bad, shape, hk, offs, sl, [0])
        pm, _ = probe_fold(amq, torch, plan, d_bad, kb, sl)
        assert om[0] > 0 and om[0] == pm[0]
    assert 0.3 * counts[0] < em[0] < 0.7 * counts[0]


# More leaves than the 1,024 threads of the workgroup that turns the leaves' unit counts into
# their prefix (prefix_inclusive_u64, turtle_kv_amd/csrc/tkv_amq_scan.h): a thread's serial run is
# 1, 2 and 3 elements, with idle threads at the end in the last two.  A unit past the first
# 1,024 leaves finds its own leaf through that prefix: the damage is reported on the damaged
# leaves and nowhere else.
@pytest.mark.parametrize("n_leaves", [1024, 1025, 2100])
@pytest.mark.parametrize("kind,bpk,cap", [(BLOOM, 10, 0), (VQF, 12, 32704)])
def test_more_leaves_than_prefix_threads(oracle, amq, torch, kind, bpk, cap, n_leaves):
    counts = [1 + (37 * i) % 9 for i in range(n_leaves)]
    hk, _ = host_keys(oracle, "k16", sum(counts))
    kb = key_batch(amq, torch, "k16", hk, None)
    plan, filt = build(amq, torch, kind, bpk, cap, counts, kb)
    zero_m, none = np.zeros(n_leaves, np.uint32), np.full(n_leaves, U64, np.uint64)
    for hint in HINTS:
        got, total = run(amq, torch, plan, filt, kb, hint=hint)
        assert_result(got, total, zero_m, none, flags=0)
    # the blocks of leaf 1,024 (where it exists) and of the last leaf zeroed
    damaged = sorted({n_leaves - 1} | ({1024} if n_leaves > 1024 else set()))
    bad = filt.cpu().numpy().copy()
    for s in damaged:
        o = int(plan.segs[s]["out_offset"]) + (64 if kind == BLOOM else 80)
        bad[o:o + 64 * int(plan.segs[s]["n_blocks"])] = 0
    em, _ = check_damaged16(oracle, amq, torch, plan, dev(torch, bad), hk, kb, damaged=damaged)
    assert list(np.flatnonzero(em)) == damaged


# ---------------------------------------------------------------------------------------
# 6. determinism and graph capture
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,bpk,cap", [(BLOOM, 10, 0), (VQF, 12, 32704)])
def test_deterministic_and_capturable(oracle, amq, torch, kind, bpk, cap):
    plan, clean, host, hk, kb = built16(oracle, amq, torch, kind, bpk, cap)
    a = LEAVES.index(16384)
    bad = host.copy()
    o = int(plan.segs[a]["out_offset"]) + (64 if kind == BLOOM else 80)
    bad[o:o + 64 * (int(plan.segs[a]["n_blocks"]) // 2)] = 0
    ranges = clamped_ranges(plan, kb.n)
    em, ef = expect16(oracle, plan, bad, hk, ranges)
    assert em[a] > 0
    d_bad = dev(torch, bad)
    r1, t1 = run(amq, torch, plan, d_bad, kb)
    r2, t2 = run(amq, torch, plan, d_bad, kb)
    assert r1.tobytes() == r2.tobytes() and t1 == t2 == int(em.sum())
    # capture on the clean filters, damage them in place, replay
    n = plan.n_segs
    filt = clean.clone()
    res = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    tot = torch.zeros(1, dtype=torch.int64, device="cuda")
    ws = torch.empty(amq.verify_members_workspace_bytes(n), dtype=torch.uint8, device="cuda")
    segs = plan.device_segs()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # (warm-up outside the capture: kernel attributes, module load)
        amq.verify_members_device(kind, filt, segs, n, plan.max_seg_blocks, kb.data, None, 16, kb.n, None, res,
                                  tot, ws, stream=side)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        amq.verify_members_device(kind, filt, segs, n, plan.max_seg_blocks, kb.data, None, 16, kb.n, None, res,
                                  tot, ws, stream=torch.cuda.current_stream())
    g.replay()
    torch.cuda.synchronize()
    got = res.cpu().numpy().view(abi.MEMBER_CHECK_DTYPE)
    assert not got["missing"].any() and int(tot.item()) == 0
    filt.copy_(d_bad)
    g.replay()
    torch.cuda.synchronize()
    got = res.cpu().numpy().view(abi.MEMBER_CHECK_DTYPE)
    assert_result(got, int(tot.item()), em, ef, flags=0)
