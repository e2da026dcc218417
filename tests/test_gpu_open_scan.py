"""GPU: tkv_amq_open_filters and tkv_amq_scan_filters against the CPU oracle and the numpy
restatement of tests/test_open_scan_abi.py -- never against the code under test.

Round trip (build with a plan, open the bytes in each location form, same segments, same probe
answers as the plan and the oracle), refusal (one corruption per copy, its documented code for
that filter only), scan (stats equal to numpy's over the oracle's bytes; a broken VQF block is
counted), graph capture and the host mirrors."""
import numpy as np
import pytest

from test_open_scan_abi import (BLOOM, BLOOM_BIG, BLOOM_MAGIC, LEAF_COUNTS, SETTINGS, VQF, VQF_BIG,
                                VQF_MAGIC, ref_open, ref_scan, ref_vqf_blocks)
from turtle_kv_amd import abi

pytestmark = pytest.mark.gpu

FORMS = ("offsets", "stride", "pages")
# every setting with the six leaf counts (the 10 bits/key Bloom batch also holds the leaf that
# spans several scan chunks), and the VQF leaf that fills its page in a batch of its own
BATCHES = [(k, b, LEAF_COUNTS + ([BLOOM_BIG] if (k, b) == (BLOOM, 10) else [])) for k, b, c in SETTINGS] + \
    [(VQF, 12, [VQF_BIG])]
CAP = {(k, b): c for k, b, c in SETTINGS}
SEG_FIELDS = ("out_offset", "n_blocks", "hash_count", "tag_bits", "hash_val_shift", "mod_magic",
              "src_page_id", "payload_bytes", "page_flags")
STAT_FIELDS = ("occupied", "header_items", "full_blocks", "empty_blocks", "max_block", "bad_blocks")


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available()
    return t


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_keys = {}


def batch_keys(oracle, kind, counts):
    """The batch's keys (sorted inside each leaf for VQF, whose build replays the leaf's order),
    ~4,000 queries -- hits from every leaf and misses -- and the leaf each one asks (a batch of
    thousands of leaves has more hits than that and no misses; its tests do not use the queries)."""
    key = (kind, tuple(counts))
    if key not in _keys:
        bounds = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
        keys = oracle.gen_keys16(77, 0, sum(counts))
        if kind == VQF:
            oracle.sort_segments(keys, bounds)
        rng = np.random.default_rng(3)
        hit_idx, hit_seg = [], []
        for s, c in enumerate(counts):
            take = min(c, 300)
            hit_idx.append(int(bounds[s]) + rng.choice(c, take, replace=False) if take else np.zeros(0, np.int64))
            hit_seg.append(np.full(take, s))
        hit_idx, hit_seg = np.concatenate(hit_idx).astype(np.int64), np.concatenate(hit_seg)
        n_miss = max(4000 - len(hit_idx), 0)     # (a batch of thousands of leaves: hits only)
        q = np.concatenate([keys[hit_idx], oracle.gen_keys16(78, 0, n_miss)])
        qs = np.concatenate([hit_seg, rng.integers(0, len(counts), n_miss)]).astype(np.uint32)
        _keys[key] = (keys, bounds, q, qs)
    return _keys[key]


def make_plan(amq, kind, bpk, counts, form):
    cap = CAP[(kind, bpk)]
    src = np.arange(700, 700 + len(counts), dtype=np.uint64)
    packed = amq.plan_filters(kind, counts, bpk, payload_capacity=cap, src_page_ids=src)
    if form == "offsets":
        return packed, dict(offsets=packed.segs["out_offset"])
    if form == "stride":
        stride = cap if kind == VQF else (int(packed.segs["payload_bytes"].max()) + 63) // 64 * 64
        return (amq.plan_filters(kind, counts, bpk, payload_capacity=cap, out_stride=stride, src_page_ids=src),
                dict(stride=stride))
    log2 = int(64 + (cap if kind == VQF else int(packed.segs["payload_bytes"].max())) - 1).bit_length()
    return amq.plan_filter_pages(kind, counts, bpk, log2, src_page_ids=src), dict(page_size_log2=log2)


def build(oracle, amq, torch, kind, bpk, counts, form):
    """(plan, open arguments, device bytes, the oracle's bytes at the plan's offsets)."""
    keys, bounds, _, _ = batch_keys(oracle, kind, counts)
    plan, where = make_plan(amq, kind, bpk, counts, form)
    filt = torch.zeros(plan.total_out_bytes, dtype=torch.uint8, device="cuda")
    amq.build_all_filters(plan, amq.KeyBatch.fixed(dev(torch, keys)), out=filt)
    host = filt.cpu().numpy()
    cap = plan.segs["payload_bytes"].astype(np.uint64) if kind == BLOOM else \
        np.full(len(counts), CAP[(kind, bpk)], np.uint64)
    ref = host.copy()
    for sg in plan.segs:  # the oracle writes its own payloads over the copy
        ref[int(sg["out_offset"]):int(sg["out_offset"]) + int(sg["payload_bytes"])] = 0
    st, ref = oracle.build_segments(kind, keys, bounds, bpk, plan.segs["out_offset"], cap, len(ref),
                                    src_page_id=np.ascontiguousarray(plan.segs["src_page_id"]), out=ref)
    assert st == 0
    return plan, where, filt, ref


def all_probes(amq, torch, plan, filt, q, qs):
    """The answers of every probe family for the pairs (q[i], leaf qs[i])."""
    kb = amq.KeyBatch.fixed(dev(torch, q))
    dqs = dev(torch, qs.astype(np.int32))
    out = {"probe": amq.probe_filters(plan, filt, kb, dqs)}
    if plan.kind == BLOOM:
        out["hashed"] = amq.bloom_probe_hashed(plan, filt, amq.bloom_query_hashes(kb, 32), 32, dqs)
    else:
        out["hashed"] = amq.vqf_probe_hashed(plan, filt, amq.vqf_hash_val(kb), dqs)
    pb = dev(torch, np.arange(len(q) + 1, dtype=np.int32))
    out["paths"] = amq.probe_paths(plan, filt, kb, pb, dqs, entry_result=True).entry_result
    return {k: v.cpu().numpy() for k, v in out.items()}


# ---------------------------------------------------------------------------------------
# 1. round trip
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("kind,bpk,counts", BATCHES, ids=lambda v: str(v) if not isinstance(v, list) else f"n{len(v)}")
def test_round_trip(oracle, amq, torch, kind, bpk, counts, form):
    plan, where, filt, ref = build(oracle, amq, torch, kind, bpk, counts, form)
    assert np.array_equal(filt.cpu().numpy(), ref), "the built bytes are the oracle's"
    opened = amq.open_filters(kind, filt, n_filters=len(counts), **where)
    assert list(opened.status) == [abi.OPEN_OK] * len(counts)
    assert list(opened.summary) == [len(counts), 0, 0, 0, 0, 0, 0] and opened.all_ok
    for name in SEG_FIELDS:
        assert np.array_equal(opened.plan.segs[name], plan.segs[name]), name
    for name in ("bits_per_key", "key_begin", "block_base"):
        assert not opened.plan.segs[name].any(), name
    shift0 = plan.segs["hash_val_shift"] == 0
    assert np.array_equal(opened.plan.segs["n_keys"][shift0], plan.segs["n_keys"][shift0])
    assert opened.plan.max_seg_blocks == plan.max_seg_blocks
    assert opened.plan.total_out_bytes == filt.numel() and opened.plan.workspace_bytes == 0
    # the restatement reads the same segments from the oracle's bytes
    for s in range(len(counts)):
        code, f = ref_open(kind, ref, s, **where)
        assert code == abi.OPEN_OK
        for name in SEG_FIELDS + ("n_keys",):
            assert f[name] == int(opened.plan.segs[name][s]), (name, s)
    if kind == VQF and counts == [VQF_BIG]:
        assert plan.segs["hash_val_shift"][0] == 1 and 0 < opened.plan.segs["n_keys"][0] < VQF_BIG
    # every probe family: opened plan == built plan == oracle
    _, _, q, qs = batch_keys(oracle, kind, counts)
    st, want = oracle.probe_segments(kind, ref, plan.segs["out_offset"], q, qs)
    assert st == 0 and 0 < int(want.sum()) < len(want)
    a, b = all_probes(amq, torch, opened.plan, filt, q, qs), all_probes(amq, torch, plan, filt, q, qs)
    for family in a:
        assert np.array_equal(a[family], b[family]), family
        assert np.array_equal(a[family], want), family


# ---------------------------------------------------------------------------------------
# 2. refusal
# ---------------------------------------------------------------------------------------
def put64(buf, off, v):
    buf[off:off + 8] = np.frombuffer(np.uint64(v).tobytes(), dtype=np.uint8)


def get64(buf, off):
    return int(np.frombuffer(bytes(buf[off:off + 8]), dtype="<u8")[0])


def corruptions(kind, ref, plan, where, form, victim):
    """(name, bytes, open arguments, documented code) for buffers in `form`."""
    off = int(plan.segs["out_offset"][victim])
    out = []

    def case(name, code, edit=None, args=None, total=None):
        b = ref.copy()
        if edit:
            edit(b)
        out.append((name, b if total is None else b[:total], dict(where, **(args or {})), code))

    if form == "offsets":
        case("magic zeroed", abi.OPEN_BAD_MAGIC, lambda b: put64(b, off, 0))
        case("other kind's magic", abi.OPEN_WRONG_KIND,
             lambda b: put64(b, off, VQF_MAGIC if kind == BLOOM else BLOOM_MAGIC))
        offs = plan.segs["out_offset"].copy()
        offs[victim] = 8
        case("offset 8", abi.OPEN_MISALIGNED, args=dict(offsets=offs))
        if kind == BLOOM:
            case("hash_count 0", abi.OPEN_BAD_GEOMETRY, lambda b: b.__setitem__(slice(off + 44, off + 46), 0))
            case("hash_count 33", abi.OPEN_BAD_GEOMETRY,
                 lambda b: b.__setitem__(slice(off + 44, off + 46), [33, 0]))
            case("bit_count off by 512", abi.OPEN_BAD_GEOMETRY, lambda b: put64(b, off + 8, get64(b, off + 8) + 512))
        else:
            case("key_remainder_bits 7", abi.OPEN_BAD_GEOMETRY, lambda b: put64(b, off + 40, 7))
            case("hash_mask with a hole", abi.OPEN_BAD_GEOMETRY, lambda b: put64(b, off + 24, 0xFFFFFFFFFFFFFFF5))
    elif form == "stride":
        if kind == BLOOM:
            # twice the blocks no longer fit the victim's slot (the largest leaf's payload)
            case("block_count doubled", abi.OPEN_OUT_OF_BOUNDS,
                 lambda b: b.__setitem__(slice(off + 40, off + 44), np.frombuffer(
                     np.uint32(2 * int(plan.segs["n_blocks"][victim])).tobytes(), dtype=np.uint8)))
        else:
            # one more block still fits the page-sized slot, and disagrees with total_size_in_bytes
            case("nblocks + 1", abi.OPEN_BAD_GEOMETRY, lambda b: put64(b, off + 56, get64(b, off + 56) + 1))
    else:
        page = off - 64
        case("wrong layout_id", abi.OPEN_BAD_PAGE, lambda b: b.__setitem__(page + 16, b[page + 16] ^ 1))
    return out


@pytest.mark.parametrize("kind,bpk", [(BLOOM, 10), (VQF, 12)])
def test_refusal(oracle, amq, torch, kind, bpk):
    counts = LEAF_COUNTS
    _, _, q, qs = batch_keys(oracle, kind, counts)
    seen = set()
    for form in FORMS:
        plan, where, filt, ref = build(oracle, amq, torch, kind, bpk, counts, form)
        st, want = oracle.probe_segments(kind, ref, plan.segs["out_offset"], q, qs)
        assert st == 0
        cases = corruptions(kind, ref, plan, where, form, victim=0)
        if form == "offsets":
            # the last slot truncated below the header size
            last = len(counts) - 1
            cases.append(("truncated", ref[:int(plan.segs["out_offset"][last]) + 48], where,
                          abi.OPEN_OUT_OF_BOUNDS))
        for name, bad, args, code in cases:
            victim = len(counts) - 1 if name == "truncated" else 0
            d_bad = dev(torch, bad)
            opened = amq.open_filters(kind, d_bad, n_filters=len(counts), **args)
            expect = [abi.OPEN_OK] * len(counts)
            expect[victim] = code
            assert list(opened.status) == expect, name
            # the restatement gives the same code from the bytes
            assert [ref_open(kind, bad, s, **args)[0] for s in range(len(counts))] == expect, name
            assert int(opened.summary.sum()) == len(counts), name
            assert int(opened.summary[code]) == 1 and int(opened.summary[abi.OPEN_OK]) == len(counts) - 1, name
            sg = opened.plan.segs[victim]
            assert sg["hash_count"] == 0 and sg["tag_bits"] == 0 and sg["n_blocks"] == 0 and sg["payload_bytes"] == 0
            # probing: the refused filter cannot reject and counts as "no filter page"; its
            # neighbours answer as before
            pm = amq.ProbeMetrics()
            got = amq.probe_filters(opened.plan, d_bad, amq.KeyBatch.fixed(dev(torch, q)),
                                    dev(torch, qs.astype(np.int32)), metrics=pm).cpu().numpy()
            mine = qs == victim
            assert mine.any() and got[mine].all(), name
            assert np.array_equal(got[~mine], want[~mine]), name
            assert pm.collect()["no_filter_page_count"] == int(mine.sum()), name
            seen.add(name)
    assert len(seen) == (9 if kind == BLOOM else 8)


# ---------------------------------------------------------------------------------------
# 3. scan
# ---------------------------------------------------------------------------------------
def ref_stats(kind, ref, plan):
    out = np.zeros(plan.n_segs, dtype=abi.FILTER_STATS_DTYPE)
    for s, sg in enumerate(plan.segs):
        a = int(sg["out_offset"])
        st = ref_scan(kind, ref[a:a + int(sg["payload_bytes"])])
        for name in STAT_FIELDS:
            out[name][s] = st[name]
    return out


@pytest.mark.parametrize("kind,bpk,counts", BATCHES, ids=lambda v: str(v) if not isinstance(v, list) else f"n{len(v)}")
def test_scan(oracle, amq, torch, kind, bpk, counts):
    plan, where, filt, ref = build(oracle, amq, torch, kind, bpk, counts, "offsets")
    want = ref_stats(kind, ref, plan)
    got = amq.scan_filters(plan, filt)
    for name in STAT_FIELDS:
        assert np.array_equal(got[name], want[name]), (name, got[name], want[name])
    assert not got["bad_blocks"].any()
    if kind == BLOOM:
        assert list(got["header_items"]) == counts
    else:
        assert np.array_equal(got["occupied"], got["header_items"])      # sum(occ) == nelts
    # an opened plan scans alike, and a second run is bit-identical
    opened = amq.open_filters(kind, filt, **where)
    assert amq.scan_filters(opened.plan, filt).tobytes() == got.tobytes()
    assert amq.scan_filters(plan, filt).tobytes() == got.tobytes()
    fill = amq.filter_fill(plan, got)
    slots = 512.0 if kind == BLOOM else np.where(plan.segs["tag_bits"] == 8, 48.0, 28.0)
    assert np.allclose(fill, want["occupied"] / (plan.segs["n_blocks"] * slots), rtol=0, atol=1e-15)


# More leaves than the 1,024 threads of the workgroup that turns the leaves' chunk counts into
# their prefix (prefix_inclusive_u64, turtle_kv_amd/csrc/tkv_amq_scan.h): a thread's serial run is
# 1, 2 and 3 elements, with idle threads at the end in the last two.
@pytest.mark.parametrize("n_leaves", [1024, 1025, 2100])
@pytest.mark.parametrize("kind,bpk", [(BLOOM, 10), (VQF, 12)])
def test_scan_more_leaves_than_prefix_threads(oracle, amq, torch, kind, bpk, n_leaves):
    counts = [1 + (37 * i) % 9 for i in range(n_leaves)]
    plan, _, filt, ref = build(oracle, amq, torch, kind, bpk, counts, "offsets")
    want = ref_stats(kind, ref, plan)
    got = amq.scan_filters(plan, filt)
    assert len(got) == n_leaves
    for name in STAT_FIELDS:
        assert np.array_equal(got[name], want[name]), (name, np.flatnonzero(got[name] != want[name])[:8])
    assert not got["bad_blocks"].any() and got["occupied"].all()
    if kind == BLOOM:
        assert list(got["header_items"]) == counts
    else:
        assert np.array_equal(got["occupied"], got["header_items"])


@pytest.mark.parametrize("bpk", [12, 22])
def test_scan_counts_a_broken_vqf_block(oracle, amq, torch, bpk):
    counts = LEAF_COUNTS
    plan, _, filt, ref = build(oracle, amq, torch, VQF, bpk, counts, "offsets")
    base = amq.scan_filters(plan, filt)
    victim = 5
    a = int(plan.segs["out_offset"][victim])
    occ, _, S = ref_vqf_blocks(ref[a:a + int(plan.segs["payload_bytes"][victim])])
    blk = int(np.argmax((occ > 0) & (occ < S)))
    md_bytes = 16 if plan.segs["tag_bits"][victim] == 8 else 8
    # the top metadata bit (a one above the B-th set bit while 0 < occ < S), and the last tag
    # slot (free while occ < S)
    for at, flip in ((a + 80 + 64 * blk + md_bytes - 1, 0x80), (a + 80 + 64 * blk + 63, 0x5A)):
        bad = ref.copy()
        bad[at] ^= flip
        want = ref_stats(VQF, bad, plan)
        assert want["bad_blocks"][victim] == 1
        got = amq.scan_filters(plan, dev(torch, bad))
        assert got["bad_blocks"][victim] == 1
        for name in STAT_FIELDS:
            assert np.array_equal(got[name], want[name]), name
        others = np.arange(len(counts)) != victim
        assert got[others].tobytes() == base[others].tobytes()


def test_scan_no_filter_segments_and_empty_batch(oracle, amq, torch):
    plan, _, filt, ref = build(oracle, amq, torch, BLOOM, 10, LEAF_COUNTS, "offsets")
    none = amq.plan_filters(BLOOM, LEAF_COUNTS, 0)                 # bits/key 0: no filters
    got = amq.scan_filters(none, filt)
    assert got.tobytes() == bytes(32 * len(LEAF_COUNTS))
    assert len(amq.scan_filters(amq.plan_filters(BLOOM, [], 10), filt)) == 0
    assert amq.open_filters(BLOOM, filt, offsets=[]).all_ok


# ---------------------------------------------------------------------------------------
# 4. graph capture
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,bpk", [(BLOOM, 10), (VQF, 12)])
def test_open_scan_probe_replay_in_graph(oracle, amq, torch, kind, bpk):
    counts = LEAF_COUNTS
    plan, where, filt, ref = build(oracle, amq, torch, kind, bpk, counts, "offsets")
    _, _, q, qs = batch_keys(oracle, kind, counts)
    n = len(counts)
    eager = amq.open_filters(kind, filt, **where)
    eager_stats = amq.scan_filters(eager.plan, filt)
    st, want = oracle.probe_segments(kind, ref, plan.segs["out_offset"], q, qs)
    assert st == 0
    d_off = dev(torch, plan.segs["out_offset"].view(np.int64))
    d_segs = torch.zeros(64 * n, dtype=torch.uint8, device="cuda")
    d_status = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    d_summary = torch.full((7,), -1, dtype=torch.int32, device="cuda")
    d_stats = torch.zeros(32 * n, dtype=torch.uint8, device="cuda")
    ws = torch.empty(amq.scan_filters_workspace_bytes(n), dtype=torch.uint8, device="cuda")
    kb, dqs = amq.KeyBatch.fixed(dev(torch, q)), dev(torch, qs.astype(np.int32))
    res = torch.zeros(len(q), dtype=torch.uint8, device="cuda")
    # the probe reads the segments the captured open writes
    gplan = amq.FilterPlan(kind, 0, np.zeros(n, dtype=abi.SEGMENT_DTYPE), filt.numel(), 0, 0, 0)
    gplan._device[str(d_segs.device)] = d_segs
    s = torch.cuda.Stream()

    def work():
        amq.open_filters_device(kind, filt, n, d_segs, d_status, d_summary, offsets=d_off, stream=s)
        amq.scan_filters_device(kind, filt, d_segs, n, d_stats, ws, stream=s)
        amq.probe_filters(gplan, filt, kb, dqs, out=res, stream=s)

    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        work()                      # warm-up on the capture stream
    s.synchronize()
    for t in (d_segs, d_stats, res):
        t.zero_()
    d_status.fill_(-1)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        work()
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    assert d_segs.cpu().numpy().tobytes() == eager.plan.segs.tobytes()
    assert d_status.cpu().tolist() == [0] * n and d_summary.cpu().tolist() == [n, 0, 0, 0, 0, 0, 0]
    assert d_stats.cpu().numpy().tobytes() == eager_stats.tobytes()
    assert np.array_equal(res.cpu().numpy(), want)


# ---------------------------------------------------------------------------------------
# 5. host mirrors
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,bpk", [(BLOOM, 10), (VQF, 12)])
def test_filter_page_from_payload(oracle, amq, torch, kind, bpk):
    n = 9000
    keys = oracle.gen_keys16(31, 0, n)
    oracle.sort_segments(keys, np.array([0, n], dtype=np.uint64))
    planned = amq.build_filter_for_leaf_in_job(bpk, 4242, amq.KeyBatch.fixed(dev(torch, keys)), 32704, kind=kind)
    q = np.concatenate([keys[:500], oracle.gen_keys16(32, 0, 1500)])
    kq = amq.KeyQuery(amq.KeyBatch.fixed(dev(torch, q)))
    want = kq.reject_page(4242, planned)
    assert amq.BoolStatus.kTrue in want and amq.BoolStatus.kFalse in want
    payload = planned.payload[:planned.filter_size].clone()
    page = amq.FilterPage.from_payload(kind, payload)
    assert page.load_status == abi.OPEN_OK and page.leaf_page_id == 4242
    assert page.filter_size == planned.filter_size
    assert kq.reject_page(4242, page) == want
    assert kq.reject_page(4243, page) == [amq.BoolStatus.kUnknown] * len(q)       # another leaf's filter
    if kind == VQF:
        v = amq.PackedVqfFilter(page)
        v.check_magic()
        hv = amq.vqf_hash_val(amq.KeyBatch.fixed(dev(torch, q)))
        assert [amq.BoolStatus.kFalse if p else amq.BoolStatus.kTrue
                for p in v.is_present(hv).cpu().tolist()] == want
    # a payload that does not open: kUnknown for every key, counted as a failed page load
    bad = payload.clone()
    bad[40 if kind == VQF else 46] = 7      # key_remainder_bits / the Bloom layout byte
    broken = amq.FilterPage.from_payload(kind, bad)
    assert broken.load_status == abi.OPEN_BAD_GEOMETRY
    m = amq.KeyQuery.metrics()
    before = m.as_dict()
    assert kq.reject_page(4242, broken) == [amq.BoolStatus.kUnknown] * len(q)
    after = m.as_dict()
    assert after["filter_page_load_failed_count"] - before["filter_page_load_failed_count"] == len(q)
    assert after["total_filter_query_count"] - before["total_filter_query_count"] == len(q)
    for name in ("no_filter_page_count", "page_id_mismatch_count", "filter_reject_count"):
        assert after[name] == before[name]
    # host bytes are uploaded
    assert amq.FilterPage.from_payload(kind, payload.cpu().numpy()).load_status == abi.OPEN_OK
