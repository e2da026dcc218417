"""The read side against the CPU oracle, where real filters cannot tell a wrong kernel from a
right one.  Every comparison is exact equality with the oracle over the same bytes.

A. Bloom, every hash index.  A real filter rejects almost every miss at its first few hash
   indices, so a probe that dropped index 20 would pass every test of real filters.  Here the
   blocks of small built filters (real headers, real plan) are overwritten with random bits of
   density 0.5^(1/k): about half of all queries pass, and for every index j < k there are queries
   whose only zero bit is bit j.  k = 1 .. 32, through the plain probe, the probe with options,
   the hashed probe (k_max = k, 32 and k - 1), the path probe and the verify pass, for 16-byte
   keys and five other key shapes.
B. VQF, a bucket longer than the 16-byte tag window of vqf_bucket_has: keys crafted into one
   bucket, so that the per-slot loop behind the window decides answers.
C. The _ex probes at more queries than two passes of their bounded grid.

The inputs of each part are built in a test that needs no GPU (the *_inputs tests): it asserts,
from the oracle alone, the conditions that make the GPU tests discriminating."""
import numpy as np
import pytest

from turtle_kv_amd import abi

from test_gpu_parity import _bloom_seed
from test_gpu_path_probe import check_against, expand, got
from test_gpu_verify import assert_result, fold, key_batch
from test_gpu_verify import run as verify_run

gpu = pytest.mark.gpu

BLOOM, VQF = 0, 1
VQF_SEED = 0x9D0924DC03E79A75
FIELDS = abi.PROBE_METRICS_FIELDS


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available()
    return t


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------------------------------
# expectations: the oracle's answer per (query, leaf), then the probes' classes on top of it
# ---------------------------------------------------------------------------------------
def expected(plan, seg, ref, page_ids=None, truth=None, k_max=None):
    """(answers, the six counters) of pairs asking leaf seg[i], as expected_metrics of
    test_gpu_pages_metrics.py derives them.  ref[i]: the oracle's answer for pair i on leaf
    min(seg[i], n_segs - 1) (unused where the leaf is outside the plan or has no filter).  k_max:
    the hashed Bloom probe's record holds k_max hashes, and a filter of more is "no filter" to it
    (include/tkv_amq.h) -- segment by segment, before the page-id check."""
    n = plan.n_segs
    sc = np.minimum(seg, n - 1)
    built = plan.segs["hash_count" if plan.kind == BLOOM else "tag_bits"] != 0
    if k_max is not None and plan.kind == BLOOM:
        built = built & (plan.segs["hash_count"] <= k_max)
    has = (seg < n) & built[sc]
    mism = np.zeros(len(seg), bool) if page_ids is None else has & (plan.segs["src_page_id"][sc] != page_ids)
    checked = has & ~mism
    pos = checked & (ref == 1)
    counts = (len(seg), int((~has).sum()), int(mism.sum()), int((checked & (ref == 0)).sum()), int(pos.sum()),
              0 if truth is None else int((pos & (truth == 0)).sum()))
    return np.where(checked, ref, 1).astype(np.uint8), dict(zip(FIELDS, counts))


def table16(oracle, plan, host, q16):
    """oracle.probe_segments of every 16-byte query on every leaf of the plan: [n_queries, n_segs].
    The column of a "no filter" segment (an opened plan's refused slot: the oracle has nothing to
    read there) is 1 and unused by `expected`."""
    t = np.ones((len(q16), plan.n_segs), np.uint8)
    q16 = np.ascontiguousarray(q16)
    built = plan.segs["hash_count" if plan.kind == BLOOM else "tag_bits"] != 0
    for s in np.flatnonzero(built):
        st, r = oracle.probe_segments(plan.kind, host, plan.segs["out_offset"], q16,
                                      np.full(len(q16), s, np.uint32))
        assert st == 0
        t[:, s] = r
    return t


def options_for(rng, plan, seg):
    """Per pair: the page id asked about (every 7th wrong) and a ground truth."""
    n = plan.n_segs
    page_ids = np.where(seg < n, plan.segs["src_page_id"][np.minimum(seg, n - 1)], 12345).astype(np.uint64)
    page_ids[::7] += 1000
    return page_ids, rng.integers(0, 2, len(seg)).astype(np.uint8)


class Routes:
    """What every route asks and what the oracle expects of it, for one set of queries (their
    bytes are the caller's): computed once per case from the oracle's table and left unchanged."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def make_routes(rng, plan, table, seg, leaf_draw, long_at, fixed_paths=None):
    """fixed_paths: {query: its path's leaves, in entry order}, in place of the random path."""
    r, n, nq = Routes(), plan.n_segs, len(seg)
    look = lambda qi, s: table[qi, np.minimum(s, n - 1)]
    r.nq, r.seg = nq, seg
    # one leaf per query: the plain probe, the probe with options, the hashed probe
    r.page_ids, r.truth = options_for(rng, plan, seg)
    r.ref = ref = look(np.arange(nq), seg)
    r.plain = expected(plan, seg, ref)
    r.opts = expected(plan, seg, ref, r.page_ids, r.truth)
    r.share = float(ref[seg < n].mean())
    # (query, leaf) pairs through pair_query
    r.pair_query, r.pair_seg = rng.integers(0, nq, nq), leaf_draw(nq)
    r.pair_page_ids, r.pair_truth = options_for(rng, plan, r.pair_seg)
    r.pair_ref = ref = look(r.pair_query, r.pair_seg)
    r.pair_plain = expected(plan, r.pair_seg, ref)
    r.pair_opts = expected(plan, r.pair_seg, ref, r.pair_page_ids, r.pair_truth)
    # paths of 0 .. 3 entries, and one of 40: past kPathMaskEntries (32), whose answers are bytes
    lens = rng.integers(0, 4, nq)
    lens[long_at] = 40
    for qi, leaves in (fixed_paths or {}).items():
        assert qi != long_at
        lens[qi] = len(leaves)
    r.path_begin = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    r.n_entries = int(r.path_begin[-1])
    r.path_leaf = leaf_draw(r.n_entries).astype(np.int64)
    for qi, leaves in (fixed_paths or {}).items():
        r.path_leaf[r.path_begin[qi]:r.path_begin[qi + 1]] = leaves
    r.path_query, r.path_entry, _ = expand(r.path_begin, r.n_entries)
    r.path_page_ids, r.path_truth = options_for(rng, plan, r.path_leaf)
    ref = look(r.path_query, r.path_leaf)
    r.path_plain = expected(plan, r.path_leaf, ref)
    r.path_opts = expected(plan, r.path_leaf, ref, r.path_page_ids, r.path_truth)
    # the verify pass: the in-plan queries grouped by leaf are each leaf's "keys"
    inplan = np.flatnonzero(seg < n)
    r.v_order = inplan[np.argsort(seg[inplan], kind="stable")]
    r.v_begin = np.concatenate([[0], np.cumsum(np.bincount(seg[inplan], minlength=n))]).astype(np.uint64)
    v_seg = seg[r.v_order].astype(np.uint32)
    r.v_missing, r.v_first = fold(n, np.arange(len(r.v_order), dtype=np.int64), v_seg, table[r.v_order, v_seg])
    return r


def assert_routes_populated(r, plan):
    """Every class of answer and every counter occurs on the oracle's side."""
    for ans, m in (r.opts, r.pair_opts, r.path_opts):
        assert all(v > 0 for v in m.values()), m
        assert 0 < int(ans.sum()) < len(ans)
    assert r.path_begin[-1] == r.n_entries and (np.diff(r.path_begin) == 40).sum() == 1
    assert (np.diff(r.path_begin) == 0).sum() > 0
    for leaves in (r.seg, r.pair_seg, r.path_leaf):
        assert (leaves >= plan.n_segs).sum() >= 2


# ---------------------------------------------------------------------------------------
# the routes on the device
# ---------------------------------------------------------------------------------------
def ids(torch, page_ids):
    return dev(torch, page_ids.view(np.int64))


def check_probe(amq, torch, plan, filt, qb, r, prefixes=()):
    d_seg = dev(torch, r.seg.astype(np.int32))
    res = amq.probe_filters(plan, filt, qb, d_seg)
    assert np.array_equal(res.cpu().numpy(), r.plain[0])
    for m in prefixes:
        sub = amq.probe_filters(plan, filt, amq.KeyBatch.fixed(qb.data[:m]), d_seg[:m])
        assert np.array_equal(sub.cpu().numpy(), r.plain[0][:m]), m
    pm = amq.ProbeMetrics()
    res = amq.probe_filters(plan, filt, qb, d_seg, query_page_ids=ids(torch, r.page_ids),
                            truth=dev(torch, r.truth), metrics=pm)
    assert np.array_equal(res.cpu().numpy(), r.opts[0])
    assert pm.collect() == r.opts[1]


def hashed_call(amq, plan, filt, hashes, k_max, d_seg, **kw):
    if plan.kind == VQF:
        return amq.vqf_probe_hashed(plan, filt, hashes, d_seg, **kw)
    return amq.bloom_probe_hashed(plan, filt, hashes, k_max, d_seg, **kw)


def hashed_expected(plan, r, k_max):
    """The four expectations of the hashed probe whose records hold k_max hashes: r's own where no
    filter of the plan has more (every VQF plan; k_max None), else `expected` over the same
    oracle answers with the longer filters classed as the header classes them."""
    if plan.kind == VQF or k_max is None or int(plan.segs["hash_count"].max()) <= k_max:
        return r.plain, r.pair_plain, r.opts, r.pair_opts
    return (expected(plan, r.seg, r.ref, k_max=k_max), expected(plan, r.pair_seg, r.pair_ref, k_max=k_max),
            expected(plan, r.seg, r.ref, r.page_ids, r.truth, k_max=k_max),
            expected(plan, r.pair_seg, r.pair_ref, r.pair_page_ids, r.pair_truth, k_max=k_max))


def check_hashed(amq, torch, plan, filt, qb, r, k_maxes=(None,)):
    d_seg, d_ps = dev(torch, r.seg.astype(np.int32)), dev(torch, r.pair_seg.astype(np.int32))
    d_pq = dev(torch, r.pair_query.astype(np.int32))
    for k_max in k_maxes:
        plain, pair_plain, opts, pair_opts = hashed_expected(plan, r, k_max)
        h = amq.vqf_hash_val(qb) if plan.kind == VQF else amq.bloom_query_hashes(qb, k_max)
        res = hashed_call(amq, plan, filt, h, k_max, d_seg)
        assert np.array_equal(res.cpu().numpy(), plain[0]), k_max
        res = hashed_call(amq, plan, filt, h, k_max, d_ps, pair_query=d_pq)
        assert np.array_equal(res.cpu().numpy(), pair_plain[0]), k_max
        pm = amq.ProbeMetrics()
        res = hashed_call(amq, plan, filt, h, k_max, d_seg, query_page_ids=ids(torch, r.page_ids),
                          truth=dev(torch, r.truth), metrics=pm)
        assert np.array_equal(res.cpu().numpy(), opts[0]), k_max
        assert pm.collect() == opts[1], k_max
        pm = amq.ProbeMetrics()
        res = hashed_call(amq, plan, filt, h, k_max, d_ps, pair_query=d_pq,
                          query_page_ids=ids(torch, r.pair_page_ids), truth=dev(torch, r.pair_truth), metrics=pm)
        assert np.array_equal(res.cpu().numpy(), pair_opts[0]), k_max
        assert pm.collect() == pair_opts[1], k_max


def check_k_max_below(amq, torch, plan, filt, qb, r, k_max):
    """Filters of the plan have more hashes than the cache holds: a pair on one of them cannot be
    rejected and counts as no_filter_page_count (include/tkv_amq.h) -- before the page-id check;
    every other pair is tested as usual.  Into zeroed results, so an answer 1 was written."""
    h = amq.bloom_query_hashes(qb, k_max)
    plain, pair_plain, opts, pair_opts = hashed_expected(plan, r, k_max)
    if (plan.segs["hash_count"] > k_max).all():     # no filter can be asked: every pair is of that class
        none = dict(zip(FIELDS, (r.nq, r.nq, 0, 0, 0, 0)))
        for ans, m in (plain, pair_plain, opts, pair_opts):
            assert ans.all() and m == none
    for seg, pq, page_ids, truth, want, want_opts in (
            (r.seg, None, r.page_ids, r.truth, plain, opts),
            (r.pair_seg, r.pair_query, r.pair_page_ids, r.pair_truth, pair_plain, pair_opts)):
        d_seg = dev(torch, seg.astype(np.int32))
        d_pq = None if pq is None else dev(torch, pq.astype(np.int32))
        out = torch.zeros(r.nq, dtype=torch.uint8, device="cuda")
        amq.bloom_probe_hashed(plan, filt, h, k_max, d_seg, out=out, pair_query=d_pq)
        assert np.array_equal(out.cpu().numpy(), want[0])
        out.zero_()
        pm = amq.ProbeMetrics()
        amq.bloom_probe_hashed(plan, filt, h, k_max, d_seg, out=out, pair_query=d_pq,
                               query_page_ids=ids(torch, page_ids), truth=dev(torch, truth), metrics=pm)
        assert np.array_equal(out.cpu().numpy(), want_opts[0])
        assert pm.collect() == want_opts[1]


def check_paths(amq, torch, plan, filt, qb, r):
    d_begin, d_leaf = dev(torch, r.path_begin.astype(np.int32)), dev(torch, r.path_leaf.astype(np.int32))
    g = got(amq.probe_paths(plan, filt, qb, d_begin, d_leaf, entry_result=True, want_entries=True))
    assert np.array_equal(g["entry_result"], r.path_plain[0])
    check_against(g, r.nq, r.path_query, r.path_entry, r.path_leaf, r.path_plain[0])
    pm = amq.ProbeMetrics()
    g = got(amq.probe_paths(plan, filt, qb, d_begin, d_leaf, entry_result=True, want_entries=True,
                            query_page_ids=ids(torch, r.path_page_ids), truth=dev(torch, r.path_truth), metrics=pm))
    assert np.array_equal(g["entry_result"], r.path_opts[0])
    check_against(g, r.nq, r.path_query, r.path_entry, r.path_leaf, r.path_opts[0])
    assert pm.collect() == r.path_opts[1]


def check_verify(amq, torch, plan, filt, vkb, r, hints=("plan", 1), flags=0):
    """max_seg_blocks as planned: the leaf's image in LDS; 1: every leaf of more than one block is
    read from global memory; a hint between: the leaves above it alone.  flags: per leaf, where
    the plan holds a "no filter" segment."""
    assert plan.max_seg_blocks > 1
    for hint in hints:
        res, total = verify_run(amq, torch, plan, filt, vkb, key_begin=r.v_begin, hint=hint)
        assert_result(res, total, r.v_missing, r.v_first, flags=flags)


def assert_built_as_oracle(amq, torch, plan, keys, host):
    """The device build of `keys` writes the oracle's payloads (headers included)."""
    out = amq.build_all_filters(plan, amq.KeyBatch.fixed(dev(torch, keys))).cpu().numpy()
    for s, sg in enumerate(plan.segs):
        o, n = int(sg["out_offset"]), int(sg["payload_bytes"])
        assert out[o:o + n].tobytes() == host[o:o + n].tobytes(), f"leaf {s}"


# ---------------------------------------------------------------------------------------
# A. Bloom: every hash index decides
# ---------------------------------------------------------------------------------------
ALL_K = list(range(1, 33))
SHAPE_K = [1, 2, 7, 8, 9, 16, 17, 32]
COUNTS_A = [3000, 1, 0, 700]
NQ_A, NQ_SHAPE = 20000, 3000
HOST_SHAPES = ("k24", "s20", "k40", "var")          # the bytes; "k24off4": k24's at another address
DEVICE_SHAPES = ("k24", "k24off4", "s20", "k40", "var")

_bloom, _bloom16, _bloom_shape = {}, {}, {}


def bloom_filters(oracle, amq, k):
    """The plan and the oracle's build of COUNTS_A at a bits/key whose hash count is k, and the
    same bytes with every block overwritten by random bits of density 0.5^(1/k)."""
    if k not in _bloom:
        f = Routes()
        f.k = k
        f.bpk = next(b for b in range(1, 47) if oracle.lib().tkvo_bloom_hash_count(b) == k)
        f.plan = amq.plan_filters(BLOOM, COUNTS_A, f.bpk, src_page_ids=np.arange(500, 504, dtype=np.uint64))
        assert (f.plan.segs["hash_count"] == k).all()
        f.keys = oracle.gen_keys16(42, 0, sum(COUNTS_A))
        f.built = np.zeros(f.plan.total_out_bytes, np.uint8)
        f.synth = np.zeros(f.plan.total_out_bytes, np.uint8)
        rng = np.random.default_rng(1000 + k)
        b = 0
        for s, sg in enumerate(f.plan.segs):
            st, ref = oracle.bloom_build(f.keys[b:], COUNTS_A[s], f.bpk, src_page_id=int(sg["src_page_id"]))
            assert st == 0 and len(ref) == int(sg["payload_bytes"]) == 64 + 64 * int(sg["n_blocks"])
            o = int(sg["out_offset"])
            f.built[o:o + len(ref)] = ref
            f.synth[o:o + 64] = ref[:64]
            bits = rng.random(512 * int(sg["n_blocks"])) < 0.5 ** (1.0 / k)
            f.synth[o + 64:o + len(ref)] = np.packbits(bits, bitorder="little")
            b += COUNTS_A[s]
        f.payload = [np.ascontiguousarray(f.synth[int(sg["out_offset"]):int(sg["out_offset"]) + int(sg["payload_bytes"])])
                     for sg in f.plan.segs]
        _bloom[k] = f
    return _bloom[k]


def random_segs(rng, n_segs, nq):
    """Random leaves of the plan, two of the indices outside it."""
    seg = rng.integers(0, n_segs, nq)
    seg[nq // 3], seg[nq // 2] = n_segs, n_segs + 5
    return seg


def bloom16(oracle, amq, k):
    if k not in _bloom16:
        f = bloom_filters(oracle, amq, k)
        rng = np.random.default_rng(2000 + k)
        c = Routes()
        c.q = rng.integers(0, 256, (NQ_A, 16), dtype=np.uint8)
        c.table = table16(oracle, f.plan, f.synth, c.q)
        n = f.plan.n_segs
        c.r = make_routes(rng, f.plan, c.table, random_segs(rng, n, NQ_A), lambda size: rng.integers(0, n + 1, size),
                          long_at=123)
        _bloom16[k] = c
    return _bloom16[k]


def shape_keys(rng, shape, n):
    """k24 / s20 / k40: [n, L] rows; var: a list of n keys of 0 .. 71 bytes."""
    if shape != "var":
        return rng.integers(0, 256, (n, {"k24": 24, "s20": 20, "k40": 40}[shape]), dtype=np.uint8)
    lens = rng.integers(0, 72, n)
    lens[:4] = (0, 31, 32, 33)
    return [rng.integers(0, 256, int(m), dtype=np.uint8).tobytes() for m in lens]


def bloom_shape(oracle, amq, k, shape):
    """Other key shapes on the same synthetic filters: oracle.bloom_query per key and leaf."""
    if (k, shape) not in _bloom_shape:
        f = bloom_filters(oracle, amq, k)
        rng = np.random.default_rng(3000 + 10 * k + HOST_SHAPES.index(shape))
        c = Routes()
        c.keys = shape_keys(rng, shape, NQ_SHAPE)
        n = f.plan.n_segs
        c.table = np.array([[oracle.bloom_query(p, bytes(key)) for p in f.payload] for key in c.keys], np.uint8)
        c.r = make_routes(rng, f.plan, c.table, random_segs(rng, n, NQ_SHAPE),
                          lambda size: rng.integers(0, n + 1, size), long_at=123)
        _bloom_shape[(k, shape)] = c
    return _bloom_shape[(k, shape)]


def take(keys, idx):
    return [keys[i] for i in idx] if isinstance(keys, list) else np.ascontiguousarray(keys[idx])


def batch(amq, torch, shape, keys):
    """The KeyBatch of host keys; k24off4: the 24-byte rows at a pointer 4 bytes off 8-byte
    alignment (key_batch of test_gpu_verify.py)."""
    if isinstance(keys, list):
        offs = np.zeros(len(keys) + 1, np.int64)
        np.cumsum([len(key) for key in keys], out=offs[1:])
        blob = np.frombuffer(b"".join(keys), dtype=np.uint8).copy()
        return amq.KeyBatch.variable(dev(torch, blob), dev(torch, offs))
    return key_batch(amq, torch, shape, np.ascontiguousarray(keys), None)


@pytest.mark.parametrize("k", ALL_K)
def test_bloom_inputs(oracle, amq, k):
    """The conditions of part A, from the references alone: about half of the checked queries
    pass; python-xxhash's evaluation of the bit test gives the oracle's answers; and every hash
    index j < k is, for at least 50 queries, the only one whose bit is zero."""
    import xxhash
    f, c = bloom_filters(oracle, amq, k), bloom16(oracle, amq, k)
    r, plan = c.r, f.plan
    assert 0.35 <= r.share <= 0.65, r.share
    assert_routes_populated(r, plan)
    assert (r.seg >= plan.n_segs).sum() == 2
    # the second evaluation
    idx = np.flatnonzero(r.seg < plan.n_segs)
    rows = [c.q[i].tobytes() for i in idx]
    sg = plan.segs[r.seg[idx]]
    h0 = [xxhash.xxh64_intdigest(b, _bloom_seed(0)) for b in rows]
    blk = np.array([(h * int(nb)) >> 64 for h, nb in zip(h0, sg["n_blocks"])], np.int64)
    bit = np.empty((len(idx), k), np.int64)
    bit[:, 0] = [h & 511 for h in h0]
    for j in range(1, k):
        seed = _bloom_seed(j)
        bit[:, j] = [xxhash.xxh64_intdigest(b, seed) & 511 for b in rows]
    all_bits = np.unpackbits(f.synth, bitorder="little")
    val = all_bits[(8 * (sg["out_offset"].astype(np.int64) + 64 + 64 * blk))[:, None] + bit]
    assert np.array_equal(val.all(axis=1), r.plain[0][idx] == 1)
    only = val.sum(axis=1) == k - 1
    decides = [int((only & (val[:, j] == 0)).sum()) for j in range(k)]
    assert min(decides) >= 50, decides
    # the verify pass has rejects to count in every leaf
    assert (r.v_missing > 0).all() and (np.diff(r.v_begin.astype(np.int64)) > r.v_missing).all()


@pytest.mark.parametrize("shape", HOST_SHAPES)
@pytest.mark.parametrize("k", SHAPE_K)
def test_bloom_shape_inputs(oracle, amq, k, shape):
    c = bloom_shape(oracle, amq, k, shape)
    assert 0.35 <= c.r.share <= 0.65, c.r.share
    assert_routes_populated(c.r, bloom_filters(oracle, amq, k).plan)
    assert (c.r.v_missing > 0).all()
    if shape == "var":
        lens = [len(key) for key in c.keys]
        assert lens[:4] == [0, 31, 32, 33] and max(lens) == 71
        assert sum(m < 32 for m in lens) > 1000 and sum(m >= 32 for m in lens) > 1000   # both hashers


_bloom_dev = {}


def bloom_device(oracle, amq, torch, k):
    """The synthetic filters on the device, once the device build of the same plan has written the
    oracle's bytes (the headers kept are the real ones)."""
    if k not in _bloom_dev:
        f = bloom_filters(oracle, amq, k)
        assert_built_as_oracle(amq, torch, f.plan, f.keys, f.built)
        _bloom_dev[k] = dev(torch, f.synth)
    return _bloom_dev[k]


@gpu
@pytest.mark.parametrize("k", ALL_K)
def test_bloom_probe_every_hash_index(oracle, amq, torch, k):
    f, c = bloom_filters(oracle, amq, k), bloom16(oracle, amq, k)
    check_probe(amq, torch, f.plan, bloom_device(oracle, amq, torch, k), amq.KeyBatch.fixed(dev(torch, c.q)), c.r,
                prefixes=(1, 255, 256, 257))


@gpu
@pytest.mark.parametrize("k", ALL_K)
def test_bloom_hashed_probe_every_hash_index(oracle, amq, torch, k):
    f, c = bloom_filters(oracle, amq, k), bloom16(oracle, amq, k)
    filt, qb = bloom_device(oracle, amq, torch, k), amq.KeyBatch.fixed(dev(torch, c.q))
    check_hashed(amq, torch, f.plan, filt, qb, c.r, k_maxes=sorted({k, 32}))
    if k >= 2:
        check_k_max_below(amq, torch, f.plan, filt, qb, c.r, k - 1)


@gpu
@pytest.mark.parametrize("k", ALL_K)
def test_bloom_path_probe_every_hash_index(oracle, amq, torch, k):
    f, c = bloom_filters(oracle, amq, k), bloom16(oracle, amq, k)
    check_paths(amq, torch, f.plan, bloom_device(oracle, amq, torch, k), amq.KeyBatch.fixed(dev(torch, c.q)), c.r)


@gpu
@pytest.mark.parametrize("k", ALL_K)
def test_bloom_verify_every_hash_index(oracle, amq, torch, k):
    f, c = bloom_filters(oracle, amq, k), bloom16(oracle, amq, k)
    check_verify(amq, torch, f.plan, bloom_device(oracle, amq, torch, k),
                 amq.KeyBatch.fixed(dev(torch, c.q[c.r.v_order])), c.r)


@gpu
@pytest.mark.parametrize("shape", DEVICE_SHAPES)
@pytest.mark.parametrize("k", SHAPE_K)
def test_bloom_other_key_shapes(oracle, amq, torch, k, shape):
    f = bloom_filters(oracle, amq, k)
    c = bloom_shape(oracle, amq, k, "k24" if shape == "k24off4" else shape)
    filt, qb = bloom_device(oracle, amq, torch, k), batch(amq, torch, shape, c.keys)
    assert qb.n == NQ_SHAPE and (shape != "k24off4" or qb.data.data_ptr() % 8 == 4)
    check_probe(amq, torch, f.plan, filt, qb, c.r)
    check_hashed(amq, torch, f.plan, filt, qb, c.r, k_maxes=sorted({k, 32}))
    if k >= 2:
        check_k_max_below(amq, torch, f.plan, filt, qb, c.r, k - 1)
    check_paths(amq, torch, f.plan, filt, qb, c.r)
    check_verify(amq, torch, f.plan, filt, batch(amq, torch, shape, take(c.keys, c.r.v_order)), c.r)


# ---------------------------------------------------------------------------------------
# B. VQF: a bucket longer than the tag window
# ---------------------------------------------------------------------------------------
# tag bits -> bits/key, crafted keys planted, unrelated keys beside them, the ordinary leaves'
# key counts, and the run that one 16-byte window (16 / 8 slots from the dword that holds the
# bucket's first slot) cannot cover
LONG = {8: dict(bpk=12, planted=24, pads=40, others=(50, 30), min_run=17, buckets=80, md_bytes=16),
        16: dict(bpk=22, planted=14, pads=18, others=(40, 25), min_run=9, buckets=36, md_bytes=8)}
SMALL_CAP = 208                 # 32 + 48 + two 64-byte blocks
TARGET = 7                      # the bucket (of block 0) the crafted keys share
CRAFTED_LEAF = 1
VQF_BLOCKS_AT = 32 + 48         # PackedVqfFilter header, vqf_metadata

_vqf = {}


def craft(rng, tag_bits, n_buckets, bucket, n):
    """Random 16-byte keys whose primary bucket is `bucket`, by brute force."""
    import xxhash
    out = []
    while len(out) < n:
        for row in rng.integers(0, 256, (4096, 16), dtype=np.uint8):
            if (xxhash.xxh64_intdigest(row.tobytes(), VQF_SEED) >> tag_bits) % n_buckets == bucket:
                out.append(row)
    return np.array(out[:n])


def bucket_run(block, md_bytes, o):
    """Slots [start, end) of bucket o: the zeros before the o-th set bit of the block's metadata."""
    ones = np.flatnonzero(np.unpackbits(block[:md_bytes], bitorder="little"))
    return (0 if o == 0 else int(ones[o - 1]) - (o - 1)), int(ones[o]) - o


def vqf_long(oracle, amq, tag_bits):
    if tag_bits in _vqf:
        return _vqf[tag_bits]
    p, c = LONG[tag_bits], Routes()
    rng = np.random.default_rng(800 + tag_bits)
    n_buckets = 2 * p["buckets"]
    crafted = craft(rng, tag_bits, n_buckets, TARGET, p["planted"] + 500)
    c.n_planted = p["planted"]
    planted, near = crafted[:c.n_planted], crafted[c.n_planted:]
    pads = rng.integers(0, 256, (p["pads"], 16), dtype=np.uint8)
    counts = [p["others"][0], c.n_planted + p["pads"], p["others"][1]]
    c.keys = np.concatenate([oracle.gen_keys16(42, 0, counts[0]), planted, pads, oracle.gen_keys16(44, 0, counts[2])])
    bounds = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    oracle.sort_segments(c.keys, bounds)
    c.plan = plan = amq.plan_filters(VQF, counts, p["bpk"], payload_capacity=SMALL_CAP,
                                     src_page_ids=np.arange(300, 303, dtype=np.uint64))
    sg = plan.segs[CRAFTED_LEAF]
    assert (int(sg["tag_bits"]), int(sg["n_blocks"]), int(sg["hash_val_shift"])) == (tag_bits, 2, 0)
    c.host = np.zeros(plan.total_out_bytes, np.uint8)
    for s, g in enumerate(plan.segs):
        st, ref, pl = oracle.vqf_build(c.keys[int(bounds[s]):], counts[s], p["bpk"], SMALL_CAP,
                                       src_page_id=int(g["src_page_id"]))
        assert st == 0 and pl.payload_used == int(g["payload_bytes"])
        c.host[int(g["out_offset"]):int(g["out_offset"]) + pl.payload_used] = ref[:pl.payload_used]
    # the target bucket's run, and the damage: another tag in the run's last slot
    blk_at = int(sg["out_offset"]) + VQF_BLOCKS_AT + 64 * (TARGET // p["buckets"])
    c.start, c.end = bucket_run(c.host[blk_at:blk_at + 64], p["md_bytes"], TARGET % p["buckets"])
    at, nb = blk_at + p["md_bytes"] + (tag_bits // 8) * (c.end - 1), tag_bits // 8
    c.damaged = c.host.copy()
    c.damaged[at:at + nb] ^= 0x5A
    c.old_tag = int.from_bytes(c.host[at:at + nb].tobytes(), "little")
    c.new_tag = int.from_bytes(c.damaged[at:at + nb].tobytes(), "little")
    # the planted keys, 500 misses of the same primary bucket, 500 random misses: each asked of the
    # crafted leaf, and once more of a random leaf (two of the indices outside the plan)
    q0 = np.concatenate([planted, near, rng.integers(0, 256, (500, 16), dtype=np.uint8)])
    c.n0 = len(q0)
    c.q = np.concatenate([q0, q0])
    seg = np.concatenate([np.full(c.n0, CRAFTED_LEAF), rng.integers(0, plan.n_segs + 2, c.n0)])
    draw = lambda size: np.where(rng.random(size) < 0.6, CRAFTED_LEAF, rng.integers(0, plan.n_segs + 1, size))
    c.tables = {"clean": table16(oracle, plan, c.host, c.q), "damaged": table16(oracle, plan, c.damaged, c.q)}
    state = rng.bit_generator.state
    c.routes = {}
    for name, table in c.tables.items():     # the same pairs and paths against both tables
        rng.bit_generator.state = state
        c.routes[name] = make_routes(rng, plan, table, seg, draw, long_at=0)
    _vqf[tag_bits] = c
    return c


@pytest.mark.parametrize("tag_bits", [8, 16])
def test_vqf_long_bucket_inputs(oracle, amq, tag_bits):
    import xxhash
    c, p = vqf_long(oracle, amq, tag_bits), LONG[tag_bits]
    plan = c.plan
    # the run is longer than the window, so its last slots are reached only by the per-slot loop
    assert c.end - c.start >= p["min_run"]
    per_dword = 32 // tag_bits
    assert c.end > (c.start // per_dword) * per_dword + 4 * per_dword
    # oracle.vqf_is_present per query on the crafted leaf's payload: the table's column
    sg = plan.segs[CRAFTED_LEAF]
    hashes = [xxhash.xxh64_intdigest(row.tobytes(), VQF_SEED) for row in c.q[:c.n0]]
    for name, host in (("clean", c.host), ("damaged", c.damaged)):
        payload = np.ascontiguousarray(host[int(sg["out_offset"]):int(sg["out_offset"]) + int(sg["payload_bytes"])])
        per_key = np.array([oracle.vqf_is_present(payload, h) for h in hashes], np.uint8)
        assert np.array_equal(per_key, c.tables[name][:c.n0, CRAFTED_LEAF])
        assert_routes_populated(c.routes[name], plan)
    clean, damaged = (c.tables[n][:c.n0, CRAFTED_LEAF] for n in ("clean", "damaged"))
    assert clean[:c.n_planted].all()                                  # every planted key is found
    n_pass = int(clean[c.n_planted:].sum())                           # misses: most are rejected, and of the
    assert n_pass < 200 and (n_pass > 0 or tag_bits == 16)            # 8-bit tags some pass (13 tags of 65,536: none)
    # the damage takes away exactly keys that owned the overwritten tag, and at least one planted key
    tags = np.array([h & ((1 << tag_bits) - 1) for h in hashes])
    lost, won = (clean == 1) & (damaged == 0), (clean == 0) & (damaged == 1)
    assert lost[:c.n_planted].any() and (tags[lost] == c.old_tag).all() and (tags[won] == c.new_tag).all()
    assert c.routes["damaged"].v_missing[CRAFTED_LEAF] > c.routes["clean"].v_missing[CRAFTED_LEAF] > 0


@gpu
@pytest.mark.parametrize("state", ["clean", "damaged"])
@pytest.mark.parametrize("tag_bits", [8, 16])
def test_vqf_long_bucket(oracle, amq, torch, tag_bits, state):
    c = vqf_long(oracle, amq, tag_bits)
    assert_built_as_oracle(amq, torch, c.plan, c.keys, c.host)
    r, filt = c.routes[state], dev(torch, c.host if state == "clean" else c.damaged)
    qb = amq.KeyBatch.fixed(dev(torch, c.q))
    check_probe(amq, torch, c.plan, filt, qb, r, prefixes=(c.n_planted,))
    check_hashed(amq, torch, c.plan, filt, qb, r)
    check_paths(amq, torch, c.plan, filt, qb, r)
    check_verify(amq, torch, c.plan, filt, amq.KeyBatch.fixed(dev(torch, c.q[r.v_order])), r)


# ---------------------------------------------------------------------------------------
# C. the _ex probes past one pass of their grid
# ---------------------------------------------------------------------------------------
EX_GRID, EX_WG = 8192, 256
N_EX = 2 * EX_GRID * EX_WG + 300
N_DISTINCT = 50000
COUNTS_C = [16384, 16384, 16384, 5]

_ex = {}


def ex_queries(oracle):
    if "q" not in _ex:
        _ex["q"] = oracle.gen_keys16(42, 0, N_EX)
    return _ex["q"]


def ex_case(oracle, amq, kind):
    """N_EX queries (the first sum(COUNTS_C) of them the leaves' own keys, asked of their own
    leaf), and N_EX pairs over the first N_DISTINCT queries: answers and counters from the oracle."""
    if kind in _ex:
        return _ex[kind]
    c, bpk, cap = Routes(), (12 if kind else 10), (32704 if kind else 0)
    n_keys, q = sum(COUNTS_C), ex_queries(oracle)
    bounds = np.concatenate([[0], np.cumsum(COUNTS_C)]).astype(np.uint64)
    c.keys = q[:n_keys].copy()
    if kind:
        oracle.sort_segments(c.keys, bounds)
    c.plan = plan = amq.plan_filters(kind, COUNTS_C, bpk, payload_capacity=cap,
                                     src_page_ids=np.arange(900, 904, dtype=np.uint64))
    n = plan.n_segs
    c.host = np.zeros(plan.total_out_bytes, np.uint8)
    for s, g in enumerate(plan.segs):
        src, keys = int(g["src_page_id"]), c.keys[int(bounds[s]):]
        if kind:
            st, ref, pl = oracle.vqf_build(keys, COUNTS_C[s], bpk, cap, src_page_id=src)
            ref = ref[:pl.payload_used]
        else:
            st, ref = oracle.bloom_build(keys, COUNTS_C[s], bpk, src_page_id=src)
        assert st == 0 and len(ref) == int(g["payload_bytes"])
        c.host[int(g["out_offset"]):int(g["out_offset"]) + len(ref)] = ref
    rng = np.random.default_rng(50 + kind)
    own = np.repeat(np.arange(n), COUNTS_C)

    def one(query_of, seg):
        """Pairs (query_of[i], seg[i]): every 7th page id wrong, the truth known."""
        inplan = seg < n
        page_ids = np.where(inplan, plan.segs["src_page_id"][np.minimum(seg, n - 1)], 12345).astype(np.uint64)
        page_ids[::7] += 1000
        truth = ((query_of < n_keys) & (seg == own[np.minimum(query_of, n_keys - 1)])).astype(np.uint8)
        st, ref = oracle.probe_segments(kind, c.host, plan.segs["out_offset"], np.ascontiguousarray(q[query_of]),
                                        np.where(inplan, seg, 0).astype(np.uint32))
        assert st == 0
        ans, m = expected(plan, seg, ref, page_ids, truth)
        assert ref[truth == 1].all()                                  # no false negatives in the reference
        return Routes(seg=seg, page_ids=page_ids, truth=truth, ans=ans, m=m)

    seg = rng.integers(0, n + 2, N_EX)
    seg[:n_keys:2] = own[::2]                                         # half of the keys ask their own leaf
    c.raw = one(np.arange(N_EX), seg)
    c.pair_query = rng.integers(0, N_DISTINCT, N_EX)
    c.pair_query[-n_keys:] = np.arange(n_keys)                        # (hits in the last pass of the grid)
    seg = rng.integers(0, n + 2, N_EX)
    seg[-n_keys::2] = own[::2]
    c.pairs = one(c.pair_query, seg)
    _ex[kind] = c
    return c


@pytest.mark.parametrize("kind", [BLOOM, VQF])
def test_ex_grid_inputs(oracle, amq, kind):
    c = ex_case(oracle, amq, kind)
    # probe_grid(n, true) (turtle_kv_amd/csrc/tkv_amq_launch.h) caps the grid of the _ex probes at
    # 8,192 workgroups of 256 lanes: more than two grids of queries, so every lane of the strided
    # loops takes a second pass and the first 300 a third, adding to its ProbeTally in each
    assert N_EX > 2 * EX_GRID * EX_WG and len(ex_queries(oracle)) == N_EX
    assert len(np.unique(ex_queries(oracle)[:N_DISTINCT], axis=0)) == N_DISTINCT
    for e in (c.raw, c.pairs):
        assert all(v > 0 for v in e.m.values()), e.m
        assert e.m["filter_positive_count"] > e.m["filter_false_positive_count"]
        for lo, hi in ((0, EX_GRID * EX_WG), (EX_GRID * EX_WG, 2 * EX_GRID * EX_WG), (2 * EX_GRID * EX_WG, N_EX)):
            assert 0 < int(e.ans[lo:hi].sum()) < hi - lo              # both answers in every pass


@gpu
@pytest.mark.parametrize("kind", [BLOOM, VQF])
def test_ex_probes_past_one_grid(oracle, amq, torch, kind):
    c = ex_case(oracle, amq, kind)
    plan, q = c.plan, ex_queries(oracle)
    assert_built_as_oracle(amq, torch, plan, c.keys, c.host)
    filt = dev(torch, c.host)
    # the raw _ex probe, into a canary-filled result
    out = torch.full((N_EX,), 0xAB, dtype=torch.uint8, device="cuda")
    pm = amq.ProbeMetrics()
    amq.probe_filters(plan, filt, amq.KeyBatch.fixed(dev(torch, q)), dev(torch, c.raw.seg.astype(np.int32)), out=out,
                      query_page_ids=ids(torch, c.raw.page_ids), truth=dev(torch, c.raw.truth), metrics=pm)
    assert np.array_equal(out.cpu().numpy(), c.raw.ans)
    assert pm.collect() == c.raw.m
    # the hashed _ex probe: N_EX pairs over N_DISTINCT hashed queries
    qb = amq.KeyBatch.fixed(dev(torch, q[:N_DISTINCT]))
    h = amq.vqf_hash_val(qb) if kind == VQF else amq.bloom_query_hashes(qb, 32)
    out.fill_(0xAB)
    pm = amq.ProbeMetrics()
    hashed_call(amq, plan, filt, h, 32, dev(torch, c.pairs.seg.astype(np.int32)), out=out,
                pair_query=dev(torch, c.pair_query.astype(np.int32)), query_page_ids=ids(torch, c.pairs.page_ids),
                truth=dev(torch, c.pairs.truth), metrics=pm)
    assert np.array_equal(out.cpu().numpy(), c.pairs.ans)
    assert pm.collect() == c.pairs.m
