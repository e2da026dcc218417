"""GPU: the path probe (tkv_amq_path_probe / probe_paths) -- every query hashed once, every
filter on its CSR path asked, the candidates compacted per query in path order.  Expectations
come from the CPU oracle over the expanded (query, leaf) pairs plus numpy compaction; the
device pair probes and the _ex metrics must agree with it too."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COUNTS = [16384, 16384, 16384, 8448, 0, 5, 1, 9000]
VQF_CAP = 32704
VQF_SEED = 0x9D0924DC03E79A75
# workgroup totals one pass of scan_totals covers (kScanTotalsSpan = 256 *
# kScanTotalsPerThread, turtle_kv_amd/csrc/tkv_amq_scan.h), each the sum of 256 queries
SCAN_SPAN = 256 * 4
QUERIES_PER_WG = 256
SETTINGS = [(0, 10), (0, 12), (0, 16), (1, 12), (1, 22)]


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available()
    return t


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def expand(path_begin, n_entries):
    """The clamped lists' (query, entry) pairs, in query then path order."""
    pb = np.asarray(path_begin, dtype=np.int64)
    b = np.minimum(pb[:-1], n_entries)
    e = np.maximum(np.minimum(pb[1:], n_entries), b)
    lens = e - b
    pair_query = np.repeat(np.arange(len(lens)), lens)
    first = np.cumsum(lens) - lens
    pair_entry = np.repeat(b, lens) + (np.arange(int(lens.sum())) - np.repeat(first, lens))
    return pair_query.astype(np.int64), pair_entry.astype(np.int64), lens


def compact(n_queries, pair_query, pair_entry, pair_leaf, ans):
    keep = ans == 1
    cand_begin = np.zeros(n_queries + 1, dtype=np.int64)
    np.cumsum(np.bincount(pair_query[keep], minlength=n_queries), out=cand_begin[1:])
    return cand_begin, pair_leaf[keep].astype(np.int64), pair_entry[keep]


def classify(plan, pair_leaf, page_ids=None):
    """no filter / mismatch / checked per pair (every planned leaf has a filter: bpk > 0)."""
    inplan = pair_leaf < plan.n_segs
    src = np.zeros(len(pair_leaf), np.uint64)
    src[inplan] = plan.segs["src_page_id"][pair_leaf[inplan]]
    mism = inplan & (src != page_ids) if page_ids is not None else np.zeros(len(pair_leaf), bool)
    return inplan, mism, inplan & ~mism


def oracle_answers16(oracle, plan, filt_np, q16, pair_query, pair_leaf, page_ids=None):
    inplan, mism, checked = classify(plan, pair_leaf, page_ids)
    st, ref = oracle.probe_segments(plan.kind, filt_np, plan.segs["out_offset"],
                                    np.ascontiguousarray(q16[pair_query]),
                                    np.where(inplan, pair_leaf, 0).astype(np.uint32))
    assert st == 0
    return np.where(checked, ref, 1).astype(np.uint8), ref


def got(res, with_entries=True):
    total = res.total()
    out = {"total": total, "cand_begin": res.cand_begin.cpu().numpy().astype(np.int64),
           "cand_leaf": res.cand_leaf.cpu().numpy().astype(np.int64)}
    if with_entries and res.cand_entry is not None:
        out["cand_entry"] = res.cand_entry.cpu().numpy().astype(np.int64)
    if res.entry_result is not None:
        out["entry_result"] = res.entry_result.cpu().numpy()
    return out


def check_against(g, n_queries, pair_query, pair_entry, pair_leaf, ans):
    cb, cl, ce = compact(n_queries, pair_query, pair_entry, pair_leaf, ans)
    assert g["total"] == cb[-1]
    assert np.array_equal(g["cand_begin"], cb)
    assert np.array_equal(g["cand_leaf"][:cb[-1]], cl)
    if "cand_entry" in g:
        assert np.array_equal(g["cand_entry"][:cb[-1]], ce)


class Case:
    """One (kind, bits per key) setting of the main case: built filters, queries, paths and the
    oracle-derived expectation, computed once per module and left unchanged."""


_cases = {}


def main_case(oracle, amq, torch, kind, bpk):
    if (kind, bpk) in _cases:
        return _cases[(kind, bpk)]
    c = Case()
    bounds = np.concatenate([[0], np.cumsum(COUNTS)]).astype(np.uint64)
    keys = oracle.gen_keys16(42, 0, sum(COUNTS))
    if kind == 1:
        oracle.sort_segments(keys, bounds)
    c.src = np.arange(700, 700 + len(COUNTS), dtype=np.uint64)
    c.plan = amq.plan_filters(kind, COUNTS, bpk, payload_capacity=VQF_CAP if kind else 0,
                              src_page_ids=c.src)
    c.filt = amq.build_all_filters(c.plan, amq.KeyBatch.fixed(dev(torch, keys)))
    c.filt_np = c.filt.cpu().numpy()
    rng = np.random.default_rng(7)
    n_hit, n_miss = 20000, 30001
    hit_idx = rng.integers(0, len(keys), n_hit)
    c.n_hit = n_hit
    c.own = np.searchsorted(bounds, hit_idx, side="right") - 1
    c.q = np.concatenate([keys[hit_idx], oracle.gen_keys16(43, 0, n_miss)])
    c.nq = len(c.q)
    lens = rng.integers(0, 10, c.nq)
    lens[123] = 300
    c.path_begin = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    c.n_entries = int(c.path_begin[-1])
    c.path_leaf = rng.integers(0, len(COUNTS) + 2, c.n_entries).astype(np.int64)
    has_first = lens[:n_hit] > 0
    c.path_leaf[c.path_begin[:n_hit][has_first]] = c.own[has_first]   # a hit's first entry: its own leaf
    c.lens = lens
    c.pair_query, c.pair_entry, _ = expand(c.path_begin, c.n_entries)
    assert np.array_equal(c.pair_entry, np.arange(c.n_entries))
    c.ans, c.ref = oracle_answers16(oracle, c.plan, c.filt_np, c.q, c.pair_query, c.path_leaf)
    c.qb = amq.KeyBatch.fixed(dev(torch, c.q))
    c.d_begin = dev(torch, c.path_begin.astype(np.int32))
    c.d_leaf = dev(torch, c.path_leaf.astype(np.int32))
    _cases[(kind, bpk)] = c
    return c


@pytest.mark.parametrize("kind,bpk", SETTINGS)
def test_main_case_equals_the_oracle(oracle, amq, torch, kind, bpk):
    c = main_case(oracle, amq, torch, kind, bpk)
    # the classes the case is there for are all populated on the oracle's side
    inplan = c.path_leaf < len(COUNTS)
    miss_entry = c.pair_query >= c.n_hit
    cb, _, _ = compact(c.nq, c.pair_query, c.pair_entry, c.path_leaf, c.ans)
    n_cand = np.diff(cb)
    assert (c.ans == 0).sum() > 100000                               # rejected entries
    assert ((c.ans == 1) & inplan & miss_entry).sum() > 0            # false positives
    assert (~inplan).sum() > 0                                       # entries outside the plan
    assert (c.lens == 0).sum() > 1000                                # empty paths
    assert ((n_cand == 0) & (c.lens > 0)).sum() > 1000               # every entry rejected
    assert ((n_cand == c.lens) & (c.lens > 0)).sum() > 1000          # whole path kept
    assert c.lens[123] == 300 and c.n_entries == 226597 and (c.lens == 0).sum() == 4942
    assert c.ans[c.path_begin[:c.n_hit][c.lens[:c.n_hit] > 0]].all()   # no own-leaf rejection
    if kind == 1 and bpk == 22:
        assert (c.plan.segs["hash_val_shift"] > 0).any()             # truncated hashes
    res = amq.probe_paths(c.plan, c.filt, c.qb, c.d_begin, c.d_leaf, entry_result=True, want_entries=True)
    # canaries: probe again into canary-filled outputs of the same shapes
    res.cand_leaf.fill_(-7)
    res.cand_entry.fill_(-7)
    L, F = amq.abi.lib(), amq.filters
    st = L.tkv_amq_path_probe(kind, F._ptr(c.filt), F._ptr(c.plan.device_segs()), c.plan.n_segs,
                              F._ptr(c.qb.data), None, 16, c.nq, F._ptr(c.d_begin), F._ptr(c.d_leaf),
                              c.n_entries, F._ptr(res.entry_result), F._ptr(res.cand_begin),
                              F._ptr(res.cand_leaf), F._ptr(res.cand_entry), None,
                              F._ptr(res.workspace), res.workspace.numel(), F._stream_handle())
    assert st == amq.abi.OK
    g = got(res)
    assert np.array_equal(g["entry_result"], c.ans)
    check_against(g, c.nq, c.pair_query, c.pair_entry, c.path_leaf, c.ans)
    assert 0 < g["total"] < c.n_entries
    assert (g["cand_leaf"][g["total"]:] == -7).all() and (g["cand_entry"][g["total"]:] == -7).all()
    # every hit's own leaf (its first entry) is a candidate
    has_first = c.lens[:c.n_hit] > 0
    first = c.path_begin[:c.n_hit][has_first]
    assert (g["entry_result"][first] == 1).all()
    assert np.array_equal(g["cand_leaf"][g["cand_begin"][:c.n_hit][has_first]], c.own[has_first])
    # without d_entry_result and d_cand_entry: the same candidates
    res2 = amq.probe_paths(c.plan, c.filt, c.qb, c.d_begin, c.d_leaf)
    assert res2.cand_entry is None and res2.entry_result is None
    check_against(got(res2), c.nq, c.pair_query, c.pair_entry, c.path_leaf, c.ans)


@pytest.mark.parametrize("kind,bpk", SETTINGS)
def test_same_answers_as_the_hashed_pair_probes(oracle, amq, torch, kind, bpk):
    c = main_case(oracle, amq, torch, kind, bpk)
    res = amq.probe_paths(c.plan, c.filt, c.qb, c.d_begin, c.d_leaf, entry_result=True)
    pq = dev(torch, c.pair_query.astype(np.int32))
    if kind == 1:
        pair = amq.vqf_probe_hashed(c.plan, c.filt, amq.vqf_hash_val(c.qb), c.d_leaf, pair_query=pq)
    else:
        pair = amq.bloom_probe_hashed(c.plan, c.filt, amq.bloom_query_hashes(c.qb, 32), 32, c.d_leaf,
                                      pair_query=pq)
    assert torch.equal(res.entry_result, pair)


@pytest.mark.parametrize("kind,bpk", [(0, 10), (1, 12)])
def test_metrics_and_page_ids(oracle, amq, torch, kind, bpk):
    c = main_case(oracle, amq, torch, kind, bpk)
    n_segs = len(COUNTS)
    inplan = c.path_leaf < n_segs
    page_ids = np.where(inplan, c.src[np.minimum(c.path_leaf, n_segs - 1)], 12345).astype(np.uint64)
    miss_entries = np.flatnonzero(c.pair_query >= c.n_hit)
    wrong = miss_entries[::7]
    page_ids[wrong] += 1000
    own_of_query = np.full(c.nq, -1, np.int64)
    own_of_query[:c.n_hit] = c.own
    truth = (c.path_leaf == own_of_query[c.pair_query]).astype(np.uint8)
    ans, ref = oracle_answers16(oracle, c.plan, c.filt_np, c.q, c.pair_query, c.path_leaf, page_ids)
    _, mism, checked = classify(c.plan, c.path_leaf, page_ids)
    pos = checked & (ref == 1)
    m_ref = {"total_filter_query_count": c.n_entries, "no_filter_page_count": int((~inplan).sum()),
             "page_id_mismatch_count": int(mism.sum()),
             "filter_reject_count": int((checked & (ref == 0)).sum()),
             "filter_positive_count": int(pos.sum()),
             "filter_false_positive_count": int((pos & (truth == 0)).sum())}
    assert all(v > 0 for v in m_ref.values())
    d_pid, d_truth = dev(torch, page_ids.view(np.int64)), dev(torch, truth)
    pm = amq.ProbeMetrics()
    res = amq.probe_paths(c.plan, c.filt, c.qb, c.d_begin, c.d_leaf, entry_result=True, want_entries=True,
                          query_page_ids=d_pid, truth=d_truth, metrics=pm)
    g = got(res)
    assert pm.collect() == m_ref
    assert np.array_equal(g["entry_result"], ans)
    check_against(g, c.nq, c.pair_query, c.pair_entry, c.path_leaf, ans)
    # entries whose page id does not match cannot be rejected: all of them are candidates
    mism_entries = np.flatnonzero(mism)
    assert len(mism_entries) > 0 and (g["entry_result"][mism_entries] == 1).all()
    assert np.isin(mism_entries, g["cand_entry"][:g["total"]]).all()
    # the _ex pair probe over the expanded pairs counts the same
    pm2 = amq.ProbeMetrics()
    pq = dev(torch, c.pair_query.astype(np.int32))
    if kind == 1:
        amq.vqf_probe_hashed(c.plan, c.filt, amq.vqf_hash_val(c.qb), c.d_leaf, pair_query=pq,
                             query_page_ids=d_pid, truth=d_truth, metrics=pm2)
    else:
        amq.bloom_probe_hashed(c.plan, c.filt, amq.bloom_query_hashes(c.qb, 32), 32, c.d_leaf,
                               pair_query=pq, query_page_ids=d_pid, truth=d_truth, metrics=pm2)
    assert pm2.collect() == m_ref
    # the counters accumulate: doubled after a second launch
    amq.probe_paths(c.plan, c.filt, c.qb, c.d_begin, c.d_leaf, query_page_ids=d_pid, truth=d_truth,
                    metrics=pm)
    assert pm.collect() == {k: 2 * v for k, v in m_ref.items()}


@pytest.mark.parametrize("kind,bpk", [(0, 10), (1, 12)])
@pytest.mark.parametrize("shape", ["k24", "var"])
def test_other_key_shapes(oracle, amq, torch, kind, bpk, shape):
    rng = np.random.default_rng(11)
    counts = [2000, 2000, 2000]
    n, n_miss = sum(counts), 750
    lens = np.full(n + n_miss, 24) if shape == "k24" else rng.integers(8, 41, n + n_miss)
    offs = np.zeros(len(lens) + 1, np.int64)
    offs[1:] = np.cumsum(lens)
    blob = rng.integers(0, 256, int(offs[-1]), dtype=np.uint8)
    key = lambda i: blob[offs[i]:offs[i + 1]].tobytes()
    if shape == "k24":
        kb = amq.KeyBatch.fixed(dev(torch, blob[:offs[n]].reshape(n, 24)))
    else:
        assert (lens < 32).sum() > 100 and (lens >= 32).sum() > 100   # both hash branches
        kb = amq.KeyBatch.variable(dev(torch, blob[:offs[n]]), dev(torch, offs[:n + 1]))
    plan = amq.plan_filters(kind, counts, bpk, payload_capacity=VQF_CAP if kind else 0)
    filt = amq.build_all_filters(plan, kb)
    f = filt.cpu().numpy()
    # 750 hits and 750 misses, paths of 0..4 entries, a hit's first entry its own leaf
    qidx = np.concatenate([rng.integers(0, n, 750), np.arange(n, n + n_miss)])
    nq = len(qidx)
    q_lens = lens[qidx]
    q_offs = np.zeros(nq + 1, np.int64)
    q_offs[1:] = np.cumsum(q_lens)
    q_blob = np.concatenate([blob[offs[i]:offs[i + 1]] for i in qidx])
    qb = (amq.KeyBatch.fixed(dev(torch, q_blob.reshape(nq, 24))) if shape == "k24"
          else amq.KeyBatch.variable(dev(torch, q_blob), dev(torch, q_offs)))
    plens = rng.integers(0, 5, nq)
    path_begin = np.concatenate([[0], np.cumsum(plens)]).astype(np.int64)
    n_entries = int(path_begin[-1])
    path_leaf = rng.integers(0, len(counts) + 1, n_entries).astype(np.int64)
    hit_first = plens[:750] > 0
    path_leaf[path_begin[:750][hit_first]] = qidx[:750][hit_first] // 2000
    pair_query, pair_entry, _ = expand(path_begin, n_entries)
    payload = [f[int(s["out_offset"]):int(s["out_offset"]) + int(s["payload_bytes"])] for s in plan.segs]
    ans = np.ones(n_entries, np.uint8)
    for e in range(n_entries):                      # a few thousand oracle calls
        leaf = path_leaf[e]
        if leaf >= len(counts):
            continue
        k = key(qidx[pair_query[e]])
        ans[e] = (oracle.vqf_is_present(payload[leaf], oracle.xxh64(k, VQF_SEED)) if kind
                  else oracle.bloom_query(payload[leaf], k))
    assert 0 < (ans == 0).sum() < n_entries
    res = amq.probe_paths(plan, filt, qb, dev(torch, path_begin.astype(np.int32)),
                          dev(torch, path_leaf.astype(np.int32)), entry_result=True, want_entries=True)
    g = got(res)
    assert np.array_equal(g["entry_result"], ans)
    check_against(g, nq, pair_query, pair_entry, path_leaf, ans)
    assert (g["entry_result"][path_begin[:750][hit_first]] == 1).all()
    # and exactly what the unhashed pair probe answers for the same pairs
    if shape == "k24":
        pq_keys = amq.KeyBatch.fixed(dev(torch, q_blob.reshape(nq, 24)[pair_query]))
        pair = amq.probe_filters(plan, filt, pq_keys, dev(torch, path_leaf.astype(np.int32)))
        assert torch.equal(res.entry_result, pair)


def small_case(oracle, amq, torch, kind):
    counts = [3000, 0, 2000]
    bounds = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    keys = oracle.gen_keys16(42, 0, sum(counts))
    if kind == 1:
        oracle.sort_segments(keys, bounds)
    plan = amq.plan_filters(kind, counts, 12 if kind else 10, payload_capacity=VQF_CAP if kind else 0)
    filt = amq.build_all_filters(plan, amq.KeyBatch.fixed(dev(torch, keys)))
    return counts, keys, plan, filt


def run_and_check(oracle, amq, torch, plan, filt, q, path_begin, path_leaf, n_entries=None):
    """probe_paths against the oracle over the clamped lists; returns the device answer."""
    nq = len(q)
    n_entries = len(path_leaf) if n_entries is None else n_entries
    pair_query, pair_entry, _ = expand(path_begin, n_entries)
    pair_leaf = np.asarray(path_leaf, np.int64)[pair_entry]
    if len(pair_query):
        ans, _ = oracle_answers16(oracle, plan, filt.cpu().numpy(), q, pair_query, pair_leaf)
    else:
        ans = np.zeros(0, np.uint8)
    qb = amq.KeyBatch.fixed(dev(torch, q) if nq else torch.empty((0, 16), dtype=torch.uint8, device="cuda"))
    res = amq.probe_paths(plan, filt, qb, dev(torch, np.asarray(path_begin).astype(np.int32)),
                          dev(torch, np.asarray(path_leaf[:n_entries]).astype(np.int32)),
                          entry_result=True, want_entries=True)
    g = got(res)
    check_against(g, nq, pair_query, pair_entry, pair_leaf, ans)
    return g, ans, pair_entry


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("nq", [0, 1, 63, 64, 65, 256, 257])
def test_edge_query_counts(oracle, amq, torch, kind, nq):
    counts, keys, plan, filt = small_case(oracle, amq, torch, kind)
    rng = np.random.default_rng(100 + nq)
    q = np.concatenate([keys[rng.integers(0, len(keys), nq // 2)], oracle.gen_keys16(43, 0, nq - nq // 2)])
    lens = rng.integers(0, 6, nq)
    path_begin = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    path_leaf = rng.integers(0, len(counts) + 1, int(path_begin[-1]))
    g, ans, _ = run_and_check(oracle, amq, torch, plan, filt, q, path_begin, path_leaf)
    assert g["cand_begin"][0] == 0 and len(g["cand_begin"]) == nq + 1
    assert np.array_equal(g["entry_result"], ans)


@pytest.mark.parametrize("kind", [0, 1])
def test_all_paths_empty_and_all_entries_rejected(oracle, amq, torch, kind):
    counts, keys, plan, filt = small_case(oracle, amq, torch, kind)
    nq = 700
    miss = oracle.gen_keys16(43, 0, nq)
    g, _, _ = run_and_check(oracle, amq, torch, plan, filt, miss, np.zeros(nq + 1, np.int64),
                            np.zeros(0, np.int64))
    assert g["total"] == 0 and not g["cand_begin"].any()
    # misses only, in-plan leaves: keep the queries every one of whose entries the oracle rejects
    path_begin = np.arange(nq + 1, dtype=np.int64) * 2
    path_leaf = np.tile(np.array([0, 2]), nq)
    pair_query, _, _ = expand(path_begin, 2 * nq)
    ans, _ = oracle_answers16(oracle, plan, filt.cpu().numpy(), miss, pair_query, path_leaf)
    keep = np.flatnonzero(ans.reshape(nq, 2).sum(axis=1) == 0)
    assert len(keep) > 600
    g, ans, _ = run_and_check(oracle, amq, torch, plan, filt, miss[keep],
                              np.arange(len(keep) + 1, dtype=np.int64) * 2, np.tile(np.array([0, 2]), len(keep)))
    assert g["total"] == 0 and not g["cand_begin"].any() and not g["entry_result"].any()


@pytest.mark.parametrize("kind", [0, 1])
def test_scan_crosses_one_pass_of_the_totals_scan(oracle, amq, torch, kind):
    counts, keys, plan, filt = small_case(oracle, amq, torch, kind)
    nq = SCAN_SPAN * QUERIES_PER_WG + 257          # more workgroup totals than one scan pass covers
    rng = np.random.default_rng(3)
    q = oracle.gen_keys16(43, 0, nq)
    hits = rng.integers(0, nq, nq // 3)
    q[hits] = keys[rng.integers(0, len(keys), len(hits))]
    lens = rng.integers(0, 3, nq)
    path_begin = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    path_leaf = rng.integers(0, len(counts) + 1, int(path_begin[-1]))
    g, ans, _ = run_and_check(oracle, amq, torch, plan, filt, q, path_begin, path_leaf)
    assert np.array_equal(g["entry_result"], ans)
    # candidates on both sides of the pass boundary
    cut = g["cand_begin"][SCAN_SPAN * QUERIES_PER_WG]
    assert 0 < cut < g["total"]


@pytest.mark.parametrize("kind", [0, 1])
def test_malformed_lists_answer_as_the_clamped_lists(oracle, amq, torch, kind):
    counts, keys, plan, filt = small_case(oracle, amq, torch, kind)
    rng = np.random.default_rng(9)
    nq = 600
    q = np.concatenate([keys[rng.integers(0, len(keys), 300)], oracle.gen_keys16(43, 0, 300)])
    lens = rng.integers(0, 6, nq)
    path_begin = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n_entries = int(path_begin[-1]) - 40            # the last ends lie past n_entries
    assert path_begin[-1] > n_entries and (path_begin > n_entries).sum() > 3
    k = next(i for i in range(200, nq) if lens[i] > 0 and lens[i - 1] > 0)
    path_begin[k + 1] = path_begin[k] - 1           # one pair decreases: query k reads as empty,
    #                                                 and query k + 1 then covers query k - 1's last entry
    slack = 64                                      # allocated past n_entries: a missing clamp reads
    path_leaf = rng.integers(0, len(counts) + 1, n_entries + slack)   # these, and answers wrongly
    pair_query, pair_entry, clens = expand(path_begin, n_entries)
    assert clens[k] == 0 and clens[-1] == 0 and pair_entry.max() < n_entries
    pair_leaf = path_leaf[pair_entry]
    ans, _ = oracle_answers16(oracle, plan, filt.cpu().numpy(), q, pair_query, pair_leaf)
    qb = amq.KeyBatch.fixed(dev(torch, q))
    d_leaf_all = dev(torch, path_leaf.astype(np.int32))
    res = amq.probe_paths(plan, filt, qb, dev(torch, path_begin.astype(np.int32)), d_leaf_all[:n_entries],
                          entry_result=True, want_entries=True)
    g = got(res)
    check_against(g, nq, pair_query, pair_entry, pair_leaf, ans)
    # d_entry_result: defined wherever exactly one path covers the entry
    cover = np.bincount(pair_entry, minlength=n_entries)
    assert (cover == 2).sum() == 1 and cover.max() == 2
    once = cover[pair_entry] == 1
    assert np.array_equal(g["entry_result"][pair_entry[once]], ans[once])


@pytest.mark.parametrize("kind", [0, 1])
def test_replays_in_a_graph(oracle, amq, torch, kind):
    c = main_case(oracle, amq, torch, kind, 12 if kind else 10)
    eager = got(amq.probe_paths(c.plan, c.filt, c.qb, c.d_begin, c.d_leaf, entry_result=True, want_entries=True))
    ws = torch.empty(amq.path_probe_workspace_bytes(c.nq, c.n_entries), dtype=torch.uint8, device="cuda")
    er = torch.zeros(c.n_entries, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm-up on the capture stream
        amq.probe_paths(c.plan, c.filt, c.qb, c.d_begin, c.d_leaf, entry_result=er, want_entries=True,
                        workspace=ws, stream=s)
    s.synchronize()
    er.zero_()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        res = amq.probe_paths(c.plan, c.filt, c.qb, c.d_begin, c.d_leaf, entry_result=er, want_entries=True,
                              workspace=ws, stream=s)
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    g = got(res)
    assert g["total"] == eager["total"]
    for k in ("cand_begin", "entry_result"):
        assert np.array_equal(g[k], eager[k])
    for k in ("cand_leaf", "cand_entry"):
        assert np.array_equal(g[k][:g["total"]], eager[k][:g["total"]])
