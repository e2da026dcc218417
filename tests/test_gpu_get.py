"""GPU: the fused point lookup (tkv_amq_get_keys / get_keys) -- every query descended from the
root, the filter of every entry on its way asked, the leaves whose filters say maybe searched, the
lookup ended at the first leaf that holds the key, and the rest of a level skipped when the key is
found below the segment's flushed item upper bound.

The expectation is `model_get` below: tests/test_gpu_walk.py's `model_one` (the entries in order)
with the visit rule of include/tkv_amq.h applied to them.  Filter answers come from the CPU oracle
over the built filter bytes, key by key, as tests/test_gpu_path_probe.py takes them.  The model
yields the result, the visit count and the class of every visit; the six metrics and the six
counts follow from those.  Every comparison is exact, every output sits between canary guards."""
import bisect
import os
import re

import numpy as np
import pytest

from test_gpu_walk import (CANARY, GUARD, LEAF_LEVEL, MALFORMED, MAX_DEPTH, clone, dev, fixed_batch, guarded, key16,
                           leaf, malformed, model_one, uneven_queries, uneven_tree, var_batch)

pytestmark = pytest.mark.gpu

VQF_CAP = 32704
VQF_SEED = 0x9D0924DC03E79A75
NOT_FOUND, NO_LEAF = (1 << 64) - 1, 0xFFFFFFFF
NO_FILTER, MISMATCH, CHECKED = 0, 1, 2                             # reject_page's classes
KINDS = [0, 1]
BPK = {0: 10, 1: 12}
METRICS = ("total_filter_query_count", "no_filter_page_count", "page_id_mismatch_count", "filter_reject_count",
           "filter_positive_count", "filter_false_positive_count")
COUNTS = ("visit_count", "leaf_search_count", "found_count", "absent_count", "unsearchable_count", "flushed_count")


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available()
    return t


# ---------------------------------------------------------------------------------------
# a world: leaves with their keys, the filters built over them, the oracle's answers
# ---------------------------------------------------------------------------------------
class World:
    """The plan's leaves (sorted lists of keys), their filters as built on the device, and the CPU
    oracle's answer for any (leaf, key), remembered.  Built once per case and left unchanged."""

    def __init__(self, oracle, amq, torch, kind, leaves, bpk=None, src=None, leaf_form="auto", shift=0):
        self.oracle, self.kind, self.leaves = oracle, kind, [list(lv) for lv in leaves]
        assert all(lv == sorted(set(lv)) for lv in self.leaves)
        counts = [len(lv) for lv in self.leaves]
        assert max(counts) <= 1000
        self.begin = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        self.src = np.arange(7000, 7000 + len(counts), dtype=np.uint64) if src is None else np.asarray(src, np.uint64)
        flat = [k for lv in self.leaves for k in lv]
        lens = {len(k) for k in flat}
        if leaf_form == "var" or len(lens) != 1:
            self.leaf_kb = build_kb = var_batch(amq, torch, flat)
        else:
            length = lens.pop()
            self.leaf_kb = build_kb = fixed_batch(amq, torch, flat, length, shift)
            if shift:                                             # (the build takes aligned keys; the search any)
                build_kb = fixed_batch(amq, torch, flat, length)
        bpk = BPK[kind] if bpk is None else bpk
        self.plan = amq.plan_filters(kind, counts, bpk, payload_capacity=VQF_CAP if kind else 0, src_page_ids=self.src)
        if bpk:
            self.filt = amq.build_all_filters(self.plan, build_kb)
        else:                                                     # no filter anywhere: no byte of this is read
            self.filt = torch.full((64,), CANARY, dtype=torch.uint8, device="cuda")
        f = self.filt.cpu().numpy()
        self.payload = [f[int(s["out_offset"]):int(s["out_offset"]) + int(s["payload_bytes"])] for s in self.plan.segs]
        self.n = len(counts)
        self._answers = {}

    @classmethod
    def over(cls, oracle, plan, leaves, payload):
        """The same over filters that no one plan built and nothing here builds: `plan` holds their
        segments (an opened array's: hash counts, tag widths and page ids per segment; a segment
        without a filter where a slot was refused), payload[s] the bytes of segment s.  Host only:
        `filt`, `leaf_kb` and the device's own copy of the plan are the caller's to attach."""
        w = cls.__new__(cls)
        w.oracle, w.kind, w.leaves = oracle, plan.kind, [list(lv) for lv in leaves]
        assert all(lv == sorted(set(lv)) for lv in w.leaves) and len(w.leaves) == plan.n_segs == len(payload)
        w.begin = np.concatenate([[0], np.cumsum([len(lv) for lv in w.leaves])]).astype(np.int64)
        w.src = plan.segs["src_page_id"].astype(np.uint64)
        w.plan, w.payload, w.n, w._answers = plan, list(payload), plan.n_segs, {}
        w.filt = w.leaf_kb = None
        return w

    def ask(self, leaf_i, page_id, key, check_ids):
        """(class, answer) of one visit, as reject_page classifies it."""
        if leaf_i >= self.n:
            return NO_FILTER, 1
        seg = self.plan.segs[leaf_i]
        if int(seg["tag_bits"] if self.kind else seg["hash_count"]) == 0:
            return NO_FILTER, 1
        if check_ids and int(self.src[leaf_i]) != page_id:
            return MISMATCH, 1
        if (leaf_i, key) not in self._answers:
            O = self.oracle
            self._answers[(leaf_i, key)] = int(O.vqf_is_present(self.payload[leaf_i], O.xxh64(key, VQF_SEED))
                                               if self.kind else O.bloom_query(self.payload[leaf_i], key))
        return CHECKED, self._answers[(leaf_i, key)]


def model_get(w, tree, q, check_ids=False, n_nodes=None):
    """Query q over `tree` in world w: ((key_index, leaf, where), [(class, answer, state)] per visit)."""
    visits, left = [], None
    for leaf_i, page_id, flushed_bound, where in model_one(tree, q, n_nodes):
        if where == left:                                         # the level was left: not visited
            continue
        cls, ans = w.ask(leaf_i, page_id, q, check_ids)
        state = None
        if ans:
            if leaf_i >= w.n:
                state = "unsearchable"
            else:
                keys = w.leaves[leaf_i]
                at = bisect.bisect_left(keys, q)
                if at == len(keys) or keys[at] != q:
                    state = "absent"
                elif at < flushed_bound:
                    state, left = "flushed", where
                else:
                    state = "found"
        visits.append((cls, ans, state))
        if state == "found":
            return (int(w.begin[leaf_i]) + at, leaf_i, where), visits
    return (NOT_FOUND, NO_LEAF, NO_LEAF), visits


def model_batch(w, tree, queries, check_ids=False, n_nodes=None):
    rows = [model_get(w, tree, q, check_ids, n_nodes) for q in queries]
    flat = [v for _, vs in rows for v in vs]
    cls = np.array([v[0] for v in flat], np.int64)
    ans = np.array([v[1] for v in flat], np.int64)
    state = np.array([v[2] or "" for v in flat])
    metrics = [len(flat), int((cls == NO_FILTER).sum()), int((cls == MISMATCH).sum()),
               int(((cls == CHECKED) & (ans == 0)).sum()), int(((cls == CHECKED) & (ans == 1)).sum()),
               int(((cls == CHECKED) & (state == "absent")).sum())]
    n = {s: int((state == s).sum()) for s in ("found", "absent", "unsearchable", "flushed")}
    counts = [len(flat), n["found"] + n["absent"] + n["flushed"], n["found"], n["absent"], n["unsearchable"],
              n["flushed"]]
    return {"key_index": np.array([r[0][0] for r in rows], np.uint64),
            "leaf": np.array([r[0][1] for r in rows], np.uint32), "where": np.array([r[0][2] for r in rows], np.uint32),
            "visits": np.array([len(r[1]) for r in rows], np.int64), "metrics": dict(zip(METRICS, metrics)),
            "counts": dict(zip(COUNTS, counts)), "rows": rows}


# ---------------------------------------------------------------------------------------
# the device side
# ---------------------------------------------------------------------------------------
def launch(amq, w, tree, qb, bufs, check_ids=False, pk=None, n_nodes=None, stream=None, key_begin=None):
    d_nodes, d_segs, d_kids, d_bounds, own_pk = tree.device()
    pk = own_pk if pk is None else pk
    b = {k: (None if v is None else v[1]) for k, v in bufs.items()}
    amq.get_keys_device(w.kind, w.filt if w.n else None, w.plan.device_segs() if w.n else None, w.n, d_nodes,
                        len(tree.nodes) if n_nodes is None else n_nodes, d_segs, len(tree.segments), d_kids,
                        len(tree.children), d_bounds, len(tree.flushed_bounds), pk.data, pk.offsets, pk.stride, pk.n,
                        qb.data, qb.offsets, qb.stride, qb.n, w.leaf_kb.data, w.leaf_kb.offsets, w.leaf_kb.stride,
                        w.leaf_kb.n, key_begin, b["result"], b["visits"],
                        amq.abi.GET_CHECK_PAGE_ID if check_ids else 0, b["metrics"], b["counts"], stream)


def buffers(torch, n, visits=True, metrics=True, counts=True):
    bufs = {"result": guarded(torch, 16 * n, torch.uint8), "visits": guarded(torch, n, torch.int32) if visits else None,
            "metrics": guarded(torch, 6, torch.int64) if metrics else None,
            "counts": guarded(torch, 6, torch.int64) if counts else None}
    for name in ("metrics", "counts"):
        if bufs[name] is not None:
            bufs[name][1].zero_()
    return bufs


def read(amq, torch, bufs):
    torch.cuda.synchronize()
    out = {}
    for name, pair in bufs.items():
        if pair is None:
            continue
        raw = pair[0].cpu().numpy()
        bts, g = raw.view(np.uint8), GUARD * raw.itemsize
        assert (bts[:g] == CANARY).all() and (bts[len(bts) - g:] == CANARY).all(), name
        out[name] = raw[GUARD:len(raw) - GUARD]
    rec = out.pop("result").view(amq.abi.GET_RESULT_DTYPE)
    out["key_index"], out["leaf"], out["where"] = rec["key_index"].copy(), rec["leaf"].copy(), rec["where"].copy()
    return out


def run(amq, torch, w, tree, qb, **kw):
    opts = {k: kw.pop(k) for k in ("visits", "metrics", "counts") if k in kw}
    bufs = buffers(torch, qb.n, **opts)
    launch(amq, w, tree, qb, bufs, **kw)
    return read(amq, torch, bufs)


def same(got, want, times=1):
    for name in ("key_index", "leaf", "where"):
        assert np.array_equal(got[name], want[name]), name
    if "visits" in got:
        assert np.array_equal(got["visits"].astype(np.int64), want["visits"])
    if "metrics" in got:
        assert dict(zip(METRICS, (int(v) for v in got["metrics"]))) == {k: times * v for k, v in want["metrics"].items()}
    if "counts" in got:
        assert dict(zip(COUNTS, (int(v) for v in got["counts"]))) == {k: times * v for k, v in want["counts"].items()}


def check(amq, torch, w, tree, queries, qb=None, **kw):
    want = model_batch(w, tree, queries, kw.get("check_ids", False), kw.get("n_nodes"))
    qb = amq.KeyBatch.from_host(queries) if qb is None else qb
    same(run(amq, torch, w, tree, qb, **kw), want)
    return want


# ---------------------------------------------------------------------------------------
# 1. the flushed rule
# ---------------------------------------------------------------------------------------
def k(i):
    return key16(i)


def flushed_world(oracle, amq, torch, kind):
    """One node of two pivots (cut at k(500)) over child leaves 0 and 1; level 0: leaves 2 and 3, level
    1: leaf 4.  X, Z and E are keys of pivot 1, Y of pivot 0."""
    X, Y, Z, E = k(700), k(100), k(650), k(800)
    filler = lambda lo, n: [k(lo + 2 * j + 1) for j in range(n)]   # odd keys: none of the four
    leaves = [[k(10), k(20)], [k(600), k(900)],
              sorted(filler(500, 60) + [X, Y, Z]),                # leaf 2: level 0, first segment
              sorted(filler(500, 30) + [X, E]),                   # leaf 3: level 0, second segment
              sorted(filler(600, 40) + [X, Z, E])]                # leaf 4: level 1
    w = World(oracle, amq, torch, kind, leaves)
    at = lambda i, key: w.leaves[i].index(key)
    seg = lambda i, fl: {"leaf": i, "page_id": 7000 + i, "active": 0b11, "flushed": fl}
    node = {"pivot_keys": [k(0), k(500), k(1000)], "children": [leaf(0), leaf(1)],
            "levels": [[seg(2, {1: at(2, X) + 1}),               # X and Z lie below pivot 1's bound; Y is pivot 0's
                        seg(3, {})],
                       [seg(4, {0: 1000, 1: at(4, X)})]]}         # X sits AT the bound (rank 1), Z and ... below it
    assert at(2, Z) < at(2, X) and at(4, Z) < at(4, X) < at(4, E) and at(2, Y) < at(2, X)
    return w, amq.TreeIndex.from_description(node), (X, Y, Z, E)


@pytest.mark.parametrize("kind", KINDS)
def test_flushed_rule(oracle, amq, torch, kind):
    w, tree, (X, Y, Z, E) = flushed_world(oracle, amq, torch, kind)
    qs = [X, Y, Z, E, k(601), k(20), k(901)] + [k(j) for j in range(400, 1000, 7)]
    want = check(amq, torch, w, tree, qs)
    res = {q: (int(want["leaf"][i]), int(want["where"][i]), int(want["visits"][i])) for i, q in enumerate(qs)}
    # X: flushed from leaf 2; leaf 3 (which holds it) is skipped with the level; found in level 1, AT its bound
    assert len(model_one(tree, X)) == 4 and res[X] == (4, 1, 2)
    assert int(want["key_index"][0]) == int(w.begin[4]) + w.leaves[4].index(X)
    assert [v[2] for v in want["rows"][0][1]] == ["flushed", "found"]
    # Y: pivot 0 -- leaf 2's bound is pivot 1's and does not apply (leaf 4's own bound for pivot 0 would)
    assert res[Y] == (2, 0, 1)
    # Z: flushed from both levels (bit_rank picks leaf 4's second bound), absent from the child: not found, and
    # one visit short of the unskipped walk
    assert res[Z][0] == NO_LEAF and res[Z][2] == len(model_one(tree, Z)) - 1 == 3
    assert [v[2] for v in want["rows"][2][1]][:2] == ["flushed", "flushed"]
    # E: not in leaf 2, so level 0 goes on to leaf 3
    assert res[E] == (3, 0, 2)
    assert want["counts"]["flushed_count"] >= 3 and want["counts"]["found_count"] >= 4
    assert want["metrics"]["total_filter_query_count"] == want["counts"]["visit_count"] == int(want["visits"].sum())
    # a bound index past n_flushed_bounds reads 0: X is found where it was flushed from
    t = clone(amq, tree)
    t.segments["flushed_begin"][0] = len(t.flushed_bounds) + 5
    want = check(amq, torch, w, t, qs)
    assert (int(want["leaf"][0]), int(want["where"][0]), int(want["visits"][0])) == (2, 0, 1)
    # without visits, metrics or counts: the same results
    got = run(amq, torch, w, tree, amq.KeyBatch.from_host(qs), visits=False, metrics=False, counts=False)
    same(got, model_batch(w, tree, qs))
    # the convenience wrapper
    pm, gc = amq.ProbeMetrics(), amq.GetCounts()
    r = amq.get_keys(w.plan, w.filt, tree, amq.KeyBatch.from_host(qs), w.leaf_kb, want_visits=True, metrics=pm, counts=gc)
    want = model_batch(w, tree, qs)
    assert np.array_equal(r.key_index.cpu().numpy().view(np.uint64), want["key_index"])
    assert np.array_equal(r.leaf.cpu().numpy().view(np.uint32), want["leaf"])
    assert np.array_equal(r.where.cpu().numpy().view(np.uint32), want["where"])
    assert np.array_equal(r.visits.cpu().numpy(), want["visits"])
    assert pm.collect() == want["metrics"] and gc.collect() == want["counts"]


@pytest.mark.parametrize("kind", KINDS)
def test_key_begin_and_the_wrapper(oracle, amq, torch, kind):
    """The leaves' ranges from d_key_begin, not from the plan: the same keys behind one more key in front, so
    the plan's own ranges are off by one and only the CSR is right.  Through the launch alone and
    through get_keys, with page ids checked against a tree that has one wrong."""
    import copy
    w, tree, (X, Y, Z, E) = flushed_world(oracle, amq, torch, kind)
    qs = [X, Y, Z, E, k(601), k(20), k(901)] + [k(j) for j in range(400, 1000, 7)]
    plain = model_batch(w, tree, qs)
    w2 = copy.copy(w)
    w2.begin = w.begin + 1
    w2.leaf_kb = fixed_batch(amq, torch, [b"\x00" * 16] + [key for lv in w.leaves for key in lv], 16)
    want = check(amq, torch, w2, tree, qs, key_begin=dev(torch, w2.begin))
    found = plain["leaf"] != NO_LEAF
    assert found[[0, 1, 3, 5]].all()                              # X, Y, E and k(20) are keys of the leaves
    assert np.array_equal(want["key_index"][found], plain["key_index"][found] + 1)
    assert np.array_equal(want["leaf"], plain["leaf"]) and np.array_equal(want["visits"], plain["visits"])
    t = clone(amq, tree)
    t.segments["leaf_page_id"][1] = 4242                          # leaf 3's segment under a wrong id
    want = model_batch(w2, t, qs, True)
    assert want["metrics"]["page_id_mismatch_count"] > 0
    pm, gc = amq.ProbeMetrics(), amq.GetCounts()
    qb = amq.KeyBatch.from_host(qs)
    r = amq.get_keys(w2.plan, w2.filt, t, qb, w2.leaf_kb, key_begin=w2.begin, check_page_ids=True, want_visits=True,
                     metrics=pm, counts=gc)
    assert np.array_equal(r.key_index.cpu().numpy().view(np.uint64), want["key_index"])
    assert np.array_equal(r.leaf.cpu().numpy().view(np.uint32), want["leaf"])
    assert np.array_equal(r.where.cpu().numpy().view(np.uint32), want["where"])
    assert np.array_equal(r.visits.cpu().numpy(), want["visits"])
    assert pm.collect() == want["metrics"] and gc.collect() == want["counts"]
    with pytest.raises(amq.TkvAmqError) as e:                     # n_segs + 1 entries, no fewer
        amq.get_keys(w2.plan, w2.filt, t, qb, w2.leaf_kb, key_begin=w2.begin[:-1])
    assert e.value.status == amq.abi.INVALID_ARGUMENT


# ---------------------------------------------------------------------------------------
# 2. early exit
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_early_exit_on_a_tree_of_height_3(oracle, amq, torch, kind):
    X = k(150)
    leaves = [[k(j) for j in range(100, 200, 5)], [k(j) for j in range(500, 600, 5)], [k(120), X, k(510)],
              [k(j) for j in range(101, 140, 2)]]
    w = World(oracle, amq, torch, kind, leaves)
    bottom = {"pivot_keys": [k(0), k(300), k(1000)], "children": [leaf(0), leaf(1)], "page_id": 61,
              "levels": [[{"leaf": 3, "page_id": 7003, "active": 0b01, "flushed": {}}]]}
    mid = {"pivot_keys": [k(0), k(1000)], "children": [bottom], "levels": [], "page_id": 62}
    root = {"pivot_keys": [k(0), k(1000)], "children": [mid],
            "levels": [[{"leaf": 2, "page_id": 7002, "active": 1, "flushed": {}}]]}
    tree = amq.TreeIndex.from_description(root)
    assert tree.nodes[0]["height"] == 3
    qs = [X, k(155), k(505), k(103), k(120), k(7)]
    want = check(amq, torch, w, tree, qs)
    # X is in the root's segment and in the bottom leaf: the root's, after one visit
    assert X in leaves[0] and (int(want["leaf"][0]), int(want["where"][0]), int(want["visits"][0])) == (2, 0, 1)
    assert len(model_one(tree, X)) == 3
    assert (int(want["leaf"][1]), int(want["where"][1])) == (0, 2 << 8 | LEAF_LEVEL)
    assert (int(want["leaf"][3]), int(want["where"][3])) == (3, 2 << 8)
    assert want["metrics"]["total_filter_query_count"] == int(want["visits"].sum()) < sum(len(model_one(tree, q)) for q in qs)


# ---------------------------------------------------------------------------------------
# 3. equality with the chain; key shapes; hash paths
# ---------------------------------------------------------------------------------------
def universe(shape, rng, n=3000):
    if shape in ("k16", "k16_shift4", "q_fixed_leaves_offs"):
        keys = {bytes(rng.integers(0, 256, 16, dtype=np.uint8)) for _ in range(n)}
    elif shape == "k24":
        keys = {bytes(rng.integers(0, 256, 24, dtype=np.uint8)) for _ in range(n)}
    elif shape == "k40":
        keys = {bytes(rng.integers(0, 256, 40, dtype=np.uint8)) for _ in range(n)}
    else:                                                         # "var": 3..45 bytes, some keys prefixes of others
        keys = {bytes(rng.integers(0, 256, int(rng.integers(3, 46)), dtype=np.uint8)) for _ in range(n)}
        for key in list(keys)[:200]:
            keys.add(key + b"\x00")
            keys.add(key[:-1])
    return sorted(keys)


_shape_cases = {}


def shape_case(oracle, amq, torch, kind, shape, bpk=None):
    """Six bottom leaves under two nodes of height 1 under a root with two levels of three segments, whose
    leaves hold samples of the key universe; no flushed bounds.  One segment's tree page id is wrong."""
    if (kind, shape, bpk) in _shape_cases:
        return _shape_cases[(kind, shape, bpk)]
    rng = np.random.default_rng(5 + kind)
    U = universe(shape, rng)
    cuts = [0] + sorted(int(x) for x in rng.choice(np.arange(200, len(U) - 200), 5, replace=False)) + [len(U)]
    while max(b - a for a, b in zip(cuts, cuts[1:])) > 900:
        cuts = [len(U) * j // 6 for j in range(7)]
    bottom = [U[a:b][::2] for a, b in zip(cuts, cuts[1:])]        # every second key: the others are misses
    sep = [U[0][:1]] + [U[c] for c in cuts[1:-1]] + [b"\xff" * 48]
    if shape != "var":
        sep[0], sep[-1] = bytes(len(U[0])), b"\xff" * len(U[0])
    upper = [sorted(set(U[int(x)] for x in rng.integers(0, len(U), 500))) for _ in range(6)]
    root_keys = [sep[0], sep[3], sep[-1]]
    w = World(oracle, amq, torch, kind, bottom + upper, bpk=bpk,
              leaf_form="var" if shape == "q_fixed_leaves_offs" else "auto", shift=4 if shape == "k16_shift4" else 0)

    def seg(j):
        active = 0
        for key in upper[j]:
            active |= 1 << bisect.bisect_right(root_keys[1:-1], key)
        return {"leaf": 6 + j, "page_id": 7006 + j, "active": active, "flushed": {}}

    kids = [{"pivot_keys": sep[0:4], "children": [leaf(i) for i in range(3)], "levels": [], "page_id": 91},
            {"pivot_keys": sep[3:7], "children": [leaf(i) for i in range(3, 6)], "page_id": 92,
             "levels": [[{"leaf": 99, "page_id": 5, "active": 0b101, "flushed": {}}]]}]   # a leaf outside the plan
    tree = amq.TreeIndex.from_description({"pivot_keys": root_keys, "children": kids,
                                           "levels": [[seg(0), seg(1), seg(2)], [seg(3), seg(4), seg(5)]]})
    tree.segments["leaf_page_id"][1] = 4242                       # a wrong page id
    picks = rng.integers(0, len(U), 400)
    qs = [U[int(x)] for x in picks]
    pk = fixed_batch(amq, torch, tree.pivot_keys, 16, 4) if shape == "k16_shift4" else None
    _shape_cases[(kind, shape, bpk)] = (w, tree, qs, pk)
    return _shape_cases[(kind, shape, bpk)]


def chain(amq, torch, w, tree, qb, check_ids):
    walk = amq.walk_paths(tree, qb, want_page_ids=True)
    ids = walk.path_page_id if check_ids else None
    cands = amq.probe_paths(w.plan, w.filt, qb, walk.path_begin, walk.path_leaf, want_entries=True, query_page_ids=ids)
    res = amq.find_keys(w.plan, w.filt, qb, cands, w.leaf_kb, query_page_ids=ids)
    torch.cuda.synchronize()
    return res.key_index.cpu().numpy().view(np.uint64), res.leaf.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", ["k16", "k16_shift4", "k24", "var", "q_fixed_leaves_offs"])
def test_equals_the_chain_and_the_model(oracle, amq, torch, kind, shape):
    w, tree, qs, pk = shape_case(oracle, amq, torch, kind, shape)
    assert not tree.segments["flushed_pivots"].any()
    qb = var_batch(amq, torch, qs) if shape == "var" else fixed_batch(amq, torch, qs, len(qs[0]))
    for check_ids in (False, True):
        want = check(amq, torch, w, tree, qs, qb=qb, pk=pk, check_ids=check_ids)
        key_index, found_leaf = chain(amq, torch, w, tree, qb, check_ids)
        assert np.array_equal(key_index, want["key_index"]) and np.array_equal(found_leaf, want["leaf"])
        n_found = want["counts"]["found_count"]
        assert 100 < n_found < len(qs) and want["counts"]["unsearchable_count"] > 0
        assert want["metrics"]["filter_reject_count"] > 100
        assert (want["metrics"]["page_id_mismatch_count"] > 0) == check_ids


def test_the_variable_length_case_holds_prefix_pairs(oracle, amq, torch):
    w, tree, qs, _ = shape_case(oracle, amq, torch, 0, "var")
    every = sorted(set(key for lv in w.leaves for key in lv))
    assert sum(b.startswith(a) for a, b in zip(every, every[1:])) > 20


@pytest.mark.parametrize("kind,bpk,shape", [(0, 14, "k16"), (0, 14, "k24"), (0, 10, "k40"), (0, 14, "k40"),
                                            (1, 22, "k16"), (1, 12, "k40")])
def test_hash_paths(oracle, amq, torch, kind, bpk, shape):
    """Bloom above 8 hashes (the parked state of 16-byte keys, the ladder of others), Bloom over 40-byte keys
    (the per-entry cache of bit indices), VQF at 22 bits per key (16-bit tags)."""
    w, tree, qs, pk = shape_case(oracle, amq, torch, kind, shape, bpk)
    if kind == 0 and bpk == 14:
        assert (w.plan.segs["hash_count"] > 8).all()
    if kind == 1 and bpk == 22:
        assert (w.plan.segs["tag_bits"] == 16).any()
    want = check(amq, torch, w, tree, qs, qb=fixed_batch(amq, torch, qs, len(qs[0])), pk=pk, check_ids=True)
    assert want["counts"]["found_count"] > 100 and want["metrics"]["filter_reject_count"] > 100


# ---------------------------------------------------------------------------------------
# 4. classes
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_classes(oracle, amq, torch, kind):
    w, tree, qs, pk = shape_case(oracle, amq, torch, kind, "k16")
    qb = fixed_batch(amq, torch, qs, 16)
    plain = check(amq, torch, w, tree, qs, qb=qb)
    ids = check(amq, torch, w, tree, qs, qb=qb, check_ids=True)
    # the segment with the wrong id is searched, never rejected, and an ABSENT there is no false positive
    wrong = int(tree.segments["leaf"][1])
    n_mis = ids["metrics"]["page_id_mismatch_count"]
    assert n_mis > 50 and plain["metrics"]["page_id_mismatch_count"] == 0
    assert ids["counts"]["leaf_search_count"] > plain["counts"]["leaf_search_count"]
    assert ids["counts"]["absent_count"] - ids["metrics"]["filter_false_positive_count"] == \
        n_mis - int((ids["leaf"] == wrong).sum())
    assert np.array_equal(ids["key_index"], plain["key_index"])
    # a leaf outside the plan: no filter page, unsearchable, and the lookup goes on to the child
    assert plain["metrics"]["no_filter_page_count"] == plain["counts"]["unsearchable_count"] > 20
    assert any(vs[-1][2] == "found" and any(v[2] == "unsearchable" for v in vs) for _, vs in plain["rows"])


@pytest.mark.parametrize("kind", KINDS)
def test_no_filters_and_an_empty_leaf(oracle, amq, torch, kind):
    leaves = [[k(j) for j in range(0, 100, 3)], [], [k(j) for j in range(100, 200, 3)], [k(3), k(50), k(150)]]
    node = {"pivot_keys": [k(0), k(60), k(100), k(1000)], "children": [leaf(0), leaf(1), leaf(2)],
            "levels": [[{"leaf": 3, "page_id": 7003, "active": 0b111, "flushed": {}}]]}
    tree = amq.TreeIndex.from_description(node)
    qs = [k(j) for j in range(0, 200)]
    # a plan at 0 bits per key: every visit is "no filter" and every leaf is searched
    w0 = World(oracle, amq, torch, kind, leaves, bpk=0)
    want = check(amq, torch, w0, tree, qs, check_ids=True)
    assert want["metrics"]["no_filter_page_count"] == want["metrics"]["total_filter_query_count"] > 0
    assert want["metrics"]["filter_false_positive_count"] == 0 and want["counts"]["absent_count"] > 100
    assert want["counts"]["leaf_search_count"] == want["counts"]["visit_count"]
    # filters, and an empty leaf under pivot 1: ABSENT if its filter lets a key through, never found
    w = World(oracle, amq, torch, kind, leaves)
    want = check(amq, torch, w, tree, qs)
    assert not (want["leaf"] == 1).any() and (want["leaf"] == 3).sum() == 3
    # no plan at all: every leaf is outside it
    none = World(oracle, amq, torch, kind, leaves)
    none.n = 0
    want = check(amq, torch, none, tree, qs)
    assert (want["leaf"] == NO_LEAF).all() and want["counts"]["unsearchable_count"] == want["counts"]["visit_count"]


# ---------------------------------------------------------------------------------------
# 5. malformed trees
# ---------------------------------------------------------------------------------------
_uneven = {}


def uneven_world(oracle, amq, torch, kind):
    """Keys for every leaf the uneven tree names: bottom leaf i holds four of its ten keys, a segment's leaf a
    third of all keys (so keys sit in several places, and the tree's random bounds flush many of them)."""
    if kind not in _uneven:
        tree = uneven_tree(amq)
        rng = np.random.default_rng(77)
        n_leaves = 15 + len(tree.segments)
        assert sorted(int(s) for s in tree.segments["leaf"]) == list(range(15, n_leaves))
        leaves = [[key16(10 * i + r) for r in (0, 2, 5, 7)] for i in range(15)]
        leaves += [[key16(x) for x in range(150) if rng.random() < 0.33] for _ in range(15, n_leaves)]
        _uneven[kind] = World(oracle, amq, torch, kind, leaves)
    return _uneven[kind]


def uneven_get_queries():
    return uneven_queries() + [key16(x) for x in range(150)]


@pytest.mark.parametrize("kind", KINDS)
def test_the_uneven_tree_with_its_flushed_bounds(oracle, amq, torch, kind):
    w, tree, qs = uneven_world(oracle, amq, torch, kind), uneven_tree(amq), uneven_get_queries()
    want = check(amq, torch, w, tree, qs, check_ids=True)
    assert want["counts"]["flushed_count"] > 10 and want["counts"]["found_count"] > 50
    assert {int(x) >> 8 for x in want["where"] if x != NO_LEAF} == {0, 1, 2}
    assert (want["visits"] < [len(model_one(tree, q)) for q in qs]).sum() > 50


@pytest.mark.parametrize("name", MALFORMED)
def test_malformed_trees_answer_as_the_clamped_model(oracle, amq, torch, name):
    w = uneven_world(oracle, amq, torch, 0)
    check(amq, torch, w, malformed(amq, name), uneven_get_queries())


@pytest.mark.parametrize("kind", KINDS)
def test_a_cycle_ends_after_max_depth_nodes(oracle, amq, torch, kind):
    leaves = [[key16(1), key16(3)], [key16(2)], [key16(2), key16(3), key16(4)]]
    w = World(oracle, amq, torch, kind, leaves)
    node = {"pivot_keys": [key16(0), key16(9)], "children": [leaf(1)],
            "levels": [[{"leaf": 2, "page_id": 7002, "active": 1, "flushed": {0: 1}}]]}
    t = amq.TreeIndex.from_description(node)
    t.nodes["height"][0] = 2
    t.children["index"][0] = 0                                    # the node is its own child
    qs = [key16(j) for j in range(6)]
    want = check(amq, torch, w, t, qs)
    # key 2 is flushed from the segment at every depth and the child leaf is never reached
    assert int(want["visits"][2]) == MAX_DEPTH and want["leaf"][2] == NO_LEAF
    assert want["counts"]["flushed_count"] == MAX_DEPTH
    assert (int(want["leaf"][3]), int(want["where"][3]), int(want["visits"][3])) == (2, 0, 1)
    # no node at all: every result is "none", every visit count 0
    want = check(amq, torch, w, t, qs, n_nodes=0)
    assert (want["leaf"] == NO_LEAF).all() and not want["visits"].any() and want["counts"]["visit_count"] == 0


# ---------------------------------------------------------------------------------------
# 6. batch sizes
# ---------------------------------------------------------------------------------------
def launch_cap():
    """kGetMaxGrid workgroups of kGetThreads lanes, read from the source."""
    from turtle_kv_amd import _build
    with open(os.path.join(_build.HERE, "csrc", "tkv_amq_read.hip")) as f:
        src = f.read()
    return (int(re.search(r"constexpr uint32_t kGetMaxGrid = (\d+);", src).group(1)),
            int(re.search(r"constexpr uint32_t kGetThreads = (\d+);", src).group(1)))


@pytest.mark.parametrize("kind", KINDS)
def test_batch_size_edges(oracle, amq, torch, kind):
    w, tree, (X, Y, Z, E) = flushed_world(oracle, amq, torch, kind)
    # n_queries == 0: OK, nothing written
    empty = amq.KeyBatch(torch.empty((0, 16), dtype=torch.uint8, device="cuda"), 0, 16, None)
    got = run(amq, torch, w, tree, empty)
    assert len(got["leaf"]) == 0 and not got["metrics"].any() and not got["counts"].any()
    # one tile more than one round of the bounded grid: the first workgroup takes a second tile
    grid, threads = launch_cap()
    nq = grid * threads + threads - 3
    base = [X, Y, Z, E, k(601), k(20), k(901), k(333)]
    one = model_batch(w, tree, base)
    pick = np.random.default_rng(9).integers(0, len(base), nq)
    q = np.frombuffer(b"".join(base), np.uint8).reshape(len(base), 16)[pick]
    got = run(amq, torch, w, tree, amq.KeyBatch.fixed(dev(torch, q)))
    for name in ("key_index", "leaf", "where", "visits"):
        assert np.array_equal(got[name].astype(np.int64), one[name].astype(np.int64)[pick]), name
    per = np.bincount(pick, minlength=len(base))
    for names, field in ((METRICS, "metrics"), (COUNTS, "counts")):
        rows = [model_batch(w, tree, [b])[field] for b in base]
        assert dict(zip(names, (int(v) for v in got[field]))) == \
            {n: sum(int(c) * r[n] for c, r in zip(per, rows)) for n in names}, field


# ---------------------------------------------------------------------------------------
# 7. graph capture
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_replays_in_a_graph(oracle, amq, torch, kind):
    w, tree, qs, pk = shape_case(oracle, amq, torch, kind, "k16")
    want = model_batch(w, tree, qs, True)
    qb = fixed_batch(amq, torch, qs, 16)
    bufs = buffers(torch, qb.n)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                    # warm-up on the capture stream
        launch(amq, w, tree, qb, bufs, check_ids=True, stream=s)
    s.synchronize()
    same(read(amq, torch, bufs), want, times=1)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        launch(amq, w, tree, qb, bufs, check_ids=True, stream=s)
    for times in (2, 3):                                          # the counters add on each replay
        bufs["result"][1].fill_(CANARY)
        bufs["visits"][1].view(torch.uint8).fill_(CANARY)
        torch.cuda.synchronize()
        graph.replay()
        same(read(amq, torch, bufs), want, times=times)
