"""GPU: the leaf search (tkv_amq_find_keys / find_keys) -- every candidate of every query searched
by a lower bound over its leaf's sorted keys, the walk ended at the first leaf that holds the key.

The expectation model: per leaf a Python dict from key bytes to the first global index that holds
them (for a sorted leaf, lower-bound-plus-equality is exactly that lookup); the walk, the states
and the counts follow in a few lines.  The end-to-end cases take their filter answers from the CPU
oracle, as tests/test_gpu_path_probe.py does."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# the lower bound's edges: sizes 0..3, a power of two and its neighbours
LEAF_COUNTS = [16384, 1025, 1024, 1023, 3, 2, 1, 0, 8448]
HAND_LEAF = len(LEAF_COUNTS)          # one more, hand-made (below)
E2E_COUNTS = [16384, 16384, 16384, 8448, 0, 5, 1, 9000]
SETTINGS = [(0, 10), (0, 12), (0, 16), (1, 12), (1, 22)]
VQF_CAP = 32704
CANARY = 0xEE
FIELDS = ("leaf_search_count", "found_count", "absent_count", "unsearchable_count")


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available()
    return t


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------
def leaf_dicts(leaves):
    """leaves: per leaf the list of its keys (bytes), in global order.  Per leaf: key -> the first
    global index that holds it; and the global index of every leaf's first key."""
    dicts, begin, g = [], [0], 0
    for keys in leaves:
        d = {}
        for k in keys:
            d.setdefault(k, g)
            g += 1
        dicts.append(d)
        begin.append(g)
    return dicts, np.asarray(begin, np.int64)


def clamp(cand_begin, n_cand):
    cb = np.asarray(cand_begin, np.int64)
    b = np.minimum(cb[:-1], n_cand)
    return b, np.maximum(np.minimum(cb[1:], n_cand), b)


def walk(dicts, queries, cand_begin, cand_leaf, n_cand, find_all, checked=None):
    """What tkv_amq_find_keys must leave behind.  `cover` counts the queries whose clamped range
    holds a position (the state is defined where it is 1; CANARY stays where it is 0); `fp`: the
    searched, absent candidates for which checked[pos] holds."""
    n_segs = len(dicts)
    nq = len(queries)
    out = {"key_index": np.full(nq, -1, np.int64), "leaf": np.full(nq, -1, np.int64),
           "cand": np.full(nq, -1, np.int64), "state": np.full(len(cand_leaf), CANARY, np.uint8),
           "cover": np.zeros(len(cand_leaf), np.int64), "fp": 0}
    cnt = dict.fromkeys(FIELDS, 0)
    b, e = clamp(cand_begin, n_cand)
    for i in range(nq):
        q, done = queries[i], False
        for pos in range(b[i], e[i]):
            out["cover"][pos] += 1
            if done and not find_all:
                out["state"][pos] = 2
                continue
            leaf = int(cand_leaf[pos])
            if leaf >= n_segs:
                out["state"][pos] = 3
                cnt["unsearchable_count"] += 1
                continue
            cnt["leaf_search_count"] += 1
            idx = dicts[leaf].get(q)
            if idx is None:
                out["state"][pos] = 0
                cnt["absent_count"] += 1
                out["fp"] += int(checked is not None and bool(checked[pos]))
            else:
                out["state"][pos] = 1
                if not done:
                    out["key_index"][i], out["leaf"][i], out["cand"][i] = idx, leaf, pos
                    done = True
                    cnt["found_count"] += 1
    out["counts"] = cnt
    return out


# ---------------------------------------------------------------------------------------
# the device side
# ---------------------------------------------------------------------------------------
def fixed_batch(amq, torch, keys, length, shift=0):
    """Fixed-length keys at `shift` bytes past a 256-byte aligned address."""
    n = len(keys)
    buf = torch.zeros(n * length + 256, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 256 == 0
    view = buf[shift:shift + n * length]
    if n:
        view.copy_(torch.from_numpy(np.frombuffer(b"".join(keys), np.uint8).copy()))
    return amq.KeyBatch.fixed(view.view(n, length))


def var_batch(amq, torch, keys):
    """Offsets form; the last key ends at the buffer's last byte."""
    offs = np.zeros(len(keys) + 1, np.int64)
    offs[1:] = np.cumsum([len(k) for k in keys])
    blob = np.frombuffer(b"".join(keys), np.uint8)
    assert len(blob) == offs[-1] and len(blob) > 0
    return amq.KeyBatch.variable(dev(torch, blob.copy()), dev(torch, offs))


def run(amq, torch, plan, qb, cands, kb, n_cand=None, **kw):
    """find_keys with the states and counts; with n_cand: the launch alone over the first n_cand
    positions into canary-filled outputs."""
    fc = amq.FindCounts()
    if n_cand is None:
        res = amq.find_keys(plan, kw.pop("filters", None), qb, cands, kb, want_state=True, counts=fc, **kw)
        raw, state = res.raw, res.state
    else:
        raw = torch.full((16 * qb.n,), CANARY, dtype=torch.uint8, device="cuda")
        state = torch.full((int(cands[1].numel()),), CANARY, dtype=torch.uint8, device="cuda")
        amq.find_keys_device(plan.kind, None, plan.device_segs(), plan.n_segs, qb.data, qb.offsets, qb.stride,
                             qb.n, cands[0], cands[1], None, n_cand, kb.data, kb.offsets, kb.stride, kb.n,
                             None, raw, state, amq.abi.FIND_ALL if kw.get("find_all") else 0, d_counts=fc.counts)
    torch.cuda.synchronize()
    rec = raw.cpu().numpy()[:16 * qb.n].view(amq.abi.FIND_RESULT_DTYPE)
    return {"key_index": rec["key_index"].view(np.int64).copy(), "leaf": rec["leaf"].view(np.int32).astype(np.int64),
            "cand": rec["cand"].view(np.int32).astype(np.int64), "state": state.cpu().numpy(),
            "counts": fc.collect()}


def same(got, want):
    for k in ("key_index", "leaf", "cand"):
        assert np.array_equal(got[k], want[k]), k
    once, never = want["cover"] == 1, want["cover"] == 0
    assert np.array_equal(got["state"][once], want["state"][once])
    assert (got["state"][never] == CANARY).all() or not never.any()
    assert got["counts"] == want["counts"]


def seg_plan(amq, kind, counts):
    """Segments only (key ranges): the hand-made candidate lists need no filter."""
    return amq.plan_filters(kind, counts, 12 if kind else 10, payload_capacity=VQF_CAP if kind else 0)


# ---------------------------------------------------------------------------------------
# 16-byte keys: the main case
# ---------------------------------------------------------------------------------------
def hand_leaf():
    """Keys that differ only in byte 0, 7, 8 or 15, by 0x00 / 0x7f / 0x80 / 0xff there: a
    little-endian or a signed compare orders them wrongly.  The base key twice: a run of equals."""
    base = bytes([0x40] * 16)
    keys = [base, base]
    for p in (0, 7, 8, 15):
        for v in (0x00, 0x7F, 0x80, 0xFF):
            keys.append(base[:p] + bytes([v]) + base[p + 1:])
    return sorted(keys)


class Main:
    pass


_main = {}


def main16(oracle):
    if _main:
        return _main["c"]
    c = Main()
    rng = np.random.default_rng(5)
    bounds = np.concatenate([[0], np.cumsum(LEAF_COUNTS)]).astype(np.uint64)
    keys = oracle.gen_keys16(42, 0, sum(LEAF_COUNTS))
    keys[int(bounds[8]) + 5] = keys[100]                  # one key present in leaves 0 and 8
    dup = keys[100].tobytes()
    oracle.sort_segments(keys, bounds)
    rows = [r.tobytes() for r in keys]
    c.leaves = [rows[int(bounds[s]):int(bounds[s + 1])] for s in range(len(LEAF_COUNTS))] + [hand_leaf()]
    c.counts = LEAF_COUNTS + [len(c.leaves[-1])]
    c.n_segs = len(c.counts)
    c.dicts, c.begin = leaf_dicts(c.leaves)
    c.all_keys = [k for leaf in c.leaves for k in leaf]
    assert dup in c.dicts[0] and dup in c.dicts[8]

    def nudge(k, d):                                      # the last byte one down or up
        return k[:15] + bytes([(k[15] + d) % 256])

    # (query, the leaf it is meant for or -1)
    qs = []
    for s, leaf in enumerate(c.leaves):
        if leaf:
            qs += [(leaf[0], s), (leaf[-1], s), (nudge(leaf[0], -1), s), (nudge(leaf[-1], 1), s)]
    qs += [(c.leaves[6][0], 6)] * 3                       # the key of the 1-key leaf
    for k in c.leaves[HAND_LEAF]:
        qs += [(k, HAND_LEAF), (nudge(k, 1), HAND_LEAF), (nudge(k, -1), HAND_LEAF)]
        qs += [(bytes([(k[0] + 1) % 256]) + k[1:], HAND_LEAF), (k[:7] + bytes([(k[7] + 1) % 256]) + k[8:], HAND_LEAF),
               (k[:8] + bytes([(k[8] - 1) % 256]) + k[9:], HAND_LEAF)]
    hit = rng.integers(0, len(c.all_keys), 40000)
    own = np.searchsorted(c.begin, hit, side="right") - 1
    qs += [(c.all_keys[i], int(s)) for i, s in zip(hit, own)]
    qs += [(r.tobytes(), -1) for r in oracle.gen_keys16(43, 0, 30001)]
    c.i_dup = len(qs)
    qs += [(dup, 0), (dup, 8)]
    c.queries = [q for q, _ in qs]
    c.nq = len(qs)
    assert c.nq > 70000
    # candidate lists: 0..5 random leaves (two of them outside the plan, the empty leaf among
    # them); the leaf a query is meant for first, in the middle or last; the same leaf twice;
    # one 300-long list
    lists = []
    for i, (_, s) in enumerate(qs):
        n = int(rng.integers(0, 6))
        lst = [int(x) for x in rng.integers(0, c.n_segs + 2, 300 if i == 123 else n)]
        if s >= 0 and i % 5 != 4:
            lst.insert((0, len(lst) // 2, len(lst))[i % 3], s)
        if i % 11 == 0 and s >= 0:
            lst += [s, s]
        lists.append(lst)
    lists[c.i_dup] = [0, 8]
    lists[c.i_dup + 1] = [8, 7, 0]
    lens = np.array([len(x) for x in lists])
    c.cand_begin = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    c.cand_leaf = np.array([x for lst in lists for x in lst], np.int64)
    c.n_cand = len(c.cand_leaf)
    assert (lens == 0).sum() > 1000 and lens[123] >= 300 and (c.cand_leaf >= c.n_segs).sum() > 1000
    assert (c.cand_leaf == 7).sum() > 1000
    c.want = {fa: walk(c.dicts, c.queries, c.cand_begin, c.cand_leaf, c.n_cand, fa) for fa in (False, True)}
    _main["c"] = c
    return c


def main_device(amq, torch, c):
    if not hasattr(c, "d_cands"):
        c.d_cands = (dev(torch, c.cand_begin.astype(np.int32)), dev(torch, c.cand_leaf.astype(np.int32)))
        c.qb = fixed_batch(amq, torch, c.queries, 16)
    return c.qb, c.d_cands


def test_the_model_covers_what_the_case_is_there_for(oracle):
    c = main16(oracle)
    w, wa = c.want[False], c.want[True]
    st = w["state"]
    assert all((st == v).sum() > 500 for v in (0, 1, 2, 3))
    assert (w["cover"] == 1).all()
    # the holder first, in the middle and last
    found = w["cand"] >= 0
    b, e = clamp(c.cand_begin, c.n_cand)
    assert (found & (w["cand"] == b)).sum() > 1000 and (found & (w["cand"] == e - 1) & (e - b > 1)).sum() > 1000
    assert (found & (w["cand"] > b) & (w["cand"] < e - 1)).sum() > 1000
    # the key held by two leaves: the first in path order wins, the second is NOT_SEARCHED, with
    # FIND_ALL FOUND, the result the same either way
    i, p = c.i_dup, int(c.cand_begin[c.i_dup])
    assert (w["leaf"][i], w["leaf"][i + 1]) == (0, 8) and list(st[p:p + 2]) == [1, 2]
    assert list(st[p + 2:p + 5]) == [1, 2, 2] and list(wa["state"][p:p + 5]) == [1, 1, 1, 0, 1]
    for k in ("key_index", "leaf", "cand"):
        assert np.array_equal(w[k], wa[k])
    # the run of equal keys: the first of them
    hb = int(c.begin[HAND_LEAF])
    base = bytes([0x40] * 16)
    assert c.all_keys[hb:].count(base) == 2 and c.dicts[HAND_LEAF][base] == hb + c.leaves[HAND_LEAF].index(base)
    assert w["counts"]["found_count"] == found.sum() and wa["counts"]["leaf_search_count"] > w["counts"]["leaf_search_count"]


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("find_all", [False, True])
def test_main_case_fast_mode(oracle, amq, torch, kind, find_all):
    c = main16(oracle)
    qb, cands = main_device(amq, torch, c)
    kb = fixed_batch(amq, torch, c.all_keys, 16)
    assert kb.data.data_ptr() % 16 == 0 and qb.data.data_ptr() % 16 == 0
    same(run(amq, torch, seg_plan(amq, kind, c.counts), qb, cands, kb, find_all=find_all), c.want[find_all])


@pytest.mark.parametrize("shape", ["leaves+8", "queries+8", "leaves in offsets form", "both in offsets form"])
@pytest.mark.parametrize("find_all", [False, True])
def test_main_case_generic_path(oracle, amq, torch, shape, find_all):
    c = main16(oracle)
    qb, cands = main_device(amq, torch, c)
    kb = fixed_batch(amq, torch, c.all_keys, 16)
    if shape == "leaves+8":
        kb = fixed_batch(amq, torch, c.all_keys, 16, shift=8)
        assert kb.data.data_ptr() % 16 == 8
    elif shape == "queries+8":
        qb = fixed_batch(amq, torch, c.queries, 16, shift=8)
    else:
        kb = var_batch(amq, torch, c.all_keys)
        if shape == "both in offsets form":
            qb = var_batch(amq, torch, c.queries)
    same(run(amq, torch, seg_plan(amq, 0, c.counts), qb, cands, kb, find_all=find_all), c.want[find_all])


# ---------------------------------------------------------------------------------------
# other key shapes
# ---------------------------------------------------------------------------------------
SMALL_COUNTS = [1025, 64, 3, 1, 0, 700]


def small_case(length):
    """Keys of `length` bytes (None: 0..40) that share prefixes of every length, so that a compare
    is decided in any word, in the tail bytes or by the length; sorted per leaf by bytes."""
    rng = np.random.default_rng(100 + (length or 0))
    pool = [rng.integers(0, 256, 40, dtype=np.uint8).tobytes() for _ in range(3)]

    def key():
        n = int(rng.integers(0, 41)) if length is None else length
        j = int(rng.integers(0, n + 1))
        k = pool[int(rng.integers(0, 3))][:j] + rng.integers(0, 256, n - j, dtype=np.uint8).tobytes()
        if n > j and rng.integers(0, 2):
            k = k[:j] + bytes([(pool[0][j] + int(rng.integers(0, 3)) - 1) % 256]) + k[j + 1:]
        return k

    leaves = []
    for s, n in enumerate(SMALL_COUNTS):
        ks = set()
        if length is None and n >= 64:
            # prefix pairs: the length decides
            ks.add(b"")
            for _ in range(8):
                k = key()[:39]
                ks.update([k, k + b"\0", k + b"\xff"])
        while len(ks) < n:
            ks.add(key())
        leaves.append(sorted(ks)[:n])
    assert [len(x) for x in leaves] == SMALL_COUNTS
    if length is None:
        assert len(leaves[-1][-1]) > 0                    # (the last key ends at the buffer's end)
    dicts, begin = leaf_dicts(leaves)
    all_keys = [k for leaf in leaves for k in leaf]
    n_segs = len(leaves)
    qs = [(k, s) for s, leaf in enumerate(leaves) for k in leaf]
    for s, leaf in enumerate(leaves):
        for k in leaf[:40] + leaf[-40:]:
            if k:
                qs += [(k[:-1] + bytes([(k[-1] + 1) % 256]), s), (k[:-1] + bytes([(k[-1] - 1) % 256]), s)]
            if length is None:
                qs += [(k + b"\0", s), (k[:-1], s), (k + b"\xff", s)]
    qs += [(key(), -1) for _ in range(1500)]
    if length is None:
        qs = [(q[:40], s) for q, s in qs]
    lists = []
    for i, (_, s) in enumerate(qs):
        lst = [int(x) for x in rng.integers(0, n_segs + 1, int(rng.integers(0, 5)))]
        if s >= 0 and i % 4 != 3:
            lst.insert((0, len(lst) // 2, len(lst))[i % 3], s)
        lists.append(lst)
    lens = np.array([len(x) for x in lists])
    cand_begin = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    cand_leaf = np.array([x for lst in lists for x in lst], np.int64)
    return leaves, dicts, all_keys, [q for q, _ in qs], cand_begin, cand_leaf


@pytest.mark.parametrize("shape", ["k24 8-aligned", "k24 4-aligned", "stride 20", "variable"])
@pytest.mark.parametrize("find_all", [False, True])
def test_other_key_shapes(amq, torch, shape, find_all):
    length = {"k24 8-aligned": 24, "k24 4-aligned": 24, "stride 20": 20, "variable": None}[shape]
    leaves, dicts, all_keys, queries, cand_begin, cand_leaf = small_case(length)
    want = walk(dicts, queries, cand_begin, cand_leaf, len(cand_leaf), find_all)
    assert want["counts"]["found_count"] > 1000 and want["counts"]["absent_count"] > 1500
    if length is None:
        kb, qb = var_batch(amq, torch, all_keys), var_batch(amq, torch, queries)
        assert len({len(k) for k in all_keys}) == 41 and int(kb.offsets[-1]) == kb.data.numel()
    else:
        shift = 4 if shape == "k24 4-aligned" else 0
        kb, qb = fixed_batch(amq, torch, all_keys, length, shift), fixed_batch(amq, torch, queries, length, shift)
        assert kb.data.data_ptr() % 8 == shift
    cands = (dev(torch, cand_begin.astype(np.int32)), dev(torch, cand_leaf.astype(np.int32)))
    same(run(amq, torch, seg_plan(amq, 1, SMALL_COUNTS), qb, cands, kb, find_all=find_all), want)


# ---------------------------------------------------------------------------------------
# malformed lists, the empty call
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("find_all", [False, True])
def test_malformed_lists_answer_as_the_clamped_lists(oracle, amq, torch, find_all):
    c = main16(oracle)
    nq = 600
    queries = c.queries[200:200 + nq]
    cand_begin = c.cand_begin[200:200 + nq + 1] - c.cand_begin[200] + 3      # positions 0..2 belong to nobody
    total = int(cand_begin[-1])
    n_cand = total - 40                                                      # the last ends lie past n_cand
    assert (cand_begin > n_cand).sum() > 3
    lens = np.diff(cand_begin)
    k = next(i for i in range(100, nq) if lens[i] > 0 and lens[i - 1] > 0)
    cand_begin = cand_begin.copy()
    cand_begin[k + 1] = cand_begin[k] - 1     # one pair decreases: query k reads as empty, and
    #                                           query k + 1 covers query k - 1's last position too
    lo = int(c.cand_begin[200])
    cand_leaf = np.concatenate([[0, 0, 0], c.cand_leaf[lo:lo + total - 3], np.zeros(64, np.int64)])
    want = walk(c.dicts, queries, cand_begin, cand_leaf, n_cand, find_all)
    b, e = clamp(cand_begin, n_cand)
    assert e[k] == b[k] and e[-1] == b[-1] and want["cover"].max() == 2 and (want["cover"] == 2).sum() == 1
    assert (want["cover"][:3] == 0).all() and (want["cover"][n_cand:] == 0).all()
    qb = fixed_batch(amq, torch, queries, 16)
    kb = fixed_batch(amq, torch, c.all_keys, 16)
    cands = (dev(torch, cand_begin.astype(np.int32)), dev(torch, cand_leaf.astype(np.int32)))
    got = run(amq, torch, seg_plan(amq, 0, c.counts), qb, cands, kb, n_cand=n_cand, find_all=find_all)
    if want["cover"].max() == 2:
        # the shared position: both queries count it; its state is one of the two
        shared = int(np.flatnonzero(want["cover"] == 2)[0])
        assert got["state"][shared] in (0, 1, 2, 3)
    same(got, want)


def test_empty_call_writes_nothing(oracle, amq, torch):
    c = main16(oracle)
    plan = seg_plan(amq, 0, c.counts)
    kb = fixed_batch(amq, torch, c.all_keys, 16)
    raw = torch.full((64,), CANARY, dtype=torch.uint8, device="cuda")
    state = torch.full((64,), CANARY, dtype=torch.uint8, device="cuda")
    fc = amq.FindCounts()
    cb = torch.zeros(1, dtype=torch.int32, device="cuda")
    amq.find_keys_device(0, None, plan.device_segs(), plan.n_segs, None, None, 16, 0, cb, None, None, 0, kb.data,
                         None, 16, kb.n, None, raw, state, d_counts=fc.counts)
    res = amq.find_keys(plan, None, amq.KeyBatch.fixed(torch.empty((0, 16), dtype=torch.uint8, device="cuda")),
                        (cb, torch.empty(0, dtype=torch.int32, device="cuda")), kb, want_state=True, counts=fc)
    torch.cuda.synchronize()
    assert res.key_index.numel() == 0 and res.state.numel() == 0
    assert (raw == CANARY).all() and (state == CANARY).all() and not any(fc.collect().values())


# ---------------------------------------------------------------------------------------
# end to end: probe_paths -> find_keys on built filters
# ---------------------------------------------------------------------------------------
_e2e = {}


def e2e_inputs(oracle):
    """The path-probe batch of tests/test_gpu_path_probe.py over leaves sorted for both kinds."""
    if "in" in _e2e:
        return _e2e["in"]
    c = Main()
    c.bounds = np.concatenate([[0], np.cumsum(E2E_COUNTS)]).astype(np.uint64)
    c.keys = oracle.gen_keys16(42, 0, sum(E2E_COUNTS))
    oracle.sort_segments(c.keys, c.bounds)
    c.src = np.arange(700, 700 + len(E2E_COUNTS), dtype=np.uint64)
    rng = np.random.default_rng(7)
    c.n_hit, n_miss = 20000, 30001
    c.hit_idx = rng.integers(0, len(c.keys), c.n_hit)
    c.own = np.searchsorted(c.bounds, c.hit_idx, side="right") - 1
    c.q = np.concatenate([c.keys[c.hit_idx], oracle.gen_keys16(43, 0, n_miss)])
    c.nq = len(c.q)
    lens = rng.integers(0, 10, c.nq)
    lens[123] = 300
    c.lens = lens
    c.path_begin = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    c.n_entries = int(c.path_begin[-1])
    c.path_leaf = rng.integers(0, len(E2E_COUNTS) + 2, c.n_entries).astype(np.int64)
    c.has_first = lens[:c.n_hit] > 0
    c.path_leaf[c.path_begin[:c.n_hit][c.has_first]] = c.own[c.has_first]   # a hit's first entry: its own leaf
    c.pair_query = np.repeat(np.arange(c.nq), lens)
    rows = [r.tobytes() for r in c.keys]
    c.dicts, _ = leaf_dicts([rows[int(c.bounds[s]):int(c.bounds[s + 1])] for s in range(len(E2E_COUNTS))])
    c.queries = [r.tobytes() for r in c.q]
    # the leaf search's answer per entry
    c.truth = np.array([l < len(E2E_COUNTS) and c.queries[i] in c.dicts[l]
                        for i, l in zip(c.pair_query, c.path_leaf)], dtype=np.uint8)
    own_of_query = np.full(c.nq, -1, np.int64)
    own_of_query[:c.n_hit] = c.own
    assert np.array_equal(c.truth, (c.path_leaf == own_of_query[c.pair_query]).astype(np.uint8))
    miss_entries = np.flatnonzero(c.pair_query >= c.n_hit)
    inplan = c.path_leaf < len(E2E_COUNTS)
    c.page_ids = np.where(inplan, c.src[np.minimum(c.path_leaf, len(E2E_COUNTS) - 1)], 12345).astype(np.uint64)
    c.page_ids[miss_entries[::7]] += 1000                 # every 7th entry of a miss asks about another page
    _e2e["in"] = c
    return c


def e2e_expect(oracle, c, kind, segs, filt_np, page_ids):
    """From the oracle's filter answers: the six KeyQuery::Metrics counters, the candidate lists and
    the class of every candidate."""
    n_segs = len(E2E_COUNTS)
    inplan = c.path_leaf < n_segs
    src = np.zeros(c.n_entries, np.uint64)
    src[inplan] = segs["src_page_id"][c.path_leaf[inplan]]
    mism = inplan & (src != page_ids) if page_ids is not None else np.zeros(c.n_entries, bool)
    checked = inplan & ~mism
    st, ref = oracle.probe_segments(kind, filt_np, segs["out_offset"], np.ascontiguousarray(c.q[c.pair_query]),
                                    np.where(inplan, c.path_leaf, 0).astype(np.uint32))
    assert st == 0
    pos = checked & (ref == 1)
    m_ref = {"total_filter_query_count": c.n_entries, "no_filter_page_count": int((~inplan).sum()),
             "page_id_mismatch_count": int(mism.sum()), "filter_reject_count": int((checked & (ref == 0)).sum()),
             "filter_positive_count": int(pos.sum()),
             "filter_false_positive_count": int((pos & (c.truth == 0)).sum())}
    keep = np.where(checked, ref, 1) == 1
    cand_begin = np.zeros(c.nq + 1, np.int64)
    np.cumsum(np.bincount(c.pair_query[keep], minlength=c.nq), out=cand_begin[1:])
    return m_ref, cand_begin, c.path_leaf[keep], np.flatnonzero(keep), checked[keep]


def e2e_case(oracle, amq, torch, kind, bpk):
    if (kind, bpk) in _e2e:
        return _e2e[(kind, bpk)]
    c = e2e_inputs(oracle)
    d = Main()
    d.plan = amq.plan_filters(kind, E2E_COUNTS, bpk, payload_capacity=VQF_CAP if kind else 0, src_page_ids=c.src)
    d.kb = amq.KeyBatch.fixed(dev(torch, c.keys))
    d.filt = amq.build_all_filters(d.plan, d.kb)
    d.filt_np = d.filt.cpu().numpy()
    d.qb = amq.KeyBatch.fixed(dev(torch, c.q))
    d.d_begin = dev(torch, c.path_begin.astype(np.int32))
    d.d_leaf = dev(torch, c.path_leaf.astype(np.int32))
    _e2e[(kind, bpk)] = d
    return d


@pytest.mark.parametrize("kind,bpk", SETTINGS)
def test_end_to_end(oracle, amq, torch, kind, bpk):
    c, d = e2e_inputs(oracle), e2e_case(oracle, amq, torch, kind, bpk)
    d_truth = dev(torch, c.truth)
    for page_ids in (None, c.page_ids):
        m_ref, cand_begin, cand_leaf, cand_entry, cand_checked = e2e_expect(oracle, c, kind, d.plan.segs, d.filt_np,
                                                                            page_ids)
        print(kind, bpk, "page ids" if page_ids is not None else "no page ids", m_ref)
        assert m_ref["filter_false_positive_count"] > 0   # (so that equality below is not 0 == 0)
        d_pid = None if page_ids is None else dev(torch, page_ids.view(np.int64))
        n_cand = int(cand_begin[-1])
        # (ii) every candidate searched: KeyQuery::Metrics complete without host truth
        pm = amq.ProbeMetrics()
        res = amq.probe_paths(d.plan, d.filt, d.qb, d.d_begin, d.d_leaf, want_entries=True, query_page_ids=d_pid,
                              metrics=pm)
        assert res.total() == n_cand
        assert np.array_equal(res.cand_begin.cpu().numpy(), cand_begin)
        assert np.array_equal(res.cand_leaf.cpu().numpy()[:n_cand], cand_leaf)
        assert np.array_equal(res.cand_entry.cpu().numpy()[:n_cand], cand_entry)
        assert pm.collect() == {**m_ref, "filter_false_positive_count": 0}
        cands = (res.cand_begin, res.cand_leaf[:n_cand], res.cand_entry[:n_cand])
        fc = amq.FindCounts()
        found = amq.find_keys(d.plan, d.filt, d.qb, cands, d.kb, find_all=True, want_state=True, query_page_ids=d_pid,
                              metrics=pm, counts=fc)
        assert pm.collect() == m_ref
        pm2 = amq.ProbeMetrics()
        amq.probe_paths(d.plan, d.filt, d.qb, d.d_begin, d.d_leaf, query_page_ids=d_pid, truth=d_truth, metrics=pm2)
        assert pm2.collect() == m_ref
        want = walk(c.dicts, c.queries, cand_begin, cand_leaf, n_cand, True, cand_checked)
        assert want["fp"] == m_ref["filter_false_positive_count"]
        assert fc.collect() == want["counts"]
        assert np.array_equal(found.state.cpu().numpy(), want["state"])
        # (iii) the walk that ends at the first hit
        pm3, fc3 = amq.ProbeMetrics(), amq.FindCounts()
        found = amq.find_keys(d.plan, d.filt, d.qb, res if page_ids is None else cands, d.kb, want_state=True,
                              query_page_ids=d_pid, metrics=pm3, counts=fc3)
        want = walk(c.dicts, c.queries, cand_begin, cand_leaf, n_cand, False, cand_checked)
        assert 0 < want["fp"] <= m_ref["filter_false_positive_count"]
        assert pm3.collect() == {**dict.fromkeys(m_ref, 0), "filter_false_positive_count": want["fp"]}
        assert fc3.collect() == want["counts"]
        assert np.array_equal(found.state.cpu().numpy()[:n_cand], want["state"])
        ki, leaf, cand = (t.cpu().numpy().astype(np.int64) for t in (found.key_index, found.leaf, found.cand))
        assert np.array_equal(ki, want["key_index"]) and np.array_equal(leaf, want["leaf"])
        assert np.array_equal(cand, want["cand"])
        # (i) every hit whose path lists its own leaf is found at exactly its own key
        hf = np.flatnonzero(c.has_first)
        assert np.array_equal(ki[hf], c.hit_idx[hf]) and np.array_equal(leaf[hf], c.own[hf])
        assert np.array_equal(cand[hf], cand_begin[hf])
        assert (ki[c.n_hit:] == -1).all() and (leaf[c.n_hit:] == -1).all()


@pytest.mark.parametrize("kind,bpk", [(0, 10), (1, 12)])
def test_opened_filters_with_the_key_csr(oracle, amq, torch, kind, bpk):
    c, d = e2e_inputs(oracle), e2e_case(oracle, amq, torch, kind, bpk)
    res = amq.probe_paths(d.plan, d.filt, d.qb, d.d_begin, d.d_leaf, want_entries=True)
    pm, fc = amq.ProbeMetrics(), amq.FindCounts()
    a = amq.find_keys(d.plan, d.filt, d.qb, res, d.kb, want_state=True, metrics=pm, counts=fc)
    opened = amq.open_filters(kind, d.filt, offsets=d.plan.segs["out_offset"])
    assert opened.all_ok and not opened.plan.segs["key_begin"].any()
    pm2, fc2 = amq.ProbeMetrics(), amq.FindCounts()
    b = amq.find_keys(opened, d.filt, d.qb, res, d.kb, key_begin=c.bounds, want_state=True, metrics=pm2, counts=fc2)
    n_cand = res.total()
    assert torch.equal(a.raw, b.raw) and torch.equal(a.state[:n_cand], b.state[:n_cand])
    assert pm.collect() == pm2.collect() and fc.collect() == fc2.collect()
    assert fc.collect()["found_count"] >= int(c.has_first.sum()) and pm.collect()["filter_false_positive_count"] > 0
    # and the device CSR form
    b2 = amq.find_keys(opened, d.filt, d.qb, res, d.kb, key_begin=dev(torch, c.bounds.view(np.int64)))
    assert torch.equal(a.raw, b2.raw)


@pytest.mark.parametrize("kind", [0, 1])
def test_chain_replays_in_a_graph(oracle, amq, torch, kind):
    c, d = e2e_inputs(oracle), e2e_case(oracle, amq, torch, kind, 12 if kind else 10)
    pm_e, fc_e = amq.ProbeMetrics(), amq.FindCounts()
    res_e = amq.probe_paths(d.plan, d.filt, d.qb, d.d_begin, d.d_leaf, want_entries=True, metrics=pm_e)
    eager = amq.find_keys(d.plan, d.filt, d.qb, res_e, d.kb, want_state=True, metrics=pm_e, counts=fc_e)
    n_cand = res_e.total()
    ws = torch.empty(amq.path_probe_workspace_bytes(c.nq, c.n_entries), dtype=torch.uint8, device="cuda")
    raw = torch.zeros(16 * c.nq, dtype=torch.uint8, device="cuda")
    state = torch.zeros(c.n_entries, dtype=torch.uint8, device="cuda")
    pm, fc = amq.ProbeMetrics(), amq.FindCounts()
    segs = d.plan.device_segs()

    def chain(s):
        res = amq.probe_paths(d.plan, d.filt, d.qb, d.d_begin, d.d_leaf, want_entries=True, metrics=pm,
                              workspace=ws, stream=s)
        amq.find_keys_device(kind, d.filt, segs, d.plan.n_segs, d.qb.data, None, 16, c.nq, res.cand_begin,
                             res.cand_leaf, res.cand_entry, c.n_entries, d.kb.data, None, 16, d.kb.n, None, raw,
                             state, 0, None, pm.counts, fc.counts, stream=s)
        return res

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm-up on the capture stream
        chain(s)
    s.synchronize()
    raw.zero_()
    state.zero_()
    pm.reset()
    fc.reset()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):  # one stream: a linear chain
        res = chain(s)
    graph.replay()
    torch.cuda.synchronize()
    assert res.total() == n_cand
    assert torch.equal(raw, eager.raw) and torch.equal(state[:n_cand], eager.state[:n_cand])
    assert pm.collect() == pm_e.collect() and fc.collect() == fc_e.collect()
