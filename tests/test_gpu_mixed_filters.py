"""The read side over OPENED arrays of mixed geometry, against the CPU oracle over the same bytes.

tkv_amq_open_filters exists so that the read side can work on filter pages it did not build, and
such an array is not uniform: Bloom filters of different hash counts side by side, in any order
and at any 16-byte offset; VQF filters of 8- and 16-bit tags and truncated hashes.  Every
read-side kernel decides per lane what to do from the segment it is asked about, and every other
test here builds its array from one plan, so that all lanes of a wave, all entries of a path and
all units of a workgroup agree.  Here they do not.

1. One Bloom array of 13 segments no single plan produces: hash counts 7, 17, 1, 32, 8, 9, 2, 16,
   3, 11 in that order, an empty leaf at k = 8, a 300-block filter (k = 32) and a 64-byte
   all-zero slot that open_filters refuses; laid out by an offsets list that is not the segment
   order, between poison bytes, with payloads at 16, 32 and 48 modulo 64.  Two copies: the blocks
   as built, and `built | random` at a share of set bits of 0.5^(1/k) per segment, so that members
   pass, about half of the misses pass and every hash index can be the deciding one.
2. open_filters and scan_filters over it; 3. every per-pair and per-path route, the hashed probe
   at k_max 32 / 16 / 8 / 7 / 1, the verify pass at three hints and with overlapping key ranges;
4. find_keys behind probe_paths and get_keys over a tree of height 2 whose every root-to-leaf
   path crosses four hash counts; 5. the same skeleton over a VQF array of five geometries.

The *_inputs tests need no GPU: they state, from the oracle alone, the conditions that make the
GPU tests discriminating.  Every comparison is exact equality."""
import copy

import numpy as np
import pytest

from turtle_kv_amd import abi

from test_gpu_find import leaf_dicts
from test_gpu_find import walk as find_walk
from test_gpu_get import COUNTS, METRICS, VQF_SEED, World, buffers, launch, launch_cap, model_batch, read
from test_gpu_get import same as get_same
from test_gpu_parity import _bloom_seed
from test_gpu_path_probe import compact
from test_gpu_read_side import (BLOOM, VQF, Routes, assert_routes_populated, batch, check_hashed, check_paths,
                                check_probe, check_verify, dev, ids, make_routes, shape_keys, table16, take)
from test_gpu_verify import assert_result, clamped_ranges, fold, pairs
from test_gpu_verify import run as verify_run
from test_gpu_walk import fixed_batch, var_batch
from test_open_scan_abi import ref_scan

gpu = pytest.mark.gpu

POISON = 0xA5                       # between the payloads: neither kind's magic, not a zero slot
SRC0 = 8100                         # segment s was built for page SRC0 + s
OUTSIDE = 99                        # a leaf index past every plan here
OPENED_FIELDS = ("n_blocks", "hash_count", "tag_bits", "hash_val_shift", "mod_magic", "src_page_id",
                 "payload_bytes", "page_flags")
STAT_FIELDS = ("occupied", "header_items", "full_blocks", "empty_blocks", "max_block", "bad_blocks")
HOST_SHAPES = ("k24", "s20", "k40", "var")
DEVICE_SHAPES = ("k24", "k24off4", "s20", "k40", "var")


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available()
    return t


def rows16(keys):
    return np.frombuffer(b"".join(keys), np.uint8).reshape(len(keys), 16).copy() if len(keys) else \
        np.zeros((0, 16), np.uint8)


def rand_keys(rng, n, length=16):
    return sorted({bytes(rng.integers(0, 256, length, dtype=np.uint8)) for _ in range(n)})


# ---------------------------------------------------------------------------------------
# an array of filters that no one plan produces
# ---------------------------------------------------------------------------------------
def one_filter(oracle, amq, kind, keys, bpk, cap, src):
    """(the segment of a one-leaf plan at this setting, the oracle's payload of `keys`)."""
    n = len(keys)
    sg = amq.plan_filters(kind, [n], bpk, payload_capacity=cap, src_page_ids=[src]).segs[0]
    arr = rows16(keys) if n else np.zeros((1, 16), np.uint8)
    if kind == BLOOM:
        st, ref = oracle.bloom_build(arr, n, bpk, src_page_id=src)
    else:
        st, ref, pl = oracle.vqf_build(arr, n, bpk, cap, src_page_id=src)
        ref = ref[:pl.payload_used]
    assert st == 0 and len(ref) == int(sg["payload_bytes"])
    return sg, np.ascontiguousarray(ref)


def header_items(kind, payload):
    """Bloom item_count (@48) / VQF nelts (@64): what an opened segment's n_keys is."""
    at = 48 if kind == BLOOM else 64
    return int(np.frombuffer(payload[at:at + 8].tobytes(), "<u8")[0])


def lay_out(amq, kind, segs_of, payloads, place, gaps):
    """The payloads in one poison-filled buffer, in `place` order with gaps[i] bytes in front of the
    i-th placed; payloads[s] None: a zeroed slot of header size.  Returns (bytes, the plan
    open_filters must reconstruct: every field the header says an opened segment gets from the
    plan segment that produced the payload, out_offset from the list, the rest zero)."""
    n, slot, pos = len(payloads), (64 if kind == BLOOM else 96), 0
    offs = np.zeros(n, np.uint64)
    for s, gap in zip(place, gaps):
        pos += gap
        offs[s] = pos
        pos += slot if payloads[s] is None else len(payloads[s])
    assert sorted(place) == list(range(n)) and not (offs % 16).any()
    host = np.full(pos + 32, POISON, np.uint8)
    segs = np.zeros(n, abi.SEGMENT_DTYPE)
    segs["out_offset"] = offs
    for s, p in enumerate(payloads):
        o = int(offs[s])
        if p is None:
            host[o:o + slot] = 0
            continue
        host[o:o + len(p)] = p
        for name in OPENED_FIELDS:
            segs[name][s] = segs_of[s][name]
        segs["n_keys"][s] = header_items(kind, p)
    plan = amq.FilterPlan(kind, 0, segs, len(host), 0, int(segs["n_blocks"].max()), int(segs["n_keys"].sum()))
    return host, plan


def or_random(rng, payload, k):
    """The Bloom payload with its blocks overwritten as built | random: random zero bits set until
    the share of set bits is 0.5^(1/k) (to one bit)."""
    bits = np.unpackbits(payload[64:], bitorder="little")
    zeros = np.flatnonzero(bits == 0)
    add = int(round(len(bits) * 0.5 ** (1.0 / k))) - (len(bits) - len(zeros))
    assert 0 <= add <= len(zeros), "the built filter is already denser than 0.5^(1/k)"
    bits[rng.choice(zeros, add, replace=False)] = 1
    out = payload.copy()
    out[64:] = np.packbits(bits, bitorder="little")
    return out


def weighted_draw(rng, weights):
    p = np.asarray(weights, np.float64) / np.sum(weights)
    return lambda size: rng.choice(len(p), size, p=p)


# ---------------------------------------------------------------------------------------
# 1. the mixed Bloom array
# ---------------------------------------------------------------------------------------
K_ORDER = [7, 17, 1, 32, 8, 9, 2, 16, 3, 11]
EMPTY, BIG, REFUSED = 10, 11, 12                       # an empty leaf at k = 8, 300 blocks at k = 32, the zero slot
SEG_K = K_ORDER + [8, 32, 0]
N_B = len(SEG_K)
BIG_BPK, BIG_KEYS = 64, 2400                           # 153,600 bits: 300 blocks
PLACE_B = [5, 12, 0, 9, 3, 11, 7, 1, 10, 4, 8, 2, 6]   # the order in the buffer
GAPS_B = [16, 32, 16, 0, 64, 48, 16, 32, 80, 16, 0, 48, 32]
CUTS = [0, 1200, 1202, 3002, 3902, 5402, 6000]         # the child leaves 4 .. 9: every second key of these slices
NQ_B, NQ_SHAPE, N_MEMBER_Q = 24000, 3000, 2000
K_MAXES = (32, 16, 8, 7, 1)
# the hand-made paths, in entry order
ASCENDING = [2, 6, 8, 0, 4, EMPTY, 5, 9, 7, 1, 3, BIG]
HAND_B = {"ascending": ASCENDING, "descending": ASCENDING[::-1], "tail": [0, 1, 4, 3, 2],
          "holes": [5, REFUSED, N_B + 3, 1], "alternating": [4, 5] * 18}
HAND_K = {"ascending": [1, 2, 3, 7, 8, 8, 9, 11, 16, 17, 32, 32], "descending": [32, 32, 17, 16, 11, 9, 8, 8, 7, 3, 2, 1],
          "tail": [7, 17, 8, 32, 1], "holes": [9, None, None, 17], "alternating": [8, 9] * 18}

_b = {}


def only_zero_share(k):
    """The share of pairs whose one zero bit is bit j, at a share of set bits of 0.5^(1/k)."""
    p = 0.5 ** (1.0 / k)
    return p ** (k - 1) * (1 - p)


def hand_paths(hand, first, n):
    """Queries first .. first + n - 1 take the hand-made paths in turn."""
    names = list(hand)
    return {first + i: hand[names[i % len(names)]] for i in range(n)}


def bloom_mixed(oracle, amq):
    if "m" in _b:
        return _b["m"]
    m, rng = Routes(), np.random.default_rng(20261021)
    hash_count = oracle.lib().tkvo_bloom_hash_count
    m.bpk = [BIG_BPK if s == BIG else next(b for b in range(1, 47) if hash_count(b) == k) if k else 0
             for s, k in enumerate(SEG_K)]
    assert hash_count(BIG_BPK) == 32
    # the leaves: 4 .. 9 cover the key universe slice by slice (the tree's child leaves), 0 .. 3 and
    # the refused slot's leaf hold samples of all of it (the tree's segments)
    m.U = U = rand_keys(rng, CUTS[-1] + 40)[:CUTS[-1]]
    sample = lambda n: sorted({U[int(x)] for x in rng.integers(0, len(U), n)})
    m.leaves = [sample(700), sample(1000), sample(280), sample(500)] + \
        [U[a:b][::2] for a, b in zip(CUTS, CUTS[1:])] + [[], rand_keys(rng, BIG_KEYS), sample(150)]
    m.segs_of, m.built_p, m.synth_p = [], [], []
    for s, k in enumerate(SEG_K):
        if s == REFUSED:
            sg, ref = None, None
        else:
            sg, ref = one_filter(oracle, amq, BLOOM, m.leaves[s], m.bpk[s], 0, SRC0 + s)
            assert int(sg["hash_count"]) == k
        m.segs_of.append(sg)
        m.built_p.append(ref)
        m.synth_p.append(None if ref is None else or_random(rng, ref, k))
    m.built, m.plan = lay_out(amq, BLOOM, m.segs_of, m.built_p, PLACE_B, GAPS_B)
    m.synth, plan2 = lay_out(amq, BLOOM, m.segs_of, m.synth_p, PLACE_B, GAPS_B)
    assert plan2.segs.tobytes() == m.plan.segs.tobytes()
    m.offsets = m.plan.segs["out_offset"].copy()
    # (query, leaf) pairs: each segment's share is what its rarest "only zero bit" needs
    m.weights = [0 if k == 0 else 45 / only_zero_share(k) for k in SEG_K]
    m.weights[REFUSED] = 300
    m.weights.append(300)                                  # index N_B: a leaf outside the plan
    m.members = [key for lv in m.leaves for key in lv]
    _b["m"] = m
    return m


def bloom_q16(oracle, amq):
    """The 16-byte batch: member keys then random ones, the oracle's table over the built | random
    copy, and every route over it (the hand-made paths at queries 1000 .. 1999: member keys)."""
    if "q16" not in _b:
        m, c, rng = bloom_mixed(oracle, amq), Routes(), np.random.default_rng(77001)
        c.q = np.concatenate([rows16(m.members)[rng.integers(0, len(m.members), N_MEMBER_Q)],
                              rng.integers(0, 256, (NQ_B - N_MEMBER_Q, 16), dtype=np.uint8)])
        c.table = table16(oracle, m.plan, m.synth, c.q)
        draw = weighted_draw(rng, m.weights)
        seg = draw(NQ_B)
        seg[NQ_B // 3], seg[NQ_B // 2] = N_B, N_B + 5
        c.hand = hand_paths(HAND_B, 1000, 1000)
        c.state = rng.bit_generator.state
        c.r = make_routes(rng, m.plan, c.table, seg, draw, long_at=123, fixed_paths=c.hand)
        _b["q16"] = c
    return _b["q16"]


def bloom_shape(oracle, amq, shape):
    """The other key shapes: oracle.bloom_query per key and filter (the hand-made paths at queries
    1000 .. 1499)."""
    if shape not in _b:
        m, c = bloom_mixed(oracle, amq), Routes()
        rng = np.random.default_rng(77100 + HOST_SHAPES.index(shape))
        c.keys = shape_keys(rng, shape, NQ_SHAPE)
        c.table = np.ones((NQ_SHAPE, N_B), np.uint8)
        for s, p in enumerate(m.synth_p):
            if p is not None:
                c.table[:, s] = [oracle.bloom_query(p, bytes(key)) for key in c.keys]
        draw = weighted_draw(rng, m.weights)
        seg = draw(NQ_SHAPE)
        seg[NQ_SHAPE // 3], seg[NQ_SHAPE // 2] = N_B, N_B + 5
        c.hand = hand_paths(HAND_B, 1000, 500)
        c.r = make_routes(rng, m.plan, c.table, seg, draw, long_at=123, fixed_paths=c.hand)
        _b[shape] = c
    return _b[shape]


def verify_case(oracle, plan, host, leaves, n_strangers, seed):
    """Every leaf's own keys followed by keys it does not hold, behind a CSR; the oracle's table of
    all of them, the expectation per leaf, and the same with overlapping ranges (key_begin that
    falls back to 0 at every second leaf, so that the others cover every key: more units than the
    grid has workgroups, and a workgroup takes units of different leaves in turn)."""
    rng, v = np.random.default_rng(seed), Routes()
    parts = [rows16(lv + rand_keys(rng, n_strangers)) for lv in leaves]
    v.keys = np.concatenate(parts)
    v.v_begin = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.uint64)
    v.table = table16(oracle, plan, host, v.keys)
    built = plan.segs["hash_count" if plan.kind == BLOOM else "tag_bits"] != 0
    v.flags = np.where(built, 0, abi.VERIFY_NO_FILTER).astype(np.uint32)

    def expect(key_begin):
        idx, seg = pairs(clamped_ranges(plan, len(v.keys), key_begin))
        keep = built[seg]                                  # (a leaf without a filter has nothing checked)
        return fold(plan.n_segs, idx[keep], seg[keep], v.table[idx[keep], seg[keep]])

    v.v_missing, v.v_first = expect(v.v_begin)
    n = len(v.keys)
    v.overlap = []
    for parity in (0, 1):
        kb = np.array([0 if s % 2 == parity else n for s in range(plan.n_segs + 1)], np.uint64)
        v.overlap.append((kb,) + expect(kb))
    return v


def bloom_verify(oracle, amq):
    if "verify" not in _b:
        m = bloom_mixed(oracle, amq)
        _b["verify"] = verify_case(oracle, m.plan, m.synth, m.leaves, 300, 77200)
    return _b["verify"]


def bit_table(q16):
    """python-xxhash: (h0 per query as Python ints, the 32 bit indices per query)."""
    import xxhash
    rows = [r.tobytes() for r in q16]
    h0 = [xxhash.xxh64_intdigest(b, _bloom_seed(0)) for b in rows]
    bit = np.empty((len(rows), 32), np.int64)
    bit[:, 0] = [h & 511 for h in h0]
    for j in range(1, 32):
        seed = _bloom_seed(j)
        bit[:, j] = [xxhash.xxh64_intdigest(b, seed) & 511 for b in rows]
    return h0, bit


def bit_values(plan, all_bits, h0, bit, query, seg):
    """For pairs on segments with a filter: (the k tested bits' values, padded with ones, [n, 32];
    which of the 32 are tested)."""
    sg = plan.segs[seg]
    blk = np.array([(h0[q] * int(nb)) >> 64 for q, nb in zip(query, sg["n_blocks"])], np.int64)
    val = all_bits[(8 * (sg["out_offset"].astype(np.int64) + 64 + 64 * blk))[:, None] + bit[query]]
    tested = np.arange(32)[None, :] < sg["hash_count"].astype(np.int64)[:, None]
    return np.where(tested, val, 1), tested


def decides(plan, all_bits, h0, bit, query, seg):
    """[n_segs, 32]: the pairs on segment s whose only zero bit is bit j."""
    keep = (seg < plan.n_segs) & (plan.segs["hash_count"][np.minimum(seg, plan.n_segs - 1)] != 0)
    query, seg = query[keep], seg[keep]
    val, _ = bit_values(plan, all_bits, h0, bit, query, seg)
    only = (val == 0).sum(axis=1) == 1
    out = np.zeros((plan.n_segs, 32), np.int64)
    np.add.at(out, (seg[only], np.argmin(val[only], axis=1)), 1)
    return out


# ---------------------------------------------------------------------------------------
# the tree over the Bloom array
# ---------------------------------------------------------------------------------------
def tree_seg(s, active=0b11, flushed=None):
    return {"leaf": s, "page_id": SRC0 + s, "active": active, "flushed": flushed or {}}


def tree_leaf(s):
    return {"leaf": s, "page_id": SRC0 + s}


def bloom_tree(oracle, amq):
    """Height 2.  The root: level 0 the segments of leaves 0, 1, 2 (k = 7, 17, 1), level 1 those of
    leaf 3 (k = 32), of the refused slot and of a leaf outside the plan; two nodes below it over the
    child leaves 4, 5, 6 (k = 8, 9, 2) and 7, 8, 9 (k = 16, 3, 11), the second with the empty leaf's
    segment: every root-to-leaf path crosses 7, 17, 1, 32 and its child's count.  A few flushed
    bounds; the segment of leaf 1 under a wrong tree page id."""
    if "tree" not in _b:
        m, t = bloom_mixed(oracle, amq), Routes()
        U, lo, hi = m.U, bytes(16), b"\xff" * 16
        sep = [lo] + [U[c] for c in CUTS[1:-1]] + [hi]
        kids = [{"pivot_keys": sep[0:4], "children": [tree_leaf(s) for s in (4, 5, 6)], "levels": [], "page_id": 91},
                {"pivot_keys": sep[3:7], "children": [tree_leaf(s) for s in (7, 8, 9)], "page_id": 92,
                 "levels": [[tree_seg(EMPTY, 0b111)]]}]
        root = {"pivot_keys": [lo, sep[3], hi], "children": kids,
                "levels": [[tree_seg(0, flushed={0: 1000}), tree_seg(1, flushed={1: 800}), tree_seg(2)],
                           [tree_seg(3, flushed={1: 450}), tree_seg(REFUSED),
                            {"leaf": OUTSIDE, "page_id": 5, "active": 0b11, "flushed": {}}]]}
        t.tree = amq.TreeIndex.from_description(root)
        assert t.tree.nodes[0]["height"] == 2 and int(t.tree.segments["leaf"][1]) == 1
        t.tree.segments["leaf_page_id"][1] = 4242
        rng = np.random.default_rng(77300)
        stored = [U[int(x)] for x in rng.integers(0, len(U), 400)] + \
            [m.leaves[REFUSED][int(x)] for x in rng.integers(0, len(m.leaves[REFUSED]), 40)]
        t.queries = {"k16": stored + [bytes(r) for r in rng.integers(0, 256, (100, 16), dtype=np.uint8)],
                     "k40": [bytes(r) for r in rng.integers(0, 256, (300, 40), dtype=np.uint8)],
                     "var": [bytes(rng.integers(0, 256, int(n), dtype=np.uint8)) for n in rng.integers(1, 72, 300)] +
                     stored[:60]}
        t.worlds = {"built": World.over(oracle, m.plan, m.leaves, m.built_p),
                    "synth": World.over(oracle, m.plan, m.leaves, m.synth_p)}
        t.want = {}
        _b["tree"] = t
    return _b["tree"]


def tree_want(t, copy_name, shape, check_ids):
    key = (copy_name, shape, check_ids)
    if key not in t.want:
        t.want[key] = model_batch(t.worlds[copy_name], t.tree, t.queries[shape], check_ids)
    return t.want[key]


# ---------------------------------------------------------------------------------------
# 6. the conditions, from the oracle alone
# ---------------------------------------------------------------------------------------
def test_bloom_array_inputs(oracle, amq):
    m = bloom_mixed(oracle, amq)
    segs = m.plan.segs
    assert list(segs["hash_count"]) == SEG_K and list(segs["hash_count"][:10]) == K_ORDER
    counts = [len(lv) for lv in m.leaves]
    assert all(1 <= c <= 3000 for s, c in enumerate(counts) if s != EMPTY) and counts[EMPTY] == 0 and 1 in counts
    assert len(set(counts)) >= 10                                        # ragged
    assert int(segs["n_blocks"][BIG]) >= 300 > 2 * int(np.delete(segs["n_blocks"], BIG).max())
    assert int(segs["n_blocks"][EMPTY]) == 1 and int(segs["n_keys"][EMPTY]) == 0
    assert not segs[REFUSED].tobytes()[8:].strip(b"\0") and int(segs["out_offset"][REFUSED]) > 0
    assert list(segs["n_keys"][:REFUSED]) == counts[:REFUSED]
    assert list(segs["src_page_id"][:REFUSED]) == list(range(SRC0, SRC0 + REFUSED))
    # the layout: not the segment order, 16-byte offsets on every residue of 64, poison between
    offs = m.offsets.astype(np.int64)
    assert list(np.argsort(offs)) == PLACE_B and PLACE_B != sorted(PLACE_B)
    filters = np.arange(N_B) != REFUSED
    for residue in (0, 16, 32, 48):
        assert ((offs % 64 == residue) & filters & (segs["n_keys"] > 100)).sum() >= 1, residue
    assert len(m.built) < 200 * 1024 and len(m.built) == len(m.synth)
    used = np.zeros(len(m.built), bool)
    for s in range(N_B):
        size = 64 if s == REFUSED else int(segs["payload_bytes"][s])
        assert not used[offs[s]:offs[s] + size].any()
        used[offs[s]:offs[s] + size] = True
    assert (m.built[~used] == POISON).all() and (m.synth[~used] == POISON).all() and (~used).sum() >= 400
    assert not m.built[offs[REFUSED]:offs[REFUSED] + 64].any()
    # the two copies: the same headers, built bits kept, the share of set bits 0.5^(1/k)
    for s, k in enumerate(SEG_K):
        if k == 0:
            continue
        a, b = m.built_p[s], m.synth_p[s]
        assert a[:64].tobytes() == b[:64].tobytes() and ((a & b) == a).all()
        share = np.unpackbits(b[64:]).mean()
        assert abs(share - 0.5 ** (1.0 / k)) <= 0.02, (s, k, share)
    # members pass both copies
    for host in (m.built, m.synth):
        for s, lv in enumerate(m.leaves):
            if s != REFUSED and lv:
                st, res = oracle.probe_segments(BLOOM, host, m.offsets, rows16(lv), np.full(len(lv), s, np.uint32))
                assert st == 0 and res.all()


def test_bloom_q16_inputs(oracle, amq):
    """About half of the pairs on every segment pass; python-xxhash gives the oracle's table; and on
    every segment with a filter every hash index j < k is, for at least 20 pairs of each pair route
    and 5 entries of the paths, the only one whose bit is zero."""
    m, c = bloom_mixed(oracle, amq), bloom_q16(oracle, amq)
    r, plan = c.r, m.plan
    assert_routes_populated(r, plan)
    built = np.flatnonzero(plan.segs["hash_count"] != 0)
    for s in built:
        for seg, ref in ((r.seg, r.ref), (r.pair_seg, r.pair_ref)):
            if len(m.leaves[s]):
                assert 0.35 <= ref[seg == s].mean() <= 0.65, (s, ref[seg == s].mean())
    assert 0.35 <= r.share <= 0.65
    # the second evaluation: the whole table
    h0, bit = bit_table(c.q)
    all_bits = np.unpackbits(m.synth, bitorder="little")
    every = np.arange(NQ_B)
    for s in built:
        val, tested = bit_values(plan, all_bits, h0, bit, every, np.full(NQ_B, s))
        assert tested.sum(axis=1).min() == tested.sum(axis=1).max() == SEG_K[s]
        assert np.array_equal(val.all(axis=1), c.table[:, s] == 1), s
    assert c.table[:, REFUSED].all()
    # every index decides
    for name, query, seg, bound in (("one leaf per query", every, r.seg, 20), ("pairs", r.pair_query, r.pair_seg, 20),
                                    ("path entries", r.path_query, r.path_leaf, 5)):
        d = decides(plan, all_bits, h0, bit, query, seg)
        for s in built:
            assert d[s, :SEG_K[s]].min() >= bound, (name, s, SEG_K[s], list(d[s, :SEG_K[s]]))
            assert not d[s, SEG_K[s]:].any()
    # the hand-made paths are what their names say, and all of them are there
    k_of = lambda leaf: int(plan.segs["hash_count"][leaf]) or None if leaf < N_B else None
    seen = set()
    for qi, leaves in c.hand.items():
        got = [int(x) for x in r.path_leaf[r.path_begin[qi]:r.path_begin[qi + 1]]]
        name = next(n for n, p in HAND_B.items() if p == got)
        assert [k_of(x) for x in got] == HAND_K[name]
        seen.add(name)
    assert seen == set(HAND_B) and len(HAND_B["alternating"]) > 32 and len(HAND_B["alternating"]) != 40
    # at every k_max below 32 some pairs are classed "no filter" by their filter's k, others tested
    for k_max in K_MAXES:
        too_long = plan.segs["hash_count"][np.minimum(r.seg, N_B - 1)] > k_max
        assert too_long.any() == (k_max < 32) and not too_long.all()


@pytest.mark.parametrize("shape", HOST_SHAPES)
def test_bloom_shape_inputs(oracle, amq, shape):
    m, c = bloom_mixed(oracle, amq), bloom_shape(oracle, amq, shape)
    assert_routes_populated(c.r, m.plan)
    assert 0.35 <= c.r.share <= 0.65, c.r.share
    built = m.plan.segs["hash_count"] != 0
    assert (c.r.v_missing[built] > 0).all() and not c.r.v_missing[~built].any()
    lens = np.diff(c.r.path_begin)
    assert sorted({int(lens[qi]) for qi in c.hand}) == sorted({len(p) for p in HAND_B.values()})
    if shape == "var":
        size = [len(key) for key in c.keys]
        assert size[:4] == [0, 31, 32, 33] and sum(n < 32 for n in size) > 1000 and sum(n >= 32 for n in size) > 1000
        assert sum(len(c.keys[qi]) >= 32 for qi in c.hand) > 100           # the bit-index cache, on the hand-made paths


def test_bloom_verify_inputs(oracle, amq):
    m, v = bloom_mixed(oracle, amq), bloom_verify(oracle, amq)
    built = m.plan.segs["hash_count"] != 0
    own = np.array([len(lv) for lv in m.leaves])
    # strangers only are rejected, in every leaf with a filter
    assert (v.v_missing[built] > 50).all() and not v.v_missing[~built].any()
    assert (v.v_first[built].astype(np.int64) >= (v.v_begin[:-1].astype(np.int64) + own)[built]).all()
    # the hints: everything in LDS; the 300-block filter alone in global memory; all but one-block filters
    nb = m.plan.segs["n_blocks"]
    assert m.plan.max_seg_blocks == nb.max() == nb[BIG] and (np.delete(nb, BIG) < 100).all() and (nb == 1).sum() >= 2
    # overlapping ranges: more units than workgroups (div_up(n_keys, chunk) + n_segs, chunks of 2,048 keys)
    n, chunk = len(v.keys), 2048
    seen = np.zeros(N_B, bool)
    for kb, missing, first in v.overlap:
        ranges = clamped_ranges(m.plan, n, kb)
        units = sum(-(-(e - b) // chunk) for (b, e), has in zip(ranges, built) if has)
        assert units > -(-n // chunk) + N_B
        full = np.array([e - b == n for b, e in ranges])
        assert (missing[full & built] > 1000).all() and not missing[~(full & built)].any()
        seen |= full
    assert seen.all()


def test_bloom_tree_inputs(oracle, amq):
    m, t = bloom_mixed(oracle, amq), bloom_tree(oracle, amq)
    assert max(len(lv) for s, lv in enumerate(m.leaves) if s != BIG) <= 1000
    named = {int(x) for x in t.tree.segments["leaf"]} | {int(x) for x in t.tree.children["index"][-6:]}
    assert named == {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, EMPTY, REFUSED, OUTSIDE} and len(t.tree.flushed_bounds) == 3
    # every root-to-leaf path crosses at least three hash counts, one of them above 8
    from test_gpu_walk import model_one
    for q in t.queries["k16"]:
        ks = {SEG_K[e[0]] for e in model_one(t.tree, q) if e[0] < N_B} - {0}
        assert len(ks) >= 3 and max(ks) > 8
        assert {e[0] for e in model_one(t.tree, q)} >= {REFUSED, OUTSIDE}
    for name in ("built", "synth"):
        for shape in ("k16", "k40", "var"):
            for check_ids in (False, True):
                want = tree_want(t, name, shape, check_ids)
                assert (want["metrics"]["page_id_mismatch_count"] > 0) == check_ids
                if shape == "k40":                                         # (no 40-byte key is stored)
                    assert want["counts"]["found_count"] == 0 and want["metrics"]["filter_reject_count"] > 0
                    continue
                if shape == "var":
                    assert want["counts"]["found_count"] > 20 and want["metrics"]["filter_reject_count"] > 0
                    continue
                every = {**want["metrics"], **want["counts"]}
                every.pop("page_id_mismatch_count")
                assert all(v > 0 for v in every.values()), (name, shape, check_ids, every)
    want = tree_want(t, "synth", "k16", False)
    assert want["metrics"]["filter_false_positive_count"] > 100 and want["metrics"]["filter_reject_count"] > 100
    assert want["counts"]["found_count"] > 100 and want["counts"]["flushed_count"] > 10


# ---------------------------------------------------------------------------------------
# 2. opening it
# ---------------------------------------------------------------------------------------
_dev = {}


def opened_on_device(amq, torch, m, name, kind, refused):
    """The two copies on the device and the array opened there (the as-built copy's: the two share
    their headers); the opened segments are the host's, field by field."""
    if name not in _dev:
        d = Routes()
        d.built, d.synth = dev(torch, m.built), (dev(torch, m.synth) if hasattr(m, "synth") else None)
        assert d.built.data_ptr() % 64 == 0
        d.opened = amq.open_filters(kind, d.built, offsets=m.offsets)
        want = [abi.OPEN_OK] * m.plan.n_segs
        want[refused] = abi.OPEN_BAD_MAGIC
        assert list(d.opened.status) == want
        assert list(d.opened.summary) == [m.plan.n_segs - 1, 1, 0, 0, 0, 0, 0] and not d.opened.all_ok
        for field in abi.SEGMENT_DTYPE.names:
            assert np.array_equal(d.opened.plan.segs[field], m.plan.segs[field]), field
        assert d.opened.plan.max_seg_blocks == m.plan.max_seg_blocks
        _dev[name] = d
    return _dev[name]


def check_scan(amq, kind, plan, filt, host, refused):
    got = amq.scan_filters(plan, filt)
    for s, sg in enumerate(plan.segs):
        if s == refused:
            assert got[s].tobytes() == bytes(32)
            continue
        o = int(sg["out_offset"])
        want = ref_scan(kind, host[o:o + int(sg["payload_bytes"])])
        for name in STAT_FIELDS:
            assert int(got[name][s]) == want[name], (s, name)
    return got


@gpu
def test_bloom_open_and_scan(oracle, amq, torch):
    m = bloom_mixed(oracle, amq)
    d = opened_on_device(amq, torch, m, "bloom", BLOOM, REFUSED)
    sg = d.opened.plan.segs[REFUSED]
    assert int(sg["out_offset"]) == int(m.offsets[REFUSED]) and not sg.tobytes()[8:].strip(b"\0")
    # the other copy opens alike
    again = amq.open_filters(BLOOM, d.synth, offsets=m.offsets)
    assert again.plan.segs.tobytes() == d.opened.plan.segs.tobytes() and list(again.status) == list(d.opened.status)
    a = check_scan(amq, BLOOM, d.opened.plan, d.built, m.built, REFUSED)
    b = check_scan(amq, BLOOM, d.opened.plan, d.synth, m.synth, REFUSED)
    keys = np.array([len(lv) for lv in m.leaves])
    keys[REFUSED] = 0
    assert list(a["header_items"]) == list(b["header_items"]) == list(keys)
    assert (b["occupied"][:REFUSED] > a["occupied"][:REFUSED]).all() and a["empty_blocks"][EMPTY] == 1


# ---------------------------------------------------------------------------------------
# 3. every per-pair and per-path route over the opened plan
# ---------------------------------------------------------------------------------------
@gpu
def test_bloom_probes_16_byte_keys(oracle, amq, torch):
    m, c = bloom_mixed(oracle, amq), bloom_q16(oracle, amq)
    d = opened_on_device(amq, torch, m, "bloom", BLOOM, REFUSED)
    qb = amq.KeyBatch.fixed(dev(torch, c.q))
    check_probe(amq, torch, d.opened.plan, d.synth, qb, c.r, prefixes=(1, 255, 256, 257))
    check_paths(amq, torch, d.opened.plan, d.synth, qb, c.r)


@gpu
def test_bloom_hashed_probe_16_byte_keys(oracle, amq, torch):
    m, c = bloom_mixed(oracle, amq), bloom_q16(oracle, amq)
    d = opened_on_device(amq, torch, m, "bloom", BLOOM, REFUSED)
    check_hashed(amq, torch, d.opened.plan, d.synth, amq.KeyBatch.fixed(dev(torch, c.q)), c.r, k_maxes=K_MAXES)


@gpu
def test_bloom_verify_16_byte_keys(oracle, amq, torch):
    m, v = bloom_mixed(oracle, amq), bloom_verify(oracle, amq)
    d = opened_on_device(amq, torch, m, "bloom", BLOOM, REFUSED)
    plan, vkb = d.opened.plan, amq.KeyBatch.fixed(dev(torch, v.keys))
    check_verify(amq, torch, plan, d.synth, vkb, v, hints=("plan", 100, 1), flags=v.flags)
    for kb, missing, first in v.overlap:
        for hint in (100, 1):
            res, total = verify_run(amq, torch, plan, d.synth, vkb, key_begin=kb, hint=hint)
            assert_result(res, total, missing, first, flags=v.flags)
    # the copy as built: no key of any leaf is missing where the leaves end at their own keys
    own = np.concatenate([[0], np.cumsum([len(lv) for lv in m.leaves])]).astype(np.uint64)
    res, total = verify_run(amq, torch, plan, d.built, amq.KeyBatch.fixed(dev(torch, rows16(m.members))), key_begin=own)
    assert_result(res, total, np.zeros(N_B, np.uint32), np.full(N_B, abi.NONE_MISSING, np.uint64), flags=v.flags)


@gpu
@pytest.mark.parametrize("shape", DEVICE_SHAPES)
def test_bloom_other_key_shapes(oracle, amq, torch, shape):
    m, c = bloom_mixed(oracle, amq), bloom_shape(oracle, amq, "k24" if shape == "k24off4" else shape)
    d = opened_on_device(amq, torch, m, "bloom", BLOOM, REFUSED)
    plan, qb = d.opened.plan, batch(amq, torch, shape, c.keys)
    assert qb.n == NQ_SHAPE and (shape != "k24off4" or qb.data.data_ptr() % 8 == 4)
    check_probe(amq, torch, plan, d.synth, qb, c.r)
    check_hashed(amq, torch, plan, d.synth, qb, c.r, k_maxes=K_MAXES)
    check_paths(amq, torch, plan, d.synth, qb, c.r)
    flags = np.where(plan.segs["hash_count"] != 0, 0, abi.VERIFY_NO_FILTER).astype(np.uint32)
    check_verify(amq, torch, plan, d.synth, batch(amq, torch, shape, take(c.keys, c.r.v_order)), c.r,
                 hints=("plan", 100, 1), flags=flags)


# ---------------------------------------------------------------------------------------
# 4. the lookups over it
# ---------------------------------------------------------------------------------------
def check_find(amq, torch, plan, filt, qb, queries, r, leaves, leaf_kb, with_ids):
    """find_keys behind probe_paths over r's paths (the hand-made ones among them): the candidates
    from the oracle's answers, the search from the leaves' dicts (tests/test_gpu_find.py)."""
    dicts, begin = leaf_dicts(leaves)
    ans = (r.path_opts if with_ids else r.path_plain)[0]
    cand_begin, cand_leaf, cand_entry = compact(r.nq, r.path_query, r.path_entry, r.path_leaf, ans)
    n_cand = int(cand_begin[-1])
    n = plan.n_segs
    sc = np.minimum(r.path_leaf, n - 1)
    checked = (r.path_leaf < n) & (plan.segs["hash_count" if plan.kind == BLOOM else "tag_bits"][sc] != 0)
    if with_ids:
        checked &= plan.segs["src_page_id"][sc] == r.path_page_ids
    want = find_walk(dicts, queries, cand_begin, cand_leaf, n_cand, False, checked[cand_entry])
    d_pid = ids(torch, r.path_page_ids) if with_ids else None
    res = amq.probe_paths(plan, filt, qb, dev(torch, r.path_begin.astype(np.int32)), dev(torch, r.path_leaf.astype(np.int32)),
                          want_entries=True, query_page_ids=d_pid)
    assert res.total() == n_cand
    pm, fc = amq.ProbeMetrics(), amq.FindCounts()
    found = amq.find_keys(plan, filt, qb, res, leaf_kb, key_begin=begin.astype(np.uint64), want_state=True,
                          query_page_ids=d_pid, metrics=pm, counts=fc)
    torch.cuda.synchronize()
    ki, lf, cand = (x.cpu().numpy().astype(np.int64) for x in (found.key_index, found.leaf, found.cand))
    assert np.array_equal(ki, want["key_index"]) and np.array_equal(lf, want["leaf"]) and np.array_equal(cand, want["cand"])
    assert np.array_equal(found.state.cpu().numpy()[:n_cand], want["state"])
    assert fc.collect() == want["counts"]
    assert pm.collect() == {**dict.fromkeys(abi.PROBE_METRICS_FIELDS, 0), "filter_false_positive_count": want["fp"]}
    return want


def device_world(amq, torch, w, plan, filt):
    """The host world with the opened plan, the device's filter bytes and the leaves' keys."""
    dw = copy.copy(w)
    dw.plan, dw.filt = plan, filt
    dw.leaf_kb = fixed_batch(amq, torch, [key for lv in w.leaves for key in lv], 16)
    return dw


def query_batch(amq, torch, shape, queries):
    return var_batch(amq, torch, queries) if shape == "var" else fixed_batch(amq, torch, queries, len(queries[0]))


def check_get(amq, torch, dw, tree, qb, want, check_ids):
    """get_keys through the raw launch into guarded buffers, key_begin given (an opened segment's
    own is 0), and through the wrapper."""
    bufs = buffers(torch, qb.n)
    launch(amq, dw, tree, qb, bufs, check_ids=check_ids, key_begin=dev(torch, dw.begin))
    get_same(read(amq, torch, bufs), want)
    pm, gc = amq.ProbeMetrics(), amq.GetCounts()
    r = amq.get_keys(dw.plan, dw.filt, tree, qb, dw.leaf_kb, key_begin=dw.begin.astype(np.uint64),
                     check_page_ids=check_ids, want_visits=True, metrics=pm, counts=gc)
    assert np.array_equal(r.key_index.cpu().numpy().view(np.uint64), want["key_index"])
    assert np.array_equal(r.leaf.cpu().numpy().view(np.uint32), want["leaf"])
    assert np.array_equal(r.visits.cpu().numpy(), want["visits"])
    assert pm.collect() == want["metrics"] and gc.collect() == want["counts"]


@gpu
@pytest.mark.parametrize("name", ["built", "synth"])
def test_bloom_find_keys_behind_the_paths(oracle, amq, torch, name):
    m, c = bloom_mixed(oracle, amq), bloom_q16(oracle, amq)
    d = opened_on_device(amq, torch, m, "bloom", BLOOM, REFUSED)
    plan, filt = d.opened.plan, getattr(d, name)
    r = c.r if name == "synth" else built_routes(oracle, amq)
    qb, queries = amq.KeyBatch.fixed(dev(torch, c.q)), [row.tobytes() for row in c.q]
    leaf_kb = fixed_batch(amq, torch, m.members, 16)
    for with_ids in (False, True):
        want = check_find(amq, torch, plan, filt, qb, queries, r, m.leaves, leaf_kb, with_ids)
        assert want["counts"]["found_count"] > 100 and want["counts"]["absent_count"] > 100
        assert want["counts"]["unsearchable_count"] > 0 and (want["fp"] > 100 or name == "built")
    if name == "synth":                                    # (the other shapes' tables are over this copy)
        for shape in ("k40", "var"):
            s = bloom_shape(oracle, amq, shape)
            keys, sqb = [bytes(key) for key in s.keys], batch(amq, torch, shape, s.keys)
            for with_ids in (False, True):
                want = check_find(amq, torch, plan, filt, sqb, keys, s.r, m.leaves, leaf_kb, with_ids)
                assert want["counts"]["absent_count"] > 100 and want["counts"]["found_count"] == 0


def built_routes(oracle, amq):
    """The 16-byte routes against the copy as built: the same pairs and paths, the other table."""
    if "built_routes" not in _b:
        m, c = bloom_mixed(oracle, amq), bloom_q16(oracle, amq)
        rng = np.random.default_rng()
        rng.bit_generator.state = c.state
        r = make_routes(rng, m.plan, table16(oracle, m.plan, m.built, c.q), c.r.seg, weighted_draw(rng, m.weights),
                        long_at=123, fixed_paths=c.hand)
        assert np.array_equal(r.path_leaf, c.r.path_leaf) and np.array_equal(r.path_page_ids, c.r.path_page_ids)
        _b["built_routes"] = r
    return _b["built_routes"]


@gpu
@pytest.mark.parametrize("shape", ["k16", "k40", "var"])
@pytest.mark.parametrize("name", ["built", "synth"])
def test_bloom_get_keys_over_the_tree(oracle, amq, torch, name, shape):
    m, t = bloom_mixed(oracle, amq), bloom_tree(oracle, amq)
    d = opened_on_device(amq, torch, m, "bloom", BLOOM, REFUSED)
    dw = device_world(amq, torch, t.worlds[name], d.opened.plan, getattr(d, name))
    qb = query_batch(amq, torch, shape, t.queries[shape])
    for check_ids in (False, True):
        check_get(amq, torch, dw, t.tree, qb, tree_want(t, name, shape, check_ids), check_ids)


def check_second_tile(amq, torch, dw, w, tree, base, check_ids):
    """One tile more than one round of the bounded grid: the first workgroup takes a second tile."""
    grid, threads = launch_cap()
    nq = grid * threads + threads - 3
    one = model_batch(w, tree, base, check_ids)
    pick = np.random.default_rng(9).integers(0, len(base), nq)
    got = read_launch(amq, torch, dw, tree, amq.KeyBatch.fixed(dev(torch, rows16(base)[pick])), check_ids)
    for field in ("key_index", "leaf", "where", "visits"):
        assert np.array_equal(got[field].astype(np.int64), one[field].astype(np.int64)[pick]), field
    per = np.bincount(pick, minlength=len(base))
    for names, field in ((METRICS, "metrics"), (COUNTS, "counts")):
        each = [model_batch(w, tree, [q], check_ids)[field] for q in base]
        assert dict(zip(names, (int(v) for v in got[field]))) == \
            {n: sum(int(c) * e[n] for c, e in zip(per, each)) for n in names}, field


def read_launch(amq, torch, dw, tree, qb, check_ids):
    bufs = buffers(torch, qb.n)
    launch(amq, dw, tree, qb, bufs, check_ids=check_ids, key_begin=dev(torch, dw.begin))
    return read(amq, torch, bufs)


@gpu
def test_bloom_get_keys_second_tile(oracle, amq, torch):
    m, t = bloom_mixed(oracle, amq), bloom_tree(oracle, amq)
    d = opened_on_device(amq, torch, m, "bloom", BLOOM, REFUSED)
    dw = device_world(amq, torch, t.worlds["synth"], d.opened.plan, d.synth)
    check_second_tile(amq, torch, dw, t.worlds["synth"], t.tree, t.queries["k16"], True)


# ---------------------------------------------------------------------------------------
# 5. VQF: the same skeleton, smaller
# ---------------------------------------------------------------------------------------
# (bits/key, payload capacity, keys): 8-bit tags; 16-bit tags; a capacity so small that hashes are
# truncated (hash_val_shift > 0, as tests/test_gpu_verify.py does it); two blocks of each width
VQF_SETTINGS = [(12, 32704, 900), (22, 65472, 700), (12, 80 + 64 * 16, 1000), (12, 208, 50), (22, 208, 25)]
V_WIDE, V_WIDE16, V_TRUNC, V_TWO, V_TWO16, V_REFUSED = range(6)
N_V = 6
PLACE_V = [3, 1, 5, 4, 0, 2]
GAPS_V = [16, 32, 16, 0, 48, 16]
NQ_V, N_MEMBER_V = 6000, 2500
HAND_V = {"widths": [V_WIDE, V_WIDE16, V_TWO, V_TWO16, V_TRUNC, V_WIDE16, V_WIDE],
          "holes": [V_TWO16, V_REFUSED, N_V + 2, V_TRUNC, V_WIDE16, V_TWO],
          "alternating": [V_TRUNC, V_TWO16] * 17}
_v = {}


def vqf_mixed(oracle, amq):
    if "m" in _v:
        return _v["m"]
    m, rng = Routes(), np.random.default_rng(20261022)
    # the truncated filter and the two two-block ones cover the universe (the tree's child leaves), the
    # wide ones and the refused slot's leaf hold samples of it
    n_child = [VQF_SETTINGS[s][2] for s in (V_TRUNC, V_TWO, V_TWO16)]
    m.cuts = np.concatenate([[0], 2 * np.cumsum(n_child)])
    m.U = U = rand_keys(rng, int(m.cuts[-1]) + 40)[:int(m.cuts[-1])]
    sample = lambda n: sorted({U[int(x)] for x in rng.integers(0, len(U), n)})
    child = [U[a:b][::2] for a, b in zip(m.cuts, m.cuts[1:])]
    m.leaves = [sample(VQF_SETTINGS[V_WIDE][2]), sample(VQF_SETTINGS[V_WIDE16][2])] + child + [sample(120)]
    m.segs_of, m.built_p = [], []
    for s in range(N_V):
        if s == V_REFUSED:
            sg, ref = None, None
        else:
            bpk, cap, _ = VQF_SETTINGS[s]
            sg, ref = one_filter(oracle, amq, VQF, m.leaves[s], bpk, cap, SRC0 + s)
        m.segs_of.append(sg)
        m.built_p.append(ref)
    m.built, m.plan = lay_out(amq, VQF, m.segs_of, m.built_p, PLACE_V, GAPS_V)
    m.offsets = m.plan.segs["out_offset"].copy()
    m.members = [key for lv in m.leaves for key in lv]
    own = np.repeat(np.arange(N_V), [len(lv) for lv in m.leaves])
    # the batch: member keys (half of them ask their own leaf), then random ones
    c = Routes()
    pick = rng.integers(0, len(m.members), N_MEMBER_V)
    c.q = np.concatenate([rows16(m.members)[pick], rng.integers(0, 256, (NQ_V - N_MEMBER_V, 16), dtype=np.uint8)])
    c.table = table16(oracle, m.plan, m.built, c.q)
    draw = weighted_draw(rng, [4, 4, 4, 4, 4, 1, 1])
    seg = draw(NQ_V)
    seg[:N_MEMBER_V:2] = own[pick][::2]
    seg[NQ_V // 3], seg[NQ_V // 2] = N_V, N_V + 5
    c.hand = hand_paths(HAND_V, 1000, 600)
    c.r = make_routes(rng, m.plan, c.table, seg, draw, long_at=123, fixed_paths=c.hand)
    m.c = c
    m.verify = verify_case(oracle, m.plan, m.built, m.leaves, 3000, 77400)
    # the tree: the wide filters, the refused slot and an outside leaf in the root's level, the others below
    lo, hi = bytes(16), b"\xff" * 16
    kids = [{"pivot_keys": [lo, U[int(m.cuts[1])], U[int(m.cuts[2])]], "page_id": 91, "levels": [],
             "children": [tree_leaf(V_TRUNC), tree_leaf(V_TWO)]},
            {"pivot_keys": [U[int(m.cuts[2])], hi], "children": [tree_leaf(V_TWO16)], "page_id": 92,
             "levels": [[tree_seg(V_TWO, 0b1)]]}]
    root = {"pivot_keys": [lo, U[int(m.cuts[2])], hi], "children": kids,
            "levels": [[tree_seg(V_WIDE, flushed={0: 300}), tree_seg(V_WIDE16), tree_seg(V_REFUSED),
                        {"leaf": OUTSIDE, "page_id": 5, "active": 0b11, "flushed": {}}]]}
    m.tree = amq.TreeIndex.from_description(root)
    m.tree.segments["leaf_page_id"][1] = 4242
    m.queries = [U[int(x)] for x in rng.integers(0, len(U), 400)] + \
        [bytes(r) for r in rng.integers(0, 256, (200, 16), dtype=np.uint8)]
    m.world = World.over(oracle, m.plan, m.leaves, m.built_p)
    m.want = {ci: model_batch(m.world, m.tree, m.queries, ci) for ci in (False, True)}
    _v["m"] = m
    return m


def test_vqf_array_inputs(oracle, amq):
    m = vqf_mixed(oracle, amq)
    segs, c = m.plan.segs, m.c
    assert list(segs["tag_bits"]) == [8, 16, 8, 8, 16, 0]
    assert list(segs["n_blocks"][[V_TWO, V_TWO16]]) == [2, 2] and int(segs["n_blocks"][V_TRUNC]) == 16
    assert list(segs["hash_val_shift"] > 0) == [False, False, True, False, False, False]
    # an opened segment's n_keys is the header's nelts: the plan's count, less what the truncation dropped
    counts = np.array([len(lv) for lv in m.leaves])
    whole = [V_WIDE, V_WIDE16, V_TWO, V_TWO16]
    assert np.array_equal(segs["n_keys"][whole], counts[whole]) and 0 < segs["n_keys"][V_TRUNC] < counts[V_TRUNC]
    assert not segs[V_REFUSED].tobytes()[8:].strip(b"\0")
    offs = m.offsets.astype(np.int64)
    assert list(np.argsort(offs)) == PLACE_V and len({int(o) % 64 for o in offs}) >= 3 and not (offs % 16).any()
    assert not m.built[offs[V_REFUSED]:offs[V_REFUSED] + 96].any()
    # oracle.vqf_is_present per key: the table's columns; members pass
    for s in range(N_V - 1):
        hashes = [oracle.xxh64(row.tobytes(), VQF_SEED) for row in c.q[:1500]]
        per_key = np.array([oracle.vqf_is_present(m.built_p[s], h) for h in hashes], np.uint8)
        assert np.array_equal(per_key, c.table[:1500, s])
        lv = m.leaves[s]
        st, res = oracle.probe_segments(VQF, m.built, m.offsets, rows16(lv), np.full(len(lv), s, np.uint32))
        assert st == 0 and res.all()
    assert_routes_populated(c.r, m.plan)
    # every segment with a filter both passes and rejects pairs of every route
    for s in range(N_V - 1):
        assert 0 < c.r.ref[c.r.seg == s].sum() < (c.r.seg == s).sum()
    # the hand-made paths alternate tag widths and cross the truncated filter
    for name, path in HAND_V.items():
        widths = [int(segs["tag_bits"][x]) for x in path if x < N_V and segs["tag_bits"][x]]
        assert V_TRUNC in path and sum(a != b for a, b in zip(widths, widths[1:])) >= 3, name
    assert len(HAND_V["alternating"]) > 32
    v = m.verify
    assert (v.v_missing[:V_REFUSED] > 1000).all() and v.v_missing[V_REFUSED] == 0
    for kb, missing, first in v.overlap:
        assert missing.sum() > 1000
    for check_ids in (False, True):
        every = {**m.want[check_ids]["metrics"], **m.want[check_ids]["counts"]}
        assert every.pop("page_id_mismatch_count") > 0 or not check_ids
        assert all(x > 0 for x in every.values()), every


@gpu
def test_vqf_open_scan_and_probes(oracle, amq, torch):
    m = vqf_mixed(oracle, amq)
    d = opened_on_device(amq, torch, m, "vqf", VQF, V_REFUSED)
    plan, c = d.opened.plan, m.c
    got = check_scan(amq, VQF, plan, d.built, m.built, V_REFUSED)
    assert not got["bad_blocks"].any() and np.array_equal(got["occupied"], got["header_items"])
    qb = amq.KeyBatch.fixed(dev(torch, c.q))
    check_probe(amq, torch, plan, d.built, qb, c.r, prefixes=(1, 255, 256, 257))
    check_hashed(amq, torch, plan, d.built, qb, c.r)
    check_paths(amq, torch, plan, d.built, qb, c.r)
    v = m.verify
    vkb = amq.KeyBatch.fixed(dev(torch, v.keys))
    check_verify(amq, torch, plan, d.built, vkb, v, hints=("plan", 100, 1), flags=v.flags)
    for kb, missing, first in v.overlap:
        res, total = verify_run(amq, torch, plan, d.built, vkb, key_begin=kb, hint=100)
        assert_result(res, total, missing, first, flags=v.flags)


@gpu
def test_vqf_lookups(oracle, amq, torch):
    m = vqf_mixed(oracle, amq)
    d = opened_on_device(amq, torch, m, "vqf", VQF, V_REFUSED)
    plan, c = d.opened.plan, m.c
    leaf_kb = fixed_batch(amq, torch, m.members, 16)
    qb, queries = amq.KeyBatch.fixed(dev(torch, c.q)), [row.tobytes() for row in c.q]
    for with_ids in (False, True):
        want = check_find(amq, torch, plan, d.built, qb, queries, c.r, m.leaves, leaf_kb, with_ids)
        assert want["counts"]["found_count"] > 100 and want["counts"]["absent_count"] > 0
    dw = device_world(amq, torch, m.world, plan, d.built)
    tq = fixed_batch(amq, torch, m.queries, 16)
    for check_ids in (False, True):
        check_get(amq, torch, dw, m.tree, tq, m.want[check_ids], check_ids)
    check_second_tile(amq, torch, dw, m.world, m.tree, m.queries, True)
