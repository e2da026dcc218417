"""GPU: the tree walk (tkv_amq_walk_paths / walk_paths) -- every query descended from the root, its
pivot found by an upper bound over the node's interior keys, an entry for every segment active for
that pivot, level by level, then the child.

The expectation model is `model` below: `bytes` comparison is std::string_view order and
bisect_right over the interior keys is the pivot; it applies the clamps include/tkv_amq.h defines
for malformed trees.  The end-to-end cases take their filter answers from the CPU oracle, as
tests/test_gpu_path_probe.py does."""
import bisect
import ctypes
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CANARY = 0xEE
GUARD = 64          # canary elements in front of and behind every output
MAX_DEPTH = 16
LEAF_LEVEL = 0xFF
VQF_CAP = 32704


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
def model_one(t, q, n_nodes=None):
    """Query q's entries (leaf, page id, flushed bound, where) over the flat tree t (a TreeIndex)."""
    n_nodes = len(t.nodes) if n_nodes is None else n_nodes
    keys, out, ni = t.pivot_keys, [], 0
    for depth in range(MAX_DEPTH):
        if ni >= n_nodes:
            break
        nd = t.nodes[ni]
        pc = int(nd["pivot_count"])
        if pc == 0 or pc > 64:
            break
        first = int(nd["pivot_key_begin"]) + 1
        n = min(pc - 1, max(0, len(keys) - first))            # interior keys past the list do not exist
        p = bisect.bisect_right(keys[first:first + n], q) if n else 0
        ls, sb = [int(x) for x in nd["level_start"]], int(nd["seg_begin"])
        for lv in range(min(int(nd["level_count"]), 7)):
            b, e = min(sb + ls[lv], len(t.segments)), min(sb + ls[lv + 1], len(t.segments))
            for s in range(b, e):                             # (a decreasing level_start: empty)
                sg = t.segments[s]
                if int(sg["active_pivots"]) >> p & 1:
                    fp, bound = int(sg["flushed_pivots"]), 0
                    if fp >> p & 1:
                        at = int(sg["flushed_begin"]) + bin(fp & ((1 << p) - 1)).count("1")
                        bound = int(t.flushed_bounds[at]) if at < len(t.flushed_bounds) else 0
                    out.append((int(sg["leaf"]), int(sg["leaf_page_id"]), bound, depth << 8 | lv))
        c = int(nd["child_begin"]) + p
        if c >= len(t.children):
            break
        ch = t.children[c]
        if int(nd["height"]) <= 1:
            out.append((int(ch["index"]), int(ch["page_id"]), 0, depth << 8 | LEAF_LEVEL))
            break
        ni = int(ch["index"])
    return out


def model(t, queries, n_nodes=None):
    paths = [model_one(t, q, n_nodes) for q in queries]
    begin = np.zeros(len(queries) + 1, np.int64)
    np.cumsum([len(p) for p in paths], out=begin[1:])
    flat = [e for p in paths for e in p]
    cols = [np.array([e[j] for e in flat], dtype=np.uint64 if j == 1 else np.int64) for j in range(4)]
    return {"begin": begin, "leaf": cols[0], "page": cols[1], "flushed": cols[2], "where": cols[3], "paths": paths}


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


def guarded(torch, n, dtype):
    """n elements between two guards, all canary bytes; (whole buffer, the n elements)."""
    whole = torch.empty(n + 2 * GUARD, dtype=dtype, device="cuda")
    whole.view(torch.uint8).fill_(CANARY)
    return whole, whole[GUARD:GUARD + n]


def run(amq, torch, tree, qb, capacity, pk=None, page=True, flushed=True, where=True, needed=True, n_nodes=None):
    """The launch alone into guarded, canary-filled outputs; the guards and every element at or past
    min(total, capacity) must be untouched."""
    d_nodes, d_segs, d_kids, d_bounds, own_pk = tree.device()
    pk = own_pk if pk is None else pk
    n = qb.n
    outs = {"begin": guarded(torch, n + 1, torch.int32), "leaf": guarded(torch, capacity, torch.int32)}
    if page:
        outs["page"] = guarded(torch, capacity, torch.int64)
    if flushed:
        outs["flushed"] = guarded(torch, capacity, torch.int32)
    if where:
        outs["where"] = guarded(torch, capacity, torch.int16)
    if needed:
        outs["needed"] = guarded(torch, 1, torch.int64)
    ws = torch.empty(amq.walk_paths_workspace_bytes(n), dtype=torch.uint8, device="cuda")

    def inner(name):
        return outs[name][1] if name in outs else None

    amq.walk_paths_device(d_nodes, len(tree.nodes) if n_nodes is None else n_nodes, d_segs, len(tree.segments),
                          d_kids, len(tree.children), d_bounds, len(tree.flushed_bounds), pk.data, pk.offsets,
                          pk.stride, pk.n, qb.data, qb.offsets, qb.stride, n, inner("begin"), inner("leaf"),
                          capacity, ws, inner("page"), inner("flushed"), inner("where"), inner("needed"))
    torch.cuda.synchronize()
    got = {}
    for name, (whole, part) in outs.items():
        raw = whole.cpu().numpy()
        size = raw.itemsize
        b = raw.view(np.uint8)
        assert (b[:GUARD * size] == CANARY).all() and (b[len(b) - GUARD * size:] == CANARY).all(), name
        got[name] = raw[GUARD:len(raw) - GUARD]
    written = int(got["begin"][-1])
    assert 0 <= written <= capacity
    for name in ("leaf", "page", "flushed", "where"):
        if name in got:
            assert (got[name][written:].view(np.uint8) == CANARY).all(), name
    return got


def same(got, want, capacity):
    """got: run()'s arrays; want: model()'s.  begin is clamped to the capacity, needed is exact,
    entries below min(total, capacity) are the model's."""
    total = int(want["begin"][-1])
    w = min(total, capacity)
    assert np.array_equal(got["begin"].astype(np.int64), np.minimum(want["begin"], capacity))
    if "needed" in got:
        assert int(got["needed"][0]) == total
    assert np.array_equal(got["leaf"][:w].view(np.uint32).astype(np.int64), want["leaf"][:w])
    if "page" in got:
        assert np.array_equal(got["page"][:w].view(np.uint64), want["page"][:w])
    if "flushed" in got:
        assert np.array_equal(got["flushed"][:w].view(np.uint32).astype(np.int64), want["flushed"][:w])
    if "where" in got:
        assert np.array_equal(got["where"][:w].view(np.uint16).astype(np.int64), want["where"][:w])


def check(amq, torch, tree, queries, qb=None, pk=None, slack=5, n_nodes=None):
    want = model(tree, queries, n_nodes)
    qb = amq.KeyBatch.from_host(queries) if qb is None else qb
    capacity = int(want["begin"][-1]) + slack
    same(run(amq, torch, tree, qb, capacity, pk=pk, n_nodes=n_nodes), want, capacity)
    return want


# ---------------------------------------------------------------------------------------
# trees
# ---------------------------------------------------------------------------------------
def key16(i):
    return b"\x40" * 8 + int(i).to_bytes(8, "big")


def nudge(k, d):
    """The key one below / above k in its last byte."""
    return k[:-1] + bytes([(k[-1] + d) % 256])


def leaf(i):
    return {"leaf": i, "page_id": 7000 + i}


def rand_levels(rng, n_pivots, next_leaf, sizes=None):
    """Levels of segments with random bit sets over n_pivots pivots; every segment names a fresh leaf."""
    sizes = [int(rng.integers(0, 4)) for _ in range(int(rng.integers(0, 4)))] if sizes is None else sizes
    levels = []
    for size in sizes:
        level = []
        for _ in range(size):
            active = int(rng.integers(0, 1 << min(n_pivots, 62))) | (1 << int(rng.integers(0, n_pivots)))
            fl = {int(p): int(rng.integers(1, 1 << 20)) for p in range(n_pivots) if rng.random() < 0.4}
            level.append({"leaf": next_leaf[0], "page_id": 7000 + next_leaf[0], "active": active, "flushed": fl})
            next_leaf[0] += 1
        levels.append(level)
    return levels


def make_tree(rng, spec, n_leaves, root_sizes=(2, 0, 3)):
    """spec: an int (a height-1 node of that many leaves) or a list of specs.  Leaf i covers
    [key16(10 i), key16(10 (i + 1))); the segments' leaves are numbered from n_leaves."""
    next_leaf, at = [n_leaves], [0]

    def build(s, root=False):
        first = at[0]
        if isinstance(s, int):
            kids = [leaf(at[0] + j) for j in range(s)]
            starts = [at[0] + j for j in range(s)]
            at[0] += s
        else:
            kids, starts = [], []
            for c in s:
                starts.append(at[0])
                kids.append(build(c))
        node = {"pivot_keys": [key16(10 * x) for x in starts] + [key16(10 * at[0])], "children": kids,
                "page_id": 600 + first}
        node["levels"] = rand_levels(rng, len(kids), next_leaf, list(root_sizes) if root else None)
        return node

    root = build(spec, root=True)
    assert at[0] == n_leaves
    root["page_id"] = 0
    return root


UNEVEN = [[3, 1], [5], [1, 2, 1, 2]]       # heights 3, 2, 1; fan-outs 3 / 2, 1, 4 / 3, 1, 5, 1, 2, 1, 2


def uneven_tree(amq):
    rng = np.random.default_rng(11)
    return amq.TreeIndex.from_description(make_tree(rng, UNEVEN, 15))


def uneven_queries():
    """Every separator, one below and one above it, below and above everything, and keys in between."""
    qs = [b"\x00" * 16, b"\xff" * 16, b"\x40" * 8 + b"\xff" * 8]
    for i in range(16):
        k = key16(10 * i)
        qs += [k, nudge(k, -1) if i else k, nudge(k, 1), key16(10 * i + 5)]
    return qs


def clone(amq, t):
    return amq.TreeIndex(t.nodes.copy(), t.segments.copy(), t.children.copy(), t.flushed_bounds.copy(),
                         list(t.pivot_keys))


# ---------------------------------------------------------------------------------------
# 1. pivot search edges
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("pivot_count", [1, 2, 3, 63, 64])
def test_pivot_search_edges(amq, torch, pivot_count):
    interior = [key16(4 * j + 2) for j in range(1, pivot_count)]
    # k0 above and kp below every query: either of them, read as a search key, changes the answer
    node = {"pivot_keys": [b"\xff" * 16] + interior + [b"\x00" * 16],
            "children": [leaf(100 + i) for i in range(pivot_count)], "levels": []}
    tree = amq.TreeIndex.from_description(node)
    qs = [b"\x00" * 16, b"\xff" * 16, key16(0), key16(4 * 70)]
    for k in interior:
        qs += [k, nudge(k, -1), nudge(k, 1)]
    want = check(amq, torch, tree, qs)
    # one entry per query, the child of its pivot: a query equal to an interior key goes right
    assert np.array_equal(want["begin"], np.arange(len(qs) + 1))
    pivots = want["leaf"] - 100
    assert np.array_equal(pivots, [bisect.bisect_right(interior, q) for q in qs])
    assert pivots[0] == 0 and pivots[1] == pivot_count - 1
    for j, k in enumerate(interior):
        assert list(pivots[4 + 3 * j:7 + 3 * j]) == [j + 1, j, j + 1]
    assert (want["where"] == LEAF_LEVEL).all() and (want["flushed"] == 0).all()


# ---------------------------------------------------------------------------------------
# 2. key shapes
# ---------------------------------------------------------------------------------------
def hand_keys(length):
    """Keys that differ only in one byte at a word edge, by 0x00 / 0x7f / 0x80 / 0xff there: a
    little-endian or a signed compare orders them wrongly."""
    base = bytes([0x40] * length)
    keys = {base}
    for p in sorted({0, 7, 8, 15, length - 8, length - 1}):
        for v in (0x00, 0x7F, 0x80, 0xFF):
            keys.add(base[:p] + bytes([v]) + base[p + 1:])
    return sorted(keys)


def shape_case(length):
    interior = hand_keys(length)
    n = len(interior) + 1
    rng = np.random.default_rng(length)
    node = {"pivot_keys": [b"\xee" * length] + interior + [b"\x11" * length],
            "children": [leaf(200 + i) for i in range(n)],
            "levels": rand_levels(rng, n, [300], [2, 1])}
    qs = [b"\x00" * length, b"\xff" * length]
    for k in interior:
        qs += [k, nudge(k, -1), nudge(k, 1), k[:-9] + bytes([(k[-9] + 1) % 256]) + k[-8:]]
    return node, qs


SHAPES = ["k16", "k24", "k16_off8", "k24_off4", "k20", "offs_pivots", "offs_queries"]


@pytest.mark.parametrize("shape", SHAPES)
def test_key_shapes(amq, torch, shape):
    length = {"k16": 16, "k16_off8": 16, "k24": 24, "k24_off4": 24, "k20": 20}.get(shape, 16)
    node, qs = shape_case(length)
    tree = amq.TreeIndex.from_description(node)
    # the fast modes need both sides aligned; a pointer off by 8 (16-byte keys) or 4 (24) on either
    # side, another stride, or offsets on either side take the general compare
    pk_shift, q_shift = {"k16_off8": (8, 0), "k24_off4": (0, 4)}.get(shape, (0, 0))
    pk = var_batch(amq, torch, tree.pivot_keys) if shape == "offs_pivots" else \
        fixed_batch(amq, torch, tree.pivot_keys, length, pk_shift)
    qb = var_batch(amq, torch, qs) if shape == "offs_queries" else fixed_batch(amq, torch, qs, length, q_shift)
    want = check(amq, torch, tree, qs, qb=qb, pk=pk)
    child = np.array([p[-1][0] - 200 for p in want["paths"]])
    assert np.array_equal(child, [bisect.bisect_right(tree.pivot_keys[1:-1], q) for q in qs])


def test_variable_length_keys_and_prefixes(amq, torch):
    interior = sorted([b"a", b"ab", b"ab\x00", b"abc", b"abcdefgh", b"abcdefghi", b"abcdefghijkl", b"abcdefghijklm",
                       b"b" * 8, b"b" * 12, b"b" * 13, b"b" * 31, b"b" * 32, b"b" * 40, b"c\xff", b"c\xff\x00"])
    n = len(interior) + 1
    node = {"pivot_keys": [b"zzzz"] + interior + [b"\x00"], "children": [leaf(400 + i) for i in range(n)],
            "levels": rand_levels(np.random.default_rng(3), n, [500], [1, 2])}
    tree = amq.TreeIndex.from_description(node)
    # a query equal to the shorter of two keys of which one is a prefix of the other stays left of
    # the longer; one byte more or less moves it across
    qs = list(interior) + [k + b"\x00" for k in interior] + [k[:-1] for k in interior if len(k) > 1]
    qs += [b"\x00", b"\xff" * 40, b"b" * 33, b"abcdefgh\x00", b"abcdefgg\xff\xff\xff\xff\xff"]
    want = check(amq, torch, tree, qs, qb=var_batch(amq, torch, qs), pk=var_batch(amq, torch, tree.pivot_keys))
    child = np.array([p[-1][0] - 400 for p in want["paths"]])
    assert np.array_equal(child, [bisect.bisect_right(interior, q) for q in qs])
    assert child[interior.index(b"ab")] == interior.index(b"ab") + 1     # "ab" < "ab\0": right of "ab" only
    # fixed 1-byte queries against the offsets-form pivots
    ones = [bytes([b]) for b in (0, 0x61, 0x62, 0x63, 0xff)]
    check(amq, torch, tree, ones, qb=fixed_batch(amq, torch, ones, 1), pk=var_batch(amq, torch, tree.pivot_keys))


# ---------------------------------------------------------------------------------------
# 3. levels and bit sets
# ---------------------------------------------------------------------------------------
def test_levels_and_bit_sets(amq, torch):
    rng = np.random.default_rng(21)
    b0, b5, b6, b63 = 1, 1 << 5, 1 << 6, 1 << 63

    def seg(i, active, flushed):
        return {"leaf": 900 + i, "page_id": (0xABCD << 32) + i, "active": active, "flushed": flushed}

    levels = [[seg(0, b0 | b5 | b63, {0: 11, 5: 55, 63: 63}),     # rank 0 (p 0), 1 (p 5), 2 (p 63)
               seg(1, b5, {3: 1, 7: 2}),                          # bits below and above 5, not at 5: bound 0
               seg(2, b5 | b6, {5: 99})],                         # three segments of one level active for p 5
              [],
              [seg(3, 0, {5: 1}),                                 # active for no pivot
               seg(4, (1 << 64) - 1, {1: 101, 5: 105, 9: 109})],  # rank mid
              [], [],
              [seg(5, b63, {63: 7})],
              [seg(6 + j, int(rng.integers(0, 1 << 63)) | b5, {int(p): int(p) + 1000 for p in rng.integers(0, 64, 9)})
               for j in range(4)]]
    interior = [key16(j) for j in range(1, 64)]
    node = {"pivot_keys": [b"\xff" * 16] + interior + [b"\x00" * 16], "children": [leaf(i) for i in range(64)],
            "levels": levels}
    tree = amq.TreeIndex.from_description(node)
    assert tree.nodes[0]["level_count"] == 7 and list(tree.nodes[0]["level_start"]) == [0, 3, 3, 5, 5, 5, 6, 10]
    qs = [key16(j) for j in range(64)]                            # query j has pivot j
    want = check(amq, torch, tree, qs)
    p5 = want["paths"][5]
    assert [e[0] for e in p5[:4]] == [900, 901, 902, 904] and [e[2] for e in p5[:4]] == [55, 0, 99, 105]
    assert [e[3] for e in p5[:4]] == [0, 0, 0, 2] and p5[-1] == (5, 7005, 0, LEAF_LEVEL)
    assert [e[1] for e in p5[:4]] == [(0xABCD << 32) + i for i in (0, 1, 2, 4)]
    assert want["paths"][0][0] == (900, 0xABCD << 32, 11, 0)
    p63 = want["paths"][63]
    assert p63[0][:3] == (900, 0xABCD << 32, 63) and (905, (0xABCD << 32) + 5, 7, 5) in p63
    assert all(e[0] != 903 for p in want["paths"] for e in p)
    # level_count 0: the child alone
    bare = amq.TreeIndex.from_description(dict(node, levels=[]))
    assert bare.nodes[0]["level_count"] == 0
    want = check(amq, torch, bare, qs)
    assert np.array_equal(want["leaf"], np.arange(64))


# ---------------------------------------------------------------------------------------
# 4. heights 1, 2 and 3; every optional output given and not given
# ---------------------------------------------------------------------------------------
def test_heights_and_optional_outputs(amq, torch):
    tree = uneven_tree(amq)
    assert sorted(set(int(h) for h in tree.nodes["height"])) == [1, 2, 3] and tree.nodes[0]["height"] == 3
    assert [int(n) for n in tree.nodes["pivot_count"]] == [3, 2, 1, 4, 3, 1, 5, 1, 2, 1, 2]
    qs = uneven_queries()
    want = model(tree, qs)
    assert {e[3] >> 8 for p in want["paths"] for e in p} == {0, 1, 2}
    assert all(p[-1][3] == (2 << 8 | LEAF_LEVEL) for p in want["paths"])
    qb = amq.KeyBatch.from_host(qs)
    cap = int(want["begin"][-1]) + 3
    full = run(amq, torch, tree, qb, cap)
    same(full, want, cap)
    bare = run(amq, torch, tree, qb, cap, page=False, flushed=False, where=False, needed=False)
    same(bare, want, cap)
    assert np.array_equal(bare["begin"], full["begin"]) and np.array_equal(bare["leaf"], full["leaf"])
    for only in ("page", "flushed", "where", "needed"):
        opts = {k: k == only for k in ("page", "flushed", "where", "needed")}
        one = run(amq, torch, tree, qb, cap, **opts)
        same(one, want, cap)
        assert np.array_equal(one["begin"], full["begin"]) and np.array_equal(one["leaf"], full["leaf"])
    # the convenience wrapper: capacity from a first run, every output
    res = amq.walk_paths(tree, qb, want_page_ids=True, want_flushed=True, want_where=True)
    assert res.capacity == int(want["begin"][-1]) == res.total() == int(res.needed.item())
    got = {"begin": res.path_begin.cpu().numpy(), "leaf": res.path_leaf.cpu().numpy(),
           "page": res.path_page_id.cpu().numpy(), "flushed": res.path_flushed.cpu().numpy(),
           "where": res.path_where.cpu().numpy(), "needed": res.needed.cpu().numpy()}
    same(got, want, res.capacity)


# ---------------------------------------------------------------------------------------
# 5. malformed trees
# ---------------------------------------------------------------------------------------
def malformed(amq, name):
    t = clone(amq, uneven_tree(amq))
    n_nodes, n_segs, n_pk, n_bounds = len(t.nodes), len(t.segments), len(t.pivot_keys), len(t.flushed_bounds)
    if name == "child_index_past_nodes":
        t.children["index"][int(t.nodes[0]["child_begin"]) + 1] = n_nodes + 5
    elif name == "child_begin_past_children":
        t.nodes["child_begin"][1] = len(t.children) - 1          # pivot 0 still has a slot, pivot 1 has none
    elif name == "key_begin_past_list":
        t.nodes["pivot_key_begin"][0] = n_pk + 3
    elif name == "key_begin_partly_past_list":
        t.nodes["pivot_key_begin"][3] = n_pk - 3                 # 2 of the 3 interior keys exist
    elif name == "level_start_decreasing":
        t.nodes["level_start"][0] = [0, 2, 1, 5, 5, 5, 5, 5]
    elif name == "seg_begin_past_segments":
        t.nodes["seg_begin"][0] = n_segs + 1
    elif name == "seg_begin_partly_past_segments":
        t.nodes["seg_begin"][0] = n_segs - 3
    elif name == "seg_begin_wraps":
        t.nodes["seg_begin"][0] = 0xFFFFFFFF
    elif name == "flushed_begin_past_bounds":
        t.segments["flushed_begin"][:3] = [n_bounds + 2, n_bounds - 1, 0xFFFFFFFF]
    elif name == "pivot_count_0":
        t.nodes["pivot_count"][1] = 0
    elif name == "pivot_count_65":
        t.nodes["pivot_count"][3] = 65
    elif name == "level_count_200":
        t.nodes["level_count"][0] = 200                          # read as 7, the levels level_start names
        t.nodes["level_start"][0] = [0, 2, 2, 5, 6, 7, 8, 9]
    elif name == "height_0":
        t.nodes["height"][1] = 0                                 # read as 1: its children are leaves
    else:
        raise AssertionError(name)
    return t


MALFORMED = ["child_index_past_nodes", "child_begin_past_children", "key_begin_past_list",
             "key_begin_partly_past_list", "level_start_decreasing", "seg_begin_past_segments",
             "seg_begin_partly_past_segments", "seg_begin_wraps", "flushed_begin_past_bounds", "pivot_count_0",
             "pivot_count_65", "level_count_200", "height_0"]


@pytest.mark.parametrize("name", MALFORMED)
def test_malformed_trees_answer_as_the_clamped_model(amq, torch, name):
    good = uneven_tree(amq)
    t = malformed(amq, name)
    qs = uneven_queries()
    want = check(amq, torch, t, qs)
    assert [len(p) for p in want["paths"]] != [len(p) for p in model(good, qs)["paths"]] or \
        not np.array_equal(want["flushed"], model(good, qs)["flushed"]) or \
        not np.array_equal(want["leaf"], model(good, qs)["leaf"]), "the damage must show"


def test_a_cycle_ends_after_max_depth_nodes(amq, torch):
    node = {"pivot_keys": [key16(0), key16(9)], "children": [leaf(1)],
            "levels": [[{"leaf": 77, "page_id": 78, "active": 1, "flushed": {0: 3}}]]}
    t = amq.TreeIndex.from_description(node)
    t.nodes["height"][0] = 2
    t.children["index"][0] = 0                                   # the node is its own child
    qs = [key16(j) for j in range(5)]
    want = check(amq, torch, t, qs)
    assert np.array_equal(want["begin"], MAX_DEPTH * np.arange(len(qs) + 1))
    assert list(want["where"][:MAX_DEPTH]) == [d << 8 for d in range(MAX_DEPTH)]
    # and no node at all: every path is empty
    want = check(amq, torch, t, qs, n_nodes=0)
    assert int(want["begin"][-1]) == 0


# ---------------------------------------------------------------------------------------
# 6. capacity
# ---------------------------------------------------------------------------------------
def test_capacity_and_empty_batch(amq, torch):
    tree = uneven_tree(amq)
    qs = uneven_queries()
    want = model(tree, qs)
    total = int(want["begin"][-1])
    qb = amq.KeyBatch.from_host(qs)
    for cap in (0, total - 1, total, total + 7, total // 2):
        got = run(amq, torch, tree, qb, cap)
        same(got, want, cap)
        assert int(got["begin"][-1]) == min(total, cap) and int(got["needed"][0]) == total
    # n_queries == 0: begin[0] = 0 and needed = 0, nothing else
    empty = amq.KeyBatch(qb.data[:0], 0, 16, None)
    got = run(amq, torch, tree, empty, 9)
    assert list(got["begin"]) == [0] and int(got["needed"][0]) == 0
    got = run(amq, torch, tree, empty, 0, page=False, flushed=False, where=False, needed=False)
    assert list(got["begin"]) == [0]


# ---------------------------------------------------------------------------------------
# 7. more queries than one round of the grid
# ---------------------------------------------------------------------------------------
def launch_cap():
    """kWalkMaxGrid workgroups of kWalkThreads lanes, read from the source."""
    from turtle_kv_amd import _build
    with open(os.path.join(_build.HERE, "csrc", "tkv_amq_walk.hip")) as f:
        src = f.read()
    grid = int(re.search(r"constexpr uint32_t kWalkMaxGrid = (\d+);", src).group(1))
    threads = int(re.search(r"constexpr uint32_t kWalkThreads = (\d+);", src).group(1))
    per = int(re.search(r"constexpr uint32_t kWalkScanPerThread = (\d+);", src).group(1))
    return grid, threads, per


def test_more_queries_than_one_grid_round(oracle, amq, torch):
    grid, threads, per = launch_cap()
    nq = grid * threads + 300                                    # every workgroup takes a second tile
    assert nq > threads * threads * per                          # and the totals' scan a second pass
    seg = [{"leaf": 50, "page_id": 51, "active": 0b011, "flushed": {1: 9}},
           {"leaf": 60, "page_id": 61, "active": 0b110, "flushed": {}}]
    q = oracle.gen_keys16(44, 0, nq)
    cut = [bytes([0x55]) + b"\x00" * 15, bytes([0xAA]) + b"\x00" * 15]
    node = {"pivot_keys": [b"\xff" * 16] + cut + [b"\x00" * 16], "children": [leaf(i) for i in range(3)],
            "levels": [seg]}
    tree = amq.TreeIndex.from_description(node)
    p = (q[:, 0] >= 0x55).astype(np.int64) + (q[:, 0] >= 0xAA)
    # the three pivots' paths, from the model; every query's path is its pivot's
    rows = model(tree, [b"\x00" * 16, b"\x60" + b"\x00" * 15, b"\xf0" + b"\x00" * 15])["paths"]
    assert [len(r) for r in rows] == [2, 3, 2] and set(np.unique(p)) == {0, 1, 2}
    table = np.array([e for r in rows for e in r], dtype=np.int64)
    off = np.array([0, 2, 5])
    lens = np.array([2, 3, 2])[p]
    begin = np.zeros(nq + 1, np.int64)
    np.cumsum(lens, out=begin[1:])
    idx = np.repeat(off[p], lens) + (np.arange(int(begin[-1])) - np.repeat(begin[:-1], lens))
    want = {"begin": begin, "leaf": table[idx, 0], "page": table[idx, 1].astype(np.uint64), "flushed": table[idx, 2],
            "where": table[idx, 3]}
    cap = int(begin[-1]) + 11
    same(run(amq, torch, tree, amq.KeyBatch.fixed(dev(torch, q)), cap), want, cap)
    short = int(begin[-1]) - 100000                              # clamped in the last tiles only
    same(run(amq, torch, tree, amq.KeyBatch.fixed(dev(torch, q)), short), want, short)


# ---------------------------------------------------------------------------------------
# 8. end to end: walk -> path probe -> leaf search
# ---------------------------------------------------------------------------------------
N_BOTTOM, N_UPPER, LEAF_KEYS = 24, 16, 2048
GROUPS = [5, 3, 7, 1, 8]                                          # bottom leaves per height-1 node


class Case:
    pass


_e2e = {}


def e2e_case(oracle, amq, torch, kind):
    """24 sorted bottom leaves under 5 nodes of height 1; 16 more leaves as segments on two levels
    of the root, holding copies of bottom keys (the same key in two or three places) and keys of
    their own.  Built once per kind and left unchanged."""
    if kind in _e2e:
        return _e2e[kind]
    c = Case()
    rng = np.random.default_rng(31 + kind)
    base = sorted(r.tobytes() for r in oracle.gen_keys16(42, 0, N_BOTTOM * 1500))
    cuts = sorted(rng.choice(np.arange(1, len(base)), N_BOTTOM - 1, replace=False))
    cuts = [0] + [int(x) for x in cuts] + [len(base)]
    while max(b - a for a, b in zip(cuts, cuts[1:])) > LEAF_KEYS:  # (no leaf above 2,048 keys)
        cuts = [0] + [len(base) * j // N_BOTTOM for j in range(1, N_BOTTOM)] + [len(base)]
    leaves = [base[a:b] for a, b in zip(cuts, cuts[1:])]
    sep = [b"\x00" * 16] + [lv[0] for lv in leaves[1:]] + [b"\xff" * 16]
    fresh = [r.tobytes() for r in oracle.gen_keys16(45, 0, N_UPPER * 300)]
    node_first = np.concatenate([[0], np.cumsum(GROUPS)])
    root_keys = [sep[int(f)] for f in node_first]
    upper = []
    for j in range(N_UPPER):
        lo, hi = sorted(int(x) for x in rng.choice(len(base), 2, replace=False))
        own = [k for k in fresh[300 * j:300 * (j + 1)] if base[lo] <= k < base[hi]]
        copies = [base[int(x)] for x in rng.integers(lo, hi, 600)] if hi > lo else []
        if j >= 8:                                                # level 1 repeats keys of level 0
            copies += upper[j - 8][::5]
        upper.append(sorted(set(own + copies)))
    leaves += upper
    c.leaves = leaves
    c.counts = [len(lv) for lv in leaves]
    assert len(leaves) == 40 and max(c.counts) <= LEAF_KEYS
    c.dicts, g = [], 0
    for lv in leaves:
        c.dicts.append({k: g + i for i, k in enumerate(lv)})
        g += len(lv)
    c.src = np.arange(3000, 3000 + len(leaves), dtype=np.uint64)

    def upper_seg(j):
        ks = upper[j]
        active = 0
        for k in ks:
            active |= 1 << (bisect.bisect_right(root_keys[1:-1], k))
        return {"leaf": N_BOTTOM + j, "page_id": int(c.src[N_BOTTOM + j]), "active": active, "flushed": {}}

    kids = []
    for n, (f, e) in enumerate(zip(node_first, node_first[1:])):
        kids.append({"pivot_keys": sep[int(f):int(e) + 1], "page_id": 100 + n, "levels": [],
                     "children": [{"leaf": i, "page_id": int(c.src[i])} for i in range(int(f), int(e))]})
    root = {"pivot_keys": root_keys, "children": kids,
            "levels": [[upper_seg(j) for j in range(8)], [upper_seg(j) for j in range(8, 16)]]}
    c.tree = amq.TreeIndex.from_description(root)
    c.wrong = 3                                                   # one segment with a wrong page id
    c.tree.segments["leaf_page_id"][c.wrong] = 99999
    keys = np.frombuffer(b"".join(k for lv in leaves for k in lv), np.uint8).reshape(-1, 16).copy()
    c.plan = amq.plan_filters(kind, c.counts, 12 if kind else 10, payload_capacity=VQF_CAP if kind else 0,
                              src_page_ids=c.src)
    c.leaf_keys = amq.KeyBatch.fixed(dev(torch, keys))
    c.filt = amq.build_all_filters(c.plan, c.leaf_keys)
    c.filt_np = c.filt.cpu().numpy()
    c.keys = keys
    _e2e[kind] = c
    return c


def e2e_queries(oracle, c, seed, n_hit=1500, n_miss=1500):
    rng = np.random.default_rng(seed)
    hit = c.keys[rng.integers(0, len(c.keys), n_hit)]
    return np.concatenate([hit, oracle.gen_keys16(46 + seed, 0, n_miss)])


def chain(amq, torch, c, q_dev, nq, capacity, bufs=None, stream=None):
    """walk -> path probe (n_entries = the capacity, the walk's page ids) -> leaf search, on raw
    buffers: three calls, nothing read back in between."""
    L = amq.abi.lib()
    plan = c.plan
    if bufs is None:
        bufs = {"begin": guarded(torch, nq + 1, torch.int32), "leaf": guarded(torch, capacity, torch.int32),
                "page": guarded(torch, capacity, torch.int64), "needed": guarded(torch, 1, torch.int64),
                "answer": guarded(torch, capacity, torch.uint8), "cbegin": guarded(torch, nq + 1, torch.int32),
                "cleaf": guarded(torch, capacity, torch.int32), "centry": guarded(torch, capacity, torch.int32),
                "result": (None, torch.full((16 * nq,), CANARY, dtype=torch.uint8, device="cuda")),
                "ws_walk": (None, torch.empty(amq.walk_paths_workspace_bytes(nq), dtype=torch.uint8, device="cuda")),
                "ws_probe": (None, torch.empty(amq.path_probe_workspace_bytes(nq, capacity), dtype=torch.uint8,
                                               device="cuda"))}
    b = {k: v[1] for k, v in bufs.items()}
    d_nodes, d_segs, d_kids, d_bounds, pk = c.tree.device()
    sh = ctypes.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
    amq.walk_paths_device(d_nodes, len(c.tree.nodes), d_segs, len(c.tree.segments), d_kids, len(c.tree.children),
                          d_bounds, len(c.tree.flushed_bounds), pk.data, pk.offsets, pk.stride, pk.n, q_dev, None, 16,
                          nq, b["begin"], b["leaf"], capacity, b["ws_walk"], b["page"], None, None, b["needed"],
                          stream)
    opts = amq.abi.ProbeOpts(b["page"].data_ptr(), None, None)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = L.tkv_amq_path_probe(plan.kind, p(c.filt), p(plan.device_segs()), plan.n_segs, p(q_dev), None, 16, nq,
                              p(b["begin"]), p(b["leaf"]), capacity, p(b["answer"]), p(b["cbegin"]), p(b["cleaf"]),
                              p(b["centry"]), ctypes.byref(opts), p(b["ws_probe"]), int(b["ws_probe"].numel()), sh)
    assert st == 0
    amq.find_keys_device(plan.kind, c.filt, plan.device_segs(), plan.n_segs, q_dev, None, 16, nq, b["cbegin"],
                         b["cleaf"], b["centry"], capacity, c.leaf_keys.data, None, 16, c.leaf_keys.n, None,
                         b["result"], d_query_page_ids=b["page"], stream=stream)
    return bufs


def read(amq, torch, bufs, nq):
    torch.cuda.synchronize()
    out = {}
    for name, (whole, part) in bufs.items():
        if whole is not None:
            raw = whole.cpu().numpy()
            bts = raw.view(np.uint8)
            g = GUARD * raw.itemsize
            assert (bts[:g] == CANARY).all() and (bts[len(bts) - g:] == CANARY).all(), name
            out[name] = raw[GUARD:len(raw) - GUARD]
    rec = bufs["result"][1].cpu().numpy().view(amq.abi.FIND_RESULT_DTYPE)
    out["key_index"] = rec["key_index"].view(np.int64).copy()
    out["found_leaf"] = rec["leaf"].view(np.int32).astype(np.int64)
    return out


def e2e_expect(oracle, c, q):
    """Paths from the model; every entry's answer from the CPU oracle (a page-id mismatch or a leaf
    outside the plan cannot reject); the newest leaf that holds each key."""
    qs = [r.tobytes() for r in q]
    want = model(c.tree, qs)
    n_ent = int(want["begin"][-1])
    pair_query = np.repeat(np.arange(len(qs)), np.diff(want["begin"]))
    leaf_of = want["leaf"]
    inplan = leaf_of < c.plan.n_segs
    src = np.zeros(n_ent, np.uint64)
    src[inplan] = c.plan.segs["src_page_id"][leaf_of[inplan]]
    checked = inplan & (src == want["page"])
    st, ref = oracle.probe_segments(c.plan.kind, c.filt_np, c.plan.segs["out_offset"],
                                    np.ascontiguousarray(q[pair_query]), np.where(inplan, leaf_of, 0).astype(np.uint32))
    assert st == 0
    want["answer"] = np.where(checked, ref, 1).astype(np.uint8)
    want["ref"], want["checked"] = ref, checked
    newest = np.full(len(qs), -1, np.int64)
    index = np.full(len(qs), -1, np.int64)
    for i, (k, path) in enumerate(zip(qs, want["paths"])):
        for e in path:
            if k in c.dicts[e[0]]:
                newest[i], index[i] = e[0], c.dicts[e[0]][k]
                break
    want["newest"], want["index"] = newest, index
    return want


def same_chain(got, want, capacity):
    total = int(want["begin"][-1])
    assert total <= capacity and int(got["needed"][0]) == total
    assert np.array_equal(got["begin"].astype(np.int64), want["begin"])
    assert np.array_equal(got["leaf"][:total].astype(np.int64), want["leaf"])
    assert np.array_equal(got["page"][:total].view(np.uint64), want["page"])
    assert np.array_equal(got["answer"][:total], want["answer"])
    keep = want["answer"] == 1
    n_cand = int(keep.sum())
    cb = np.zeros(len(want["begin"]), np.int64)
    np.cumsum(np.bincount(np.repeat(np.arange(len(cb) - 1), np.diff(want["begin"]))[keep], minlength=len(cb) - 1),
              out=cb[1:])
    assert np.array_equal(got["cbegin"].astype(np.int64), cb)
    assert np.array_equal(got["cleaf"][:n_cand].astype(np.int64), want["leaf"][keep])
    assert np.array_equal(got["centry"][:n_cand].astype(np.int64), np.flatnonzero(keep))
    # n_entries is the capacity: nothing past the totals is touched
    assert (got["answer"][total:] == CANARY).all()
    for name in ("leaf", "page"):
        assert (got[name][total:].view(np.uint8) == CANARY).all(), name
    for name in ("cleaf", "centry"):
        assert (got[name][n_cand:].view(np.uint8) == CANARY).all(), name
    assert np.array_equal(got["found_leaf"], want["newest"])
    assert np.array_equal(got["key_index"], want["index"])


@pytest.mark.parametrize("kind", [0, 1])
def test_end_to_end(oracle, amq, torch, kind):
    c = e2e_case(oracle, amq, torch, kind)
    q = e2e_queries(oracle, c, 1)
    want = e2e_expect(oracle, c, q)
    total = int(want["begin"][-1])
    # every present key is found, in its newest leaf at its own index; some keys live in two levels
    assert (want["newest"][:1500] >= 0).all() and (want["newest"][1500:] == -1).all()
    places = [sum(r.tobytes() in d for d in c.dicts) for r in q[:1500]]
    assert max(places) >= 3 and places.count(2) > 100
    assert (want["newest"][:1500] >= N_BOTTOM).sum() > 100 and (want["newest"][:1500] < N_BOTTOM).sum() > 100
    # the wrong page id: entries of that segment cannot reject, whatever the filter says
    wrong = want["leaf"] == int(c.tree.segments["leaf"][c.wrong])
    assert wrong.any() and not want["checked"][wrong].any() and (want["answer"][wrong] == 1).all()
    assert (want["ref"][wrong] == 0).any(), "some of them the filter alone would have rejected"
    assert want["checked"][~wrong].all()
    capacity = total + 37
    bufs = chain(amq, torch, c, dev(torch, q), len(q), capacity)
    same_chain(read(amq, torch, bufs, len(q)), want, capacity)


# ---------------------------------------------------------------------------------------
# 9. the three calls in one captured graph
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1])
def test_chain_replays_in_a_graph(oracle, amq, torch, kind):
    c = e2e_case(oracle, amq, torch, kind)
    batches = [e2e_queries(oracle, c, seed) for seed in (1, 2, 3)]
    nq = len(batches[0])
    wants = [e2e_expect(oracle, c, q) for q in batches]
    capacity = max(int(w["begin"][-1]) for w in wants) + 50
    eager = []
    for q in batches[1:]:
        eager.append(read(amq, torch, chain(amq, torch, c, dev(torch, q), nq, capacity), nq))
    q_dev = dev(torch, batches[0])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                    # warm-up on the capture stream
        bufs = chain(amq, torch, c, q_dev, nq, capacity, stream=s)
    s.synchronize()
    c.plan.device_segs()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        chain(amq, torch, c, q_dev, nq, capacity, bufs=bufs, stream=s)
    for q, want, e in zip(batches[1:], wants[1:], eager):
        q_dev.copy_(torch.from_numpy(q))                          # different queries, in place
        for name, (whole, part) in bufs.items():                  # (fresh canaries for this replay)
            if whole is not None:
                whole.view(torch.uint8).fill_(CANARY)
        torch.cuda.synchronize()
        graph.replay()
        got = read(amq, torch, bufs, nq)
        same_chain(got, want, capacity)
        total = int(want["begin"][-1])
        for name in ("begin", "cbegin", "key_index", "found_leaf", "needed"):
            assert np.array_equal(got[name], e[name]), name
        for name in ("leaf", "page", "answer"):
            assert np.array_equal(got[name][:total], e[name][:total]), name
