"""GPU: the point lookup with values (tkv_amq_get_values / get_values, tkv_amq_gather_values) --
tkv_amq_get_keys' descent with the value rule of the reference's find_key: each found item's packed
value (an op byte, then the data) is folded into the lookup's value, and the lookup goes on through
the older levels and the child while an ADD_I32 is pending.

The expectation is `model_value` below: tests/test_gpu_get.py's `model_get` with the fold of
include/tkv_amq.h (`Fold`, `as_i32`, `unpack`, restated from the rule, not from the reference's
code) in place of its "found" branch, over a host copy of the value array read with the clamps the
header defines (`Values.get`).  The fold itself is held to a hand-written table on the CPU
(tests/test_values_model.py).  Every comparison is exact, every output sits between canary guards."""
import bisect

import numpy as np
import pytest

from test_gpu_get import (COUNTS, KINDS, METRICS, NO_LEAF, NOT_FOUND, World, flushed_world, launch_cap, model_batch,
                          run as run_keys, shape_case, uneven_get_queries, uneven_world)
from test_gpu_walk import (CANARY, GUARD, LEAF_LEVEL, MALFORMED, MAX_DEPTH, dev, fixed_batch, guarded, key16, leaf,
                           malformed, model_one, uneven_tree, var_batch)

pytestmark = pytest.mark.gpu

DELETE, NOOP, WRITE, ADD, PAGE_SLICE = range(5)
OP_NONE = 0xFF
COMBINED, BAD_COMBINE = 1, 2
VCOUNTS = COUNTS + ("item_count", "bad_combine_count")
FIELDS = ("key_index", "last_index", "leaf", "where", "i32", "op", "flags", "n_items")
M32 = 0xFFFFFFFF


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available()
    return t


# ---------------------------------------------------------------------------------------
# the model: a value, its integer, the fold
# ---------------------------------------------------------------------------------------
def unpack(value):
    """(op, data) of a packed value; a value of length 0 reads as NOOP with no data."""
    return (value[0], bytes(value[1:])) if len(value) else (NOOP, b"")


def as_i32(data):
    """0 bytes: 0; 1, 2 or 3: the sign-extended little-endian integer; 4 or more: the first four."""
    if len(data) == 0:
        return 0
    return int.from_bytes(data[:4], "little", signed=True)


def signed(x):
    x &= M32
    return x - (1 << 32) if x >> 31 else x


class Fold:
    """One lookup's value.  take() folds an item and says what the descent does next: "stop" or
    "leave" (the level; the lookup goes on with the next level or the child)."""

    def __init__(self):
        self.op, self.acc, self.flags, self.n_items, self.bad = None, 0, 0, 0, 0
        self.key_index, self.leaf, self.where, self.last_index, self.last_depth = NOT_FOUND, NO_LEAF, NO_LEAF, NOT_FOUND, None

    def take(self, value, index, leaf_i, where):
        op, data = unpack(value)
        depth = where >> 8
        # the child leaf is a depth of its own: its item is always the first taken there
        first_here = (where & 0xFF) == LEAF_LEVEL or depth != self.last_depth
        self.last_depth, self.last_index = depth, index
        self.n_items += 1
        if self.op is None:                                       # no value yet: the value becomes the item
            self.op, self.key_index, self.leaf, self.where = op, index, leaf_i, where
            if op == ADD:
                self.acc = as_i32(data) & M32
                return "leave"
            return "stop"
        assert self.op == ADD                                     # (anything else ended the lookup)
        if op == WRITE:
            self.acc, self.op, self.flags = (self.acc + as_i32(data)) & M32, WRITE, self.flags | COMBINED
            return "stop"
        if op == DELETE:
            self.op, self.flags = WRITE, self.flags | COMBINED
            return "stop"
        if op == ADD:
            self.acc, self.flags = (self.acc + as_i32(data)) & M32, self.flags | COMBINED
            return "leave"
        self.flags |= BAD_COMBINE                                 # "Bad combination of opcodes": the value is unchanged
        self.bad += 1
        return "stop" if first_here else "leave"

    def record(self):
        return (self.key_index, self.last_index, self.leaf, self.where, signed(self.acc),
                OP_NONE if self.op is None else self.op, self.flags, min(self.n_items, 0xFFFF))


class Values:
    """The leaves' values as the entry points take them: bytes, offsets or a fixed stride, and the
    size the call names (which may be less than what the arrays address).  get(i) is item i's
    value under the header's clamps."""

    def __init__(self, amq, torch, blob, offs=None, stride=0, n_bytes=None, shift=0):
        self.blob = bytes(blob)
        self.offs, self.stride = (None if offs is None else [int(x) for x in offs]), stride
        self.n_bytes = len(self.blob) if n_bytes is None else n_bytes
        buf = torch.zeros(len(self.blob) + 256 + shift, dtype=torch.uint8, device="cuda")
        assert buf.data_ptr() % 256 == 0
        self.data = buf[shift:shift + len(self.blob)]
        if len(self.blob):
            self.data.copy_(torch.from_numpy(np.frombuffer(self.blob, np.uint8).copy()))
        self.d_offs = None if offs is None else dev(torch, np.array(self.offs, np.uint64).view(np.int64))
        self.n = len(self.offs) - 1 if offs is not None else None

    @classmethod
    def packed(cls, amq, torch, values, shift=0):
        """The offsets form, value after value."""
        offs = np.concatenate([[0], np.cumsum([len(v) for v in values])])
        return cls(amq, torch, b"".join(values), offs=offs, shift=shift)

    @classmethod
    def fixed(cls, amq, torch, values, shift=0):
        stride = len(values[0])
        assert stride > 0 and all(len(v) == stride for v in values)
        return cls(amq, torch, b"".join(values), stride=stride, shift=shift)

    def get(self, i):
        nb = min(self.n_bytes, len(self.blob))
        if self.offs is not None:
            b = min(self.offs[i], nb)
            e = max(min(self.offs[i + 1], nb), b)
        else:
            b, e = min(i * self.stride, nb), min((i + 1) * self.stride, nb)
        return self.blob[b:e]


def model_value(w, vals, tree, q, check_ids=False, n_nodes=None):
    """Query q over `tree` in world w with values vals: (Fold, [(class, answer, state)] per visit)."""
    visits, left, fold = [], None, Fold()
    for leaf_i, page_id, flushed_bound, where in model_one(tree, q, n_nodes):
        if where == left:                                         # the level was left: not visited
            continue
        cls, ans = w.ask(leaf_i, page_id, q, check_ids)
        state = step = None
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
                    state = "found"                               # (as a visit's class; the item is taken)
                    index = int(w.begin[leaf_i]) + at
                    step = fold.take(vals.get(index), index, leaf_i, where)
                    if step == "leave":
                        left = where
        visits.append((cls, ans, state))
        if step == "stop":
            break
    return fold, visits


def model_values(w, vals, tree, queries, check_ids=False, n_nodes=None):
    rows = [model_value(w, vals, tree, q, check_ids, n_nodes) for q in queries]
    flat = [v for _, vs in rows for v in vs]
    cls = np.array([v[0] for v in flat], np.int64)
    ans = np.array([v[1] for v in flat], np.int64)
    state = np.array([v[2] or "" for v in flat])
    metrics = [len(flat), int((cls == 0).sum()), int((cls == 1).sum()),
               int(((cls == 2) & (ans == 0)).sum()), int(((cls == 2) & (ans == 1)).sum()),
               int(((cls == 2) & (state == "absent")).sum())]
    n = {s: int((state == s).sum()) for s in ("found", "absent", "unsearchable", "flushed")}
    counts = [len(flat), n["found"] + n["absent"] + n["flushed"], sum(f.n_items > 0 for f, _ in rows), n["absent"],
              n["unsearchable"], n["flushed"], n["found"], sum(f.bad for f, _ in rows)]
    assert n["found"] == sum(f.n_items for f, _ in rows)
    rec = np.zeros(len(rows), dtype=[("key_index", "<u8"), ("last_index", "<u8"), ("leaf", "<u4"), ("where", "<u4"),
                                     ("i32", "<i4"), ("op", "u1"), ("flags", "u1"), ("n_items", "<u2")])
    for i, (f, _) in enumerate(rows):
        rec[i] = f.record()
    return {"rec": rec, "visits": np.array([len(r[1]) for r in rows], np.int64),
            "metrics": dict(zip(METRICS, metrics)), "counts": dict(zip(VCOUNTS, counts)), "rows": rows}


def model_gather(rec, vals, n_keys, out_stride):
    """(slots with CANARY where nothing is written, lengths) of tkv_amq_gather_values."""
    slots = np.full((len(rec), out_stride), CANARY, np.uint8)
    lens = np.zeros(len(rec), np.int64)
    for i, r in enumerate(rec):
        data = b""
        if int(r["key_index"]) < n_keys:
            if int(r["flags"]) & COMBINED:
                data = int(r["i32"]).to_bytes(4, "little", signed=True)
            elif int(r["op"]) != DELETE:
                data = vals.get(int(r["key_index"]))[1:]
        lens[i] = len(data)
        n = min(len(data), out_stride)
        slots[i, :n] = np.frombuffer(data[:n], np.uint8)
    return slots, lens


# ---------------------------------------------------------------------------------------
# the device side
# ---------------------------------------------------------------------------------------
def launch(amq, w, vals, tree, qb, bufs, check_ids=False, pk=None, n_nodes=None, stream=None, key_begin=None):
    d_nodes, d_segs, d_kids, d_bounds, own_pk = tree.device()
    pk = own_pk if pk is None else pk
    b = {k: (None if v is None else v[1]) for k, v in bufs.items()}
    amq.get_values_device(w.kind, w.filt if w.n else None, w.plan.device_segs() if w.n else None, w.n, d_nodes,
                          len(tree.nodes) if n_nodes is None else n_nodes, d_segs, len(tree.segments), d_kids,
                          len(tree.children), d_bounds, len(tree.flushed_bounds), pk.data, pk.offsets, pk.stride, pk.n,
                          qb.data, qb.offsets, qb.stride, qb.n, w.leaf_kb.data, w.leaf_kb.offsets, w.leaf_kb.stride,
                          w.leaf_kb.n, key_begin, vals.data, vals.d_offs, vals.stride, vals.n_bytes, b["result"],
                          b["visits"], amq.abi.GET_CHECK_PAGE_ID if check_ids else 0, b["metrics"], b["counts"], stream)


def buffers(torch, n, visits=True, metrics=True, counts=True):
    bufs = {"result": guarded(torch, 32 * n, torch.uint8), "visits": guarded(torch, n, torch.int32) if visits else None,
            "metrics": guarded(torch, 6, torch.int64) if metrics else None,
            "counts": guarded(torch, 8, torch.int64) if counts else None}
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
    out["rec"] = out.pop("result").view(amq.abi.VALUE_RESULT_DTYPE).copy()
    return out


def run(amq, torch, w, vals, tree, qb, **kw):
    opts = {k: kw.pop(k) for k in ("visits", "metrics", "counts") if k in kw}
    bufs = buffers(torch, qb.n, **opts)
    launch(amq, w, vals, tree, qb, bufs, **kw)
    return read(amq, torch, bufs)


def same(got, want, times=1):
    for name in FIELDS:
        assert np.array_equal(got["rec"][name], want["rec"][name]), name
    if "visits" in got:
        assert np.array_equal(got["visits"].astype(np.int64), want["visits"])
    if "metrics" in got:
        assert dict(zip(METRICS, (int(v) for v in got["metrics"]))) == {k: times * v for k, v in want["metrics"].items()}
    if "counts" in got:
        assert dict(zip(VCOUNTS, (int(v) for v in got["counts"]))) == {k: times * v for k, v in want["counts"].items()}


def check(amq, torch, w, vals, tree, queries, qb=None, **kw):
    want = model_values(w, vals, tree, queries, kw.get("check_ids", False), kw.get("n_nodes"))
    qb = amq.KeyBatch.from_host(queries) if qb is None else qb
    same(run(amq, torch, w, vals, tree, qb, **kw), want)
    return want


def run_gather(amq, torch, rec, vals, n_keys, out_stride, shift=0, stream=None):
    """tkv_amq_gather_values over the records `rec` (host) into guarded slots `shift` bytes past an aligned
    address; (slots, lengths), every byte the kernel did not write still CANARY."""
    n = len(rec)
    d_rec = dev(torch, np.frombuffer(rec.tobytes(), np.uint8).copy()) if n else None
    whole = torch.empty(n * out_stride + 2 * 256 + shift, dtype=torch.uint8, device="cuda")
    whole.fill_(CANARY)
    out = whole[256 + shift:256 + shift + n * out_stride]
    lens_whole, lens = guarded(torch, n, torch.int32)
    amq.gather_values_device(d_rec, n, vals.data, vals.d_offs, vals.stride, vals.n_bytes, n_keys, out, out_stride, lens,
                             stream)
    torch.cuda.synchronize()
    raw, lraw = whole.cpu().numpy(), lens_whole.cpu().numpy()
    assert (raw[:256 + shift] == CANARY).all() and (raw[256 + shift + n * out_stride:] == CANARY).all()
    assert (lraw.view(np.uint8)[:4 * GUARD] == CANARY).all() and (lraw.view(np.uint8)[4 * (GUARD + n):] == CANARY).all()
    return raw[256 + shift:256 + shift + n * out_stride].reshape(n, out_stride), lraw[GUARD:GUARD + n].astype(np.int64)


def k(i):
    return key16(i)


def i32(x, width=4):
    return int(x).to_bytes(width, "little", signed=True)


def value_list(w, value_of):
    """One value per leaf key, in the order of the leaf keys: value_of(leaf index, key)."""
    return [value_of(li, key) for li, lv in enumerate(w.leaves) for key in lv]


# ---------------------------------------------------------------------------------------
# 1. the combine table on a tree of height 2
# ---------------------------------------------------------------------------------------
# Where a key can sit, newest first: the root's three levels (leaves 2, 3, 4), the child node's one level
# (leaf 5) and the child leaf (leaf 0).  A case: name -> {place: packed value}.
PLACES = ("r0", "r1", "r2", "c0", "leaf")
PLACE_LEAF = {"r0": 2, "r1": 3, "r2": 4, "c0": 5, "leaf": 0}
PLACE_WHERE = {"r0": 0, "r1": 1, "r2": 2, "c0": 1 << 8, "leaf": 1 << 8 | LEAF_LEVEL}
TABLE = {
    "add_add_write": {"r0": bytes([ADD]) + i32(5), "r1": bytes([ADD]) + i32(-7), "r2": bytes([WRITE]) + i32(100),
                      "leaf": bytes([WRITE]) + i32(1)},
    "add_delete": {"r0": bytes([ADD]) + i32(9), "r1": bytes([DELETE]), "r2": bytes([WRITE]) + i32(3)},
    "add_x4_pending": {"r0": bytes([ADD]) + i32(1), "r1": bytes([ADD]) + i32(20), "r2": bytes([ADD]) + i32(300),
                       "leaf": bytes([ADD]) + i32(-4000)},
    "write_first": {"r0": bytes([WRITE]) + b"hello", "r1": bytes([ADD]) + i32(1), "leaf": bytes([WRITE]) + b"old"},
    "delete_first": {"r1": bytes([DELETE]), "r2": bytes([WRITE]) + i32(8)},
    "noop_first": {"r0": bytes([NOOP]) + b"xy", "r1": bytes([WRITE]) + i32(8)},
    "add_noop_write_one_node": {"r0": bytes([ADD]) + i32(2), "r1": bytes([NOOP]), "r2": bytes([WRITE]) + i32(40)},
    "add_then_noop_first_of_child": {"r0": bytes([ADD]) + i32(6), "c0": bytes([NOOP]), "leaf": bytes([WRITE]) + i32(1)},
    "add_then_slice_in_child_leaf": {"r2": bytes([ADD]) + i32(-6), "leaf": bytes([PAGE_SLICE]) + b"slice"},
    "add_add_in_child_then_write": {"r1": bytes([ADD]) + i32(1), "c0": bytes([ADD]) + i32(2),
                                         "leaf": bytes([WRITE]) + i32(3)},
    "add_noop_in_root_then_noop_first_of_child": {"r0": bytes([ADD]) + i32(70), "r2": bytes([PAGE_SLICE]) + b"p",
                                                  "c0": bytes([NOOP]) + b"q", "leaf": bytes([WRITE]) + i32(1)},
    "only_in_the_leaf": {"leaf": bytes([WRITE]) + b"bottom"},
    "nowhere": {},
}
# name -> (op, flags, i32, n_items, first place, last place, visits)
TABLE_WANT = {
    "add_add_write": (WRITE, COMBINED, 98, 3, "r0", "r2", 3),
    "add_delete": (WRITE, COMBINED, 9, 2, "r0", "r1", 2),
    "add_x4_pending": (ADD, COMBINED, -3679, 4, "r0", "leaf", 5),
    "write_first": (WRITE, 0, 0, 1, "r0", "r0", 1),
    "delete_first": (DELETE, 0, 0, 1, "r1", "r1", 2),
    "noop_first": (NOOP, 0, 0, 1, "r0", "r0", 1),
    "add_noop_write_one_node": (WRITE, COMBINED | BAD_COMBINE, 42, 3, "r0", "r2", 3),
    "add_then_noop_first_of_child": (ADD, BAD_COMBINE, 6, 2, "r0", "c0", 4),      # the leaf's WRITE is never visited
    "add_then_slice_in_child_leaf": (ADD, BAD_COMBINE, -6, 2, "r2", "leaf", 5),
    "add_add_in_child_then_write": (WRITE, COMBINED, 6, 3, "r1", "leaf", 5),
    "add_noop_in_root_then_noop_first_of_child": (ADD, BAD_COMBINE, 70, 3, "r0", "c0", 4),
    "only_in_the_leaf": (WRITE, 0, 0, 1, "leaf", "leaf", 5),
    "nowhere": (OP_NONE, 0, 0, 0, None, None, 5),
}


def table_world(oracle, amq, torch, kind):
    names = list(TABLE)
    key_of = {name: k(100 + 10 * j) for j, name in enumerate(names)}
    filler = [k(100 + 10 * j + 5) for j in range(len(names))]     # in every leaf, a WRITE everywhere
    leaves = [[] for _ in range(6)]
    held = {}
    for name, places in TABLE.items():
        for place, value in places.items():
            leaves[PLACE_LEAF[place]].append(key_of[name])
            held[(PLACE_LEAF[place], key_of[name])] = value
    leaves = [sorted(lv + filler) for lv in leaves]
    leaves[1] = [k(5000)]                                         # the child's second leaf: nothing of ours
    w = World(oracle, amq, torch, kind, leaves)
    seg = lambda i: {"leaf": i, "page_id": 7000 + i, "active": 0b1, "flushed": {}}
    child = {"pivot_keys": [k(0), k(4000), k(9000)], "children": [leaf(0), leaf(1)], "levels": [[seg(5)]], "page_id": 71}
    root = {"pivot_keys": [k(0), k(9000)], "children": [child], "levels": [[seg(2)], [seg(3)], [seg(4)]]}
    tree = amq.TreeIndex.from_description(root)
    assert tree.nodes[0]["height"] == 2
    values = value_list(w, lambda li, key: held.get((li, key), bytes([WRITE]) + b"fill"))
    return w, tree, key_of, values


@pytest.mark.parametrize("kind", KINDS)
def test_the_combine_table(oracle, amq, torch, kind):
    w, tree, key_of, values = table_world(oracle, amq, torch, kind)
    vals = Values.packed(amq, torch, values)
    names = list(TABLE)
    qs = [key_of[n] for n in names]
    want = check(amq, torch, w, vals, tree, qs)
    at = lambda place, key: int(w.begin[PLACE_LEAF[place]]) + w.leaves[PLACE_LEAF[place]].index(key)
    bad = 0
    for i, name in enumerate(names):                              # the model against the table written by hand
        op, flags, acc, n_items, first, last, visits = TABLE_WANT[name]
        r = want["rec"][i]
        assert (int(r["op"]), int(r["flags"]), int(r["i32"]), int(r["n_items"])) == (op, flags, acc, n_items), name
        assert int(want["visits"][i]) == visits, name
        if first is None:
            assert (int(r["key_index"]), int(r["last_index"]), int(r["leaf"]), int(r["where"])) == \
                (NOT_FOUND, NOT_FOUND, NO_LEAF, NO_LEAF), name
        else:
            assert (int(r["key_index"]), int(r["leaf"]), int(r["where"])) == \
                (at(first, qs[i]), PLACE_LEAF[first], PLACE_WHERE[first]), name
            assert int(r["last_index"]) == at(last, qs[i]), name
        bad += bool(flags & BAD_COMBINE)
    c = want["counts"]
    assert c["found_count"] == len(names) - 1 and c["item_count"] == sum(v[3] for v in TABLE_WANT.values())
    assert c["bad_combine_count"] == bad + 1                      # (one lookup meets two)
    assert c["visit_count"] == sum(v[6] for v in TABLE_WANT.values()) == want["metrics"]["total_filter_query_count"]
    # the fixed-stride form cannot hold this table (its values differ in length); the wrapper, with a gather
    vc, pm = amq.ValueCounts(), amq.ProbeMetrics()
    r = amq.get_values(w.plan, w.filt, tree, amq.KeyBatch.from_host(qs), w.leaf_kb,
                       amq.KeyBatch.variable(vals.data, vals.d_offs), want_visits=True, metrics=pm, counts=vc, gather=8)
    got = r.records()
    for name in FIELDS:
        assert np.array_equal(got[name], want["rec"][name]), name
    assert np.array_equal(r.visits.cpu().numpy(), want["visits"])
    assert np.array_equal(r.key_index.cpu().numpy().view(np.uint64), want["rec"]["key_index"])
    assert np.array_equal(r.leaf.cpu().numpy().view(np.uint32), want["rec"]["leaf"])
    assert np.array_equal(r.where.cpu().numpy().view(np.uint32), want["rec"]["where"])
    assert vc.collect() == want["counts"] and pm.collect() == want["metrics"]
    slots, lens = model_gather(want["rec"], vals, len(values), 8)
    assert np.array_equal(r.lengths.cpu().numpy(), lens)
    got_slots = r.slots.cpu().numpy()
    for i in range(len(qs)):
        n = min(int(lens[i]), 8)
        assert np.array_equal(got_slots[i, :n], slots[i, :n]), names[i]
    assert bytes(got_slots[names.index("write_first"), :5]) == b"hello" and lens[names.index("only_in_the_leaf")] == 6
    assert bytes(got_slots[names.index("add_add_write"), :4]) == i32(98)


# ---------------------------------------------------------------------------------------
# 2. the flushed rule against the value rule
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_the_flushed_rule_against_the_value_rule(oracle, amq, torch, kind):
    """test_gpu_get.py's flushed world -- level 0: leaves 2 then 3, level 1: leaf 4 -- with every item an ADD but
    the child leaves' (WRITE).  X is flushed from leaf 2 (not taken, level left, leaf 3 not visited), taken AT its
    bound in leaf 4.  E is absent from leaf 2 and taken from leaf 3; Y is taken from leaf 2 and the level left."""
    w, tree, (X, Y, Z, E) = flushed_world(oracle, amq, torch, kind)
    qs = [X, Y, Z, E, k(601), k(20), k(901), k(600)] + [k(j) for j in range(400, 1000, 7)]
    values = value_list(w, lambda li, key: (bytes([WRITE]) + i32(1000 + li)) if li < 2 else (bytes([ADD]) + i32(1 << li)))
    for vals in (Values.packed(amq, torch, values), Values.fixed(amq, torch, values, shift=3)):
        want = check(amq, torch, w, vals, tree, qs)
        rec = want["rec"]
        # X: flushed (leaf 2), taken (leaf 4, an ADD of 16), absent from the child leaf: pending, 3 visits, 1 item
        assert [v[2] for v in want["rows"][0][1]][:2] == ["flushed", "found"] and int(want["visits"][0]) == 3
        assert len(model_one(tree, X)) == 4
        assert (int(rec["op"][0]), int(rec["i32"][0]), int(rec["n_items"][0]), int(rec["leaf"][0])) == (ADD, 16, 1, 4)
        # Y (pivot 0): taken from leaf 2, the level is left, nothing else holds it
        assert (int(rec["op"][1]), int(rec["i32"][1]), int(rec["leaf"][1]), int(rec["flags"][1])) == (ADD, 4, 2, 0)
        # E: absent from leaf 2, taken from leaf 3 (8) and from leaf 4 (16): pending 24, combined
        assert (int(rec["op"][3]), int(rec["i32"][3]), int(rec["n_items"][3]), int(rec["flags"][3])) == (ADD, 24, 2, COMBINED)
        assert (int(rec["leaf"][3]), int(rec["where"][3])) == (3, 0)
        # Z: flushed from both levels, in no child leaf: nothing
        assert int(rec["op"][2]) == OP_NONE and int(rec["n_items"][2]) == 0
        # k(600) is only in child leaf 1: a WRITE, the item's own bytes
        assert (int(rec["op"][7]), int(rec["flags"][7]), int(rec["i32"][7]), int(rec["leaf"][7])) == (WRITE, 0, 0, 1)
        assert want["counts"]["flushed_count"] >= 3 and want["counts"]["item_count"] > want["counts"]["found_count"]
    # X in a second segment of level 1 is never visited once leaf 4's ADD is taken: put leaf 3 there
    t2 = {"pivot_keys": [k(0), k(500), k(1000)], "children": [leaf(0), leaf(1)],
          "levels": [[{"leaf": 2, "page_id": 7002, "active": 0b11, "flushed": {}}],
                     [{"leaf": 4, "page_id": 7004, "active": 0b11, "flushed": {}},
                      {"leaf": 3, "page_id": 7003, "active": 0b11, "flushed": {}}]]}
    tree2 = amq.TreeIndex.from_description(t2)
    vals = Values.packed(amq, torch, values)
    want = check(amq, torch, w, vals, tree2, [X, E])
    # X: leaf 2 (4), leaf 4 (16), not leaf 3 (which holds it: 8), the child: 3 visits of the 4 entries
    assert len(model_one(tree2, X)) == 4 and int(want["visits"][0]) == 3
    assert (int(want["rec"]["i32"][0]), int(want["rec"]["n_items"][0])) == (20, 2)
    assert (int(want["rec"]["i32"][1]), int(want["rec"]["n_items"][1])) == (16, 1)   # E: leaf 4, not leaf 3


# ---------------------------------------------------------------------------------------
# 3. filters between the levels of a chain
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_filters_between_the_levels_of_a_chain(oracle, amq, torch, kind):
    """Seven root levels; the chain's keys are ADDs in the first and the last, and between them lie a level whose
    filter rejects, a leaf outside the plan and -- for the keys picked so -- a false positive.  A WRITE in the
    child leaf ends every chain."""
    chain = [k(2 * j) for j in range(300)]
    others = [[k(10_000 + 1000 * lv + j) for j in range(400)] for lv in range(4)]
    leaves = [sorted(chain), [k(9_000_000)],                      # the child leaves
              sorted(chain), others[0], others[1], others[2], others[3], sorted(chain)]
    w = World(oracle, amq, torch, kind, leaves)
    seg = lambda i, pid=None: {"leaf": i, "page_id": 7000 + i if pid is None else pid, "active": 0b1, "flushed": {}}
    root = {"pivot_keys": [k(0), k(5_000_000), k(9_999_999)], "children": [leaf(0), leaf(1)],
            "levels": [[seg(2)], [seg(3)], [seg(99, 5)], [seg(4)], [seg(5)], [seg(6)], [seg(7)]]}
    tree = amq.TreeIndex.from_description(root)
    qs = chain + [k(2 * j + 1) for j in range(200)]
    values = value_list(w, lambda li, key: (bytes([WRITE]) + i32(7)) if li < 2 else (bytes([ADD]) + i32(li)))
    vals = Values.fixed(amq, torch, values)
    want = check(amq, torch, w, vals, tree, qs, check_ids=True)
    hit = want["rec"][:len(chain)]
    assert (hit["op"] == WRITE).all() and (hit["i32"] == 2 + 7 + 7).all() and (hit["n_items"] == 3).all()
    assert (hit["flags"] == COMBINED).all() and (want["visits"][:len(chain)] == 8).all()
    assert (want["rec"]["op"][len(chain):] == OP_NONE).all()
    m, c = want["metrics"], want["counts"]
    assert m["filter_reject_count"] > 1000 and c["unsearchable_count"] == len(qs) == m["no_filter_page_count"]
    between = [vs[1:7] for _, vs in want["rows"][:len(chain)]]
    assert sum(any(v[2] == "absent" and v[0] == 2 for v in vs) for vs in between) > 0   # a false positive in between
    assert m["filter_false_positive_count"] > 0


# ---------------------------------------------------------------------------------------
# 4. as_i32 widths and wrap, through the kernel, in both value forms
# ---------------------------------------------------------------------------------------
INTS = {0: [0], 1: [-128, -1, 127, 5], 2: [-32768, -2, 0x7FFF, 300], 3: [-(1 << 23), -3, (1 << 23) - 1, 70000],
        4: [-(1 << 31), -4, 0x7FFFFFFF, 1], 8: [-(1 << 31), -5, 0x7FFFFFFF, 1]}


def width_world(oracle, amq, torch, kind):
    """One node, level 0 (leaf 1) over level 1 (leaf 2) over the child leaf 0; every key in all three."""
    keys = [k(j) for j in range(40)]
    w = World(oracle, amq, torch, kind, [keys, keys, keys])
    seg = lambda i: {"leaf": i, "page_id": 7000 + i, "active": 0b1, "flushed": {}}
    root = {"pivot_keys": [k(0), k(9999)], "children": [leaf(0)], "levels": [[seg(1)], [seg(2)]]}
    return w, amq.TreeIndex.from_description(root), keys


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("width", [0, 1, 2, 3, 4, 8])
def test_as_i32_widths(oracle, amq, torch, kind, width):
    w, tree, keys = width_world(oracle, amq, torch, kind)

    def data(x):
        return b"" if width == 0 else i32(x, width) if width < 8 else i32(x) + b"\xAA\xBB\xCC\xDD"

    xs = INTS[width]
    # key j: ADD xs[j % n] over ADD 1000 over WRITE xs[(j + 1) % n]; the middle one is four bytes wide if it fits
    def value_of(li, key):
        j = keys.index(key)
        if li == 1:
            return bytes([ADD]) + data(xs[j % len(xs)])
        if li == 2:
            return bytes([ADD]) + (data(1000) if width in (2, 3, 4, 8) else data(xs[0]))
        return bytes([WRITE]) + data(xs[(j + 1) % len(xs)])

    values = value_list(w, value_of)
    for vals in (Values.packed(amq, torch, values, shift=1), Values.fixed(amq, torch, values, shift=2)):
        want = check(amq, torch, w, vals, tree, keys)
        mid = 1000 if width in (2, 3, 4, 8) else xs[0]
        for j in range(len(keys)):
            total = signed(xs[j % len(xs)] + mid + xs[(j + 1) % len(xs)])
            assert int(want["rec"]["i32"][j]) == total and int(want["rec"]["op"][j]) == WRITE, j
        assert (want["rec"]["n_items"] == 3).all()
    if width in (4, 8):                                           # 0x7fffffff + 1 wraps to the most negative integer
        j = [(xs[j % len(xs)], xs[(j + 1) % len(xs)]) for j in range(len(keys))].index((0x7FFFFFFF, 1))
        values[int(w.begin[2]) + j] = bytes([ADD]) + data(0)
        vals = Values.packed(amq, torch, values)
        want = check(amq, torch, w, vals, tree, keys)
        assert int(want["rec"]["i32"][j]) == -(1 << 31)


# ---------------------------------------------------------------------------------------
# 5. value array edges
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_value_array_edges(oracle, amq, torch, kind):
    w, tree, keys = width_world(oracle, amq, torch, kind)
    n = len(keys)
    base = value_list(w, lambda li, key: (bytes([ADD]) + i32(3 + li)) if li else (bytes([WRITE]) + i32(50)))
    # offsets: a zero-length value in level 0 (NOOP: ends the lookup), an end below its begin, offsets past the size
    offs = np.concatenate([[0], np.cumsum([len(v) for v in base])]).astype(np.int64)
    blob = b"".join(base)
    o = offs.copy()
    zero_at, back_at = int(w.begin[1]) + 4, int(w.begin[1]) + 9
    o[zero_at + 1] = o[zero_at]                                   # item zero_at is empty (the next one starts late)
    o[back_at + 1] = o[back_at] - 3                               # item back_at ends below its begin: empty
    vals = Values(amq, torch, blob, offs=o)
    want = check(amq, torch, w, vals, tree, keys)
    for j in (4, 9):
        assert (int(want["rec"]["op"][j]), int(want["rec"]["n_items"][j]), int(want["visits"][j])) == (NOOP, 1, 1)
    assert int(want["rec"]["op"][5]) == WRITE
    # the size names less than the arrays address: level 1's last items and the whole of... nothing else is cut
    cut = int(offs[int(w.begin[2]) + n - 3]) + 2                  # two bytes into the third-last item of leaf 2
    vals = Values(amq, torch, blob, offs=offs, n_bytes=cut)
    want = check(amq, torch, w, vals, tree, keys)
    # that item is ADD with one data byte (3 + 2 = 5, as_i32 of one byte); the two behind it are empty: NOOP, a bad
    # combination after level 0's ADD in the same node: the lookup goes on to the child's WRITE
    assert int(want["rec"]["i32"][n - 3]) == 4 + 5 + 50 and int(want["rec"]["flags"][n - 3]) == COMBINED
    assert int(want["rec"]["i32"][n - 1]) == 4 + 50 and int(want["rec"]["flags"][n - 1]) == COMBINED | BAD_COMBINE
    assert want["counts"]["bad_combine_count"] == 2
    # offsets far past the size, and the largest there are
    o = offs.copy()
    o[int(w.begin[1]):] = np.array([1 << 40, (1 << 63) - 1] * n * 2, np.int64)[:len(o) - int(w.begin[1])]
    vals = Values(amq, torch, blob, offs=o)
    want = check(amq, torch, w, vals, tree, keys)
    assert (want["rec"]["op"] == NOOP).all() and (want["rec"]["n_items"] == 1).all()
    # a fixed stride whose last item crosses the buffer end, and items wholly past it
    for short in (1, 3, 5, 6, 11):
        vals = Values(amq, torch, blob, stride=5, n_bytes=len(blob) - short)
        want = check(amq, torch, w, vals, tree, keys)
        assert (want["rec"]["op"][:n - 3] == WRITE).all()
    assert int(want["rec"]["i32"][n - 1]) == 4 + 50 and int(want["rec"]["flags"][n - 1]) == COMBINED | BAD_COMBINE
    # no value bytes at all: every item is an empty NOOP
    vals = Values(amq, torch, blob, stride=5, n_bytes=0)
    want = check(amq, torch, w, vals, tree, keys)
    assert (want["rec"]["op"] == NOOP).all()


# ---------------------------------------------------------------------------------------
# 6. equivalence with tkv_amq_get_keys
# ---------------------------------------------------------------------------------------
def write_values(amq, torch, w, form):
    n = int(w.begin[-1])
    values = [bytes([WRITE]) + i32(j * 2654435761 & 0x7FFFFFFF) for j in range(n)]
    return Values.fixed(amq, torch, values, shift=1) if form == "fixed" else Values.packed(amq, torch, values)


def equal_to_get_keys(amq, torch, w, vals, tree, qs, qb, pk, check_ids):
    want = model_values(w, vals, tree, qs, check_ids)
    got = run(amq, torch, w, vals, tree, qb, pk=pk, check_ids=check_ids)
    same(got, want)
    keys = run_keys(amq, torch, w, tree, qb, pk=pk, check_ids=check_ids)
    plain = model_batch(w, tree, qs, check_ids)
    for name in ("key_index", "leaf", "where"):
        assert np.array_equal(got["rec"][name], keys[name]) and np.array_equal(keys[name], plain[name]), name
    assert np.array_equal(got["rec"]["last_index"], keys["key_index"])
    assert np.array_equal(got["visits"], keys["visits"]) and np.array_equal(got["metrics"], keys["metrics"])
    assert np.array_equal(got["counts"][:6], keys["counts"]) and int(got["counts"][6]) == int(keys["counts"][2])
    assert int(got["counts"][7]) == 0 and not got["rec"]["flags"].any() and not got["rec"]["i32"].any()
    found = keys["leaf"] != NO_LEAF
    assert (got["rec"]["op"][found] == WRITE).all() and (got["rec"]["op"][~found] == OP_NONE).all()
    assert np.array_equal(got["rec"]["n_items"], found.astype(np.uint16))
    return want


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", ["k16", "k16_shift4", "k24", "var", "q_fixed_leaves_offs"])
def test_equals_get_keys_when_every_value_is_a_write(oracle, amq, torch, kind, shape):
    w, tree, qs, pk = shape_case(oracle, amq, torch, kind, shape)
    qb = var_batch(amq, torch, qs) if shape == "var" else fixed_batch(amq, torch, qs, len(qs[0]))
    vals = write_values(amq, torch, w, "fixed" if shape in ("k16", "k24") else "offsets")
    for check_ids in (False, True):
        want = equal_to_get_keys(amq, torch, w, vals, tree, qs, qb, pk, check_ids)
        assert 100 < want["counts"]["found_count"] < len(qs) and want["counts"]["unsearchable_count"] > 0


@pytest.mark.parametrize("kind,bpk,shape", [(0, 14, "k16"), (0, 14, "k24"), (0, 10, "k40"), (0, 14, "k40"),
                                            (1, 22, "k16"), (1, 12, "k40")])
def test_equals_get_keys_on_every_hash_path(oracle, amq, torch, kind, bpk, shape):
    w, tree, qs, pk = shape_case(oracle, amq, torch, kind, shape, bpk)
    vals = write_values(amq, torch, w, "fixed")
    want = equal_to_get_keys(amq, torch, w, vals, tree, qs, fixed_batch(amq, torch, qs, len(qs[0])), pk, True)
    assert want["counts"]["found_count"] > 100 and want["metrics"]["filter_reject_count"] > 100


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", ["k16", "k24", "var"])
def test_key_shapes_with_deltas(oracle, amq, torch, kind, shape):
    """The same worlds with the update buffers' items ADDs: every hit in a buffer goes on to the bottom."""
    w, tree, qs, pk = shape_case(oracle, amq, torch, kind, shape)
    values = value_list(w, lambda li, key: (bytes([WRITE]) + i32(len(key))) if li < 6 else (bytes([ADD]) + i32(li - 9)))
    vals = Values.fixed(amq, torch, values)
    qb = var_batch(amq, torch, qs) if shape == "var" else fixed_batch(amq, torch, qs, len(qs[0]))
    want = check(amq, torch, w, vals, tree, qs, qb=qb, pk=pk, check_ids=True)
    assert want["counts"]["item_count"] > want["counts"]["found_count"] + 50
    assert (want["rec"]["flags"] & COMBINED).sum() > 50 and (want["rec"]["op"] == ADD).sum() > 10


# ---------------------------------------------------------------------------------------
# 7. the uneven tree, malformed trees, the cycle: a mix of ops
# ---------------------------------------------------------------------------------------
def mixed_values(amq, torch, w, seed=5):
    rng = np.random.default_rng(seed)
    ops = [ADD, ADD, ADD, WRITE, WRITE, DELETE, NOOP, PAGE_SLICE, 9]
    values = []
    for _ in range(int(w.begin[-1])):
        op = ops[int(rng.integers(0, len(ops)))]
        values.append(bytes([op]) + bytes(rng.integers(0, 256, int(rng.integers(0, 7)), dtype=np.uint8)))
    values[0] = b""
    return Values.packed(amq, torch, values)


@pytest.mark.parametrize("kind", KINDS)
def test_the_uneven_tree_with_its_flushed_bounds(oracle, amq, torch, kind):
    w, tree, qs = uneven_world(oracle, amq, torch, kind), uneven_tree(amq), uneven_get_queries()
    want = check(amq, torch, w, mixed_values(amq, torch, w), tree, qs, check_ids=True)
    c = want["counts"]
    assert c["flushed_count"] > 10 and c["found_count"] > 50 and c["item_count"] > c["found_count"] + 10
    assert c["bad_combine_count"] > 0 and (want["rec"]["n_items"] >= 3).any()
    assert {int(x) for x in want["rec"]["op"]} >= {DELETE, NOOP, WRITE, ADD, PAGE_SLICE, 9, OP_NONE}


@pytest.mark.parametrize("name", MALFORMED)
def test_malformed_trees_answer_as_the_clamped_model(oracle, amq, torch, name):
    w = uneven_world(oracle, amq, torch, 0)
    check(amq, torch, w, mixed_values(amq, torch, w), malformed(amq, name), uneven_get_queries())


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
    values = value_list(w, lambda li, key: bytes([ADD]) + i32(key[-1]))
    want = check(amq, torch, w, Values.fixed(amq, torch, values), t, qs)
    # key 2 is flushed at every depth; key 3 and key 4 are taken at every depth: MAX_DEPTH items each
    assert int(want["visits"][2]) == MAX_DEPTH and int(want["rec"]["n_items"][2]) == 0
    for j in (3, 4):
        assert (int(want["rec"]["n_items"][j]), int(want["rec"]["i32"][j]), int(want["rec"]["op"][j])) == \
            (MAX_DEPTH, MAX_DEPTH * j, ADD)
        assert int(want["rec"]["last_index"][j]) == int(want["rec"]["key_index"][j])
    want = check(amq, torch, w, Values.fixed(amq, torch, values), t, qs, n_nodes=0)
    assert (want["rec"]["op"] == OP_NONE).all() and not want["visits"].any() and want["counts"]["visit_count"] == 0


# ---------------------------------------------------------------------------------------
# 8. batch sizes and optional outputs
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_batch_size_edges(oracle, amq, torch, kind):
    w, tree, key_of, values = table_world(oracle, amq, torch, kind)
    vals = Values.packed(amq, torch, values)
    base = [key_of[n] for n in TABLE]
    one = model_values(w, vals, tree, base)
    rows = [model_values(w, vals, tree, [b]) for b in base]
    grid, threads = launch_cap()
    # 0: nothing written; grid * threads + 1: the smallest batch that takes a second grid round -- the first
    # workgroup's first wave carries its tallies from tile 0 into tile `grid`
    for nq in (0, 1, 255, 256, 257, grid * threads + 1):
        pick = np.random.default_rng(nq).integers(0, len(base), nq)
        q = np.frombuffer(b"".join(base), np.uint8).reshape(len(base), 16)[pick]
        qb = amq.KeyBatch(torch.empty((0, 16), dtype=torch.uint8, device="cuda"), 0, 16, None) if nq == 0 else \
            amq.KeyBatch.fixed(dev(torch, q))
        got = run(amq, torch, w, vals, tree, qb)
        for name in FIELDS:
            assert np.array_equal(got["rec"][name], one["rec"][name][pick]), (nq, name)
        assert np.array_equal(got["visits"].astype(np.int64), one["visits"][pick])
        per = np.bincount(pick, minlength=len(base))
        for names, field in ((METRICS, "metrics"), (VCOUNTS, "counts")):
            assert dict(zip(names, (int(v) for v in got[field]))) == \
                {n: sum(int(c) * r[field][n] for c, r in zip(per, rows)) for n in names}, (nq, field)
    # every optional output as NULL, one at a time and all at once: the same records
    qb = amq.KeyBatch.from_host(base)
    for off in ({"visits": False}, {"metrics": False}, {"counts": False},
                {"visits": False, "metrics": False, "counts": False}):
        same(run(amq, torch, w, vals, tree, qb, **off), one)


# ---------------------------------------------------------------------------------------
# 9. graph capture: the lookup and the gather as one linear chain
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_lookup_and_gather_replay_in_a_graph(oracle, amq, torch, kind):
    w, tree, qs, pk = shape_case(oracle, amq, torch, kind, "k16")
    values = value_list(w, lambda li, key: (bytes([WRITE]) + key[:11]) if li < 6 else (bytes([ADD]) + i32(li - 9)))
    vals = Values.packed(amq, torch, values)
    want = model_values(w, vals, tree, qs, True)
    out_stride = 8
    slots, lens = model_gather(want["rec"], vals, len(values), out_stride)
    qb = fixed_batch(amq, torch, qs, 16)
    bufs = buffers(torch, qb.n)
    out_whole, out = guarded(torch, qb.n * out_stride, torch.uint8)
    len_whole, d_lens = guarded(torch, qb.n, torch.int32)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())

    def both():
        launch(amq, w, vals, tree, qb, bufs, check_ids=True, stream=s)
        amq.gather_values_device(bufs["result"][1], qb.n, vals.data, vals.d_offs, vals.stride, vals.n_bytes,
                                 len(values), out, out_stride, d_lens, s)

    def verify():
        same(read(amq, torch, bufs), want)
        raw = out_whole.cpu().numpy()
        assert (raw[:GUARD] == CANARY).all() and (raw[len(raw) - GUARD:] == CANARY).all()
        assert np.array_equal(raw[GUARD:len(raw) - GUARD].reshape(qb.n, out_stride), slots)
        lraw = len_whole.cpu().numpy()
        assert np.array_equal(lraw[GUARD:GUARD + qb.n], lens) and (lraw.view(np.uint8)[:4 * GUARD] == CANARY).all()

    with torch.cuda.stream(s):                                    # warm-up on the capture stream: the eager run
        both()
    s.synchronize()
    verify()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        both()
    for _ in range(2):                                            # counters zeroed, outputs refilled between replays
        for name in ("metrics", "counts"):
            bufs[name][1].zero_()
        bufs["result"][1].fill_(CANARY)
        bufs["visits"][1].view(torch.uint8).fill_(CANARY)
        out.fill_(CANARY)
        d_lens.view(torch.uint8).fill_(CANARY)
        torch.cuda.synchronize()
        graph.replay()
        verify()


# ---------------------------------------------------------------------------------------
# 10. the gather
# ---------------------------------------------------------------------------------------
def record(key_index, op=WRITE, flags=0, acc=0, n_items=1):
    return (key_index, key_index, 0, 0, acc, op, flags, n_items)


@pytest.mark.parametrize("out_stride", [3, 8, 21, 128])
@pytest.mark.parametrize("form", ["offsets", "fixed"])
def test_the_gather(amq, torch, out_stride, form):
    dtype = np.dtype([("key_index", "<u8"), ("last_index", "<u8"), ("leaf", "<u4"), ("where", "<u4"), ("i32", "<i4"),
                      ("op", "u1"), ("flags", "u1"), ("n_items", "<u2")])
    rng = np.random.default_rng(out_stride)
    lengths = [0, 1, 3, 4, 5, out_stride - 1, out_stride, out_stride + 5, 2 * out_stride + 3, 101]
    if form == "fixed":
        # one length per array: try each
        arrays = [[bytes([WRITE]) + bytes(rng.integers(0, 256, n, dtype=np.uint8)) for _ in range(9)] for n in lengths]
    else:
        # every length, interleaved with empty values, so the starts fall on all four byte alignments
        values = []
        for rep in range(4):
            for n in lengths:
                values.append(bytes([WRITE, ADD, NOOP, PAGE_SLICE][rep]) + bytes(rng.integers(0, 256, n, dtype=np.uint8)))
            values.append(b"")
            values.append(bytes([WRITE]) * (rep + 1))
        arrays = [values]
    for values in arrays:
        n_keys = len(values)
        for shift in (0, 1, 2, 3):
            vals = Values.fixed(amq, torch, values, shift=shift) if form == "fixed" else \
                Values.packed(amq, torch, values, shift=shift)
            if form == "offsets":
                starts = {(vals.data.data_ptr() + o + 1) % 4 for o in vals.offs[:-1]}
                assert starts == {0, 1, 2, 3}
            rows = [record(j, op=unpack(values[j])[0]) for j in range(n_keys)]
            rows += [record(1, op=WRITE, flags=COMBINED, acc=-2), record(2, op=ADD, flags=COMBINED | BAD_COMBINE, acc=0x12345678),
                     record(3, op=DELETE), record(NOT_FOUND, op=OP_NONE, n_items=0),
                     record(n_keys, op=WRITE), record(n_keys + (1 << 40), op=WRITE, flags=COMBINED, acc=7),
                     record((1 << 63) + 5, op=ADD)]
            rec = np.array(rows, dtype=dtype)
            want_slots, want_lens = model_gather(rec, vals, n_keys, out_stride)
            assert want_lens[n_keys] == 4 and want_lens[n_keys + 2] == 0 and not want_lens[n_keys + 3:].any()
            for out_shift in ((0, 5) if shift == 0 else (0,)):
                slots, lens = run_gather(amq, torch, rec, vals, n_keys, out_stride, shift=out_shift)
                assert np.array_equal(lens, want_lens)
                assert np.array_equal(slots, want_slots)          # CANARY wherever nothing is to be written
    # an empty batch, and lengths alone (out_stride 0, no slots)
    vals = Values.packed(amq, torch, [bytes([WRITE]) + b"abc"])
    run_gather(amq, torch, np.zeros(0, dtype), vals, 1, out_stride)
    d_rec = dev(torch, np.frombuffer(np.array([record(0)], dtype).tobytes(), np.uint8).copy())
    _, d_len = guarded(torch, 1, torch.int32)
    amq.gather_values_device(d_rec, 1, vals.data, vals.d_offs, vals.stride, vals.n_bytes, 1, None, 0, d_len)
    assert int(d_len.cpu()[0]) == 3
