"""tkv_amq_walk_paths as far as it goes without a device: the symbols bind, the three tree records
are 32, 32 and 16 bytes with their fields where the header puts them, the workspace size, every
InvalidArgument case of include/tkv_amq.h judged on host pointers that are never dereferenced, the
answer without a GPU, and TreeIndex (description -> flat arrays -> description, and the
PackedNodePage limits it refuses).  tests/test_gpu_walk.py holds the device code to a bisect model."""
import ctypes
import os
import re

import numpy as np
import pytest

from turtle_kv_amd import abi


@pytest.fixture(scope="module")
def L():
    return abi.lib()


@pytest.fixture(scope="module")
def some():
    """A 16-byte aligned host address: the argument checks look at pointers, never through them."""
    buf = (ctypes.c_uint8 * 4096)()
    p = ctypes.addressof(buf)
    p = p + (-p % 16)
    return buf, p


def call(L, nodes=None, n_nodes=2, segs=None, n_segs=3, kids=None, n_kids=4, bounds=None, n_bounds=2, pk=None,
         pkoffs=None, pkstride=16, n_pk=5, q=None, qoffs=None, qstride=16, n_queries=4, begin=None, leaf=None,
         page=None, flushed=None, where=None, capacity=8, needed=None, ws=None, ws_bytes=None):
    v = ctypes.c_void_p
    if ws_bytes is None:
        ws_bytes = L.tkv_amq_walk_paths_ws_bytes(n_queries if n_queries <= 0xffffffff else 0)
    return L.tkv_amq_walk_paths(v(nodes), n_nodes, v(segs), n_segs, v(kids), n_kids, v(bounds), n_bounds, v(pk),
                                v(pkoffs), pkstride, n_pk, v(q), v(qoffs), qstride, n_queries, v(begin), v(leaf),
                                v(page), v(flushed), v(where), capacity, v(needed), v(ws), ws_bytes, None)


def good_args(p):
    return dict(nodes=p, segs=p, kids=p, bounds=p, pk=p, q=p, begin=p, leaf=p, ws=p)


def test_symbols_exist_and_bind(L):
    for name in ("tkv_amq_walk_paths_ws_bytes", "tkv_amq_walk_paths"):
        assert name in abi.EXPORTS and hasattr(L, name)
    assert L.tkv_amq_walk_paths.restype is ctypes.c_int and len(L.tkv_amq_walk_paths.argtypes) == 26
    import turtle_kv_amd as amq
    for name in ("TreeIndex", "WalkResult", "walk_paths", "walk_paths_device", "walk_paths_workspace_bytes"):
        assert hasattr(amq, name) and name in amq.__all__


def test_record_sizes_and_field_offsets():
    assert (ctypes.sizeof(abi.TreeNode), ctypes.sizeof(abi.TreeSegment), ctypes.sizeof(abi.TreeChild)) == (32, 32, 16)
    assert (abi.TREE_NODE_DTYPE.itemsize, abi.TREE_SEGMENT_DTYPE.itemsize, abi.TREE_CHILD_DTYPE.itemsize) == \
        (32, 32, 16)
    want = {abi.TreeNode: (abi.TREE_NODE_DTYPE, {"pivot_key_begin": 0, "seg_begin": 4, "child_begin": 8,
                                                 "pivot_count": 16, "height": 17, "level_count": 18,
                                                 "level_start": 20}),
            abi.TreeSegment: (abi.TREE_SEGMENT_DTYPE, {"leaf_page_id": 0, "active_pivots": 8, "flushed_pivots": 16,
                                                       "leaf": 24, "flushed_begin": 28}),
            abi.TreeChild: (abi.TREE_CHILD_DTYPE, {"page_id": 0, "index": 8})}
    for struct, (dtype, fields) in want.items():
        for name, off in fields.items():
            assert getattr(struct, name).offset == off == dtype.fields[name][1], (struct, name)
    assert abi.TreeNode.level_start.size == 8 and abi.TREE_NODE_DTYPE.fields["level_start"][0].shape == (8,)


def test_header_declares_the_records_and_keeps_the_abi_version():
    with open(os.path.join(abi._build.ROOT, "include", "tkv_amq.h")) as f:
        src = f.read()
    assert "#define TKV_AMQ_ABI_VERSION 3\n" in src
    for name, value in (("TKV_AMQ_WALK_MAX_DEPTH", abi.WALK_MAX_DEPTH), ("TKV_AMQ_WALK_LEAF_LEVEL",
                                                                        abi.WALK_LEAF_LEVEL)):
        m = re.search(r"#define %s (0x[0-9a-f]+|\d+)u\b" % name, src)
        assert m and int(m.group(1), 0) == value, name
    assert (abi.WALK_MAX_DEPTH, abi.WALK_LEAF_LEVEL) == (16, 0xFF)
    for name in ("tkv_amq_tree_node", "tkv_amq_tree_segment", "tkv_amq_tree_child"):
        assert re.search(r"typedef struct %s \{" % name, src), name
    assert "tkv_amq_walk.hip" in " ".join(abi._build.SOURCES)


def test_ws_bytes(L):
    ws = L.tkv_amq_walk_paths_ws_bytes
    sizes = [ws(n) for n in (0, 1, 2, 255, 256, 257, 4096, 1 << 20, 25_000_000, 0xffffffff)]
    assert sizes[0] >= 16 and all(a <= b for a, b in zip(sizes, sizes[1:])) and all(s % 16 == 0 for s in sizes)
    # 16 bytes per query (the pivot trail) and a total per 256 queries
    assert ws(25_000_000) >= 16 * 25_000_000 + 8 * (25_000_000 // 256)
    assert ws(25_000_000) <= 17 * 25_000_000
    assert ws(1 << 32) == 0 and ws((1 << 64) - 1) == 0
    import turtle_kv_amd as amq
    assert amq.walk_paths_workspace_bytes(4096) == ws(4096)


# (a bad call is InvalidArgument with or without a device: the arguments are judged first)
def test_invalid_arguments(L, some):
    _, p = some
    good = good_args(p)
    # counts above 0xffffffff
    for name in ("n_nodes", "n_segs", "n_kids", "n_bounds", "n_pk", "n_queries", "capacity"):
        assert call(L, **{**good, name: 1 << 32}, ws_bytes=1 << 40) == abi.INVALID_ARGUMENT, name
    # a null required buffer with a non-zero count
    for name in ("nodes", "segs", "kids", "bounds", "pk", "q", "begin", "leaf", "ws"):
        assert call(L, **{**good, name: None}) == abi.INVALID_ARGUMENT, name
    # a fixed key form with stride 0, on either side (offsets carry no stride)
    assert call(L, pkstride=0, **good) == abi.INVALID_ARGUMENT
    assert call(L, qstride=0, **good) == abi.INVALID_ARGUMENT
    assert call(L, pkstride=0, qstride=0, pkoffs=p, **good) == abi.INVALID_ARGUMENT
    assert call(L, pkstride=0, qstride=0, qoffs=p, **good) == abi.INVALID_ARGUMENT
    # a misaligned node, segment or child array (16 bytes) or d_needed (8 bytes)
    for name in ("nodes", "segs", "kids"):
        for off in (4, 8):
            assert call(L, **{**good, name: p + off}) == abi.INVALID_ARGUMENT, (name, off)
    assert call(L, needed=p + 4, **good) == abi.INVALID_ARGUMENT
    assert call(L, n_queries=0, needed=p + 4) == abi.INVALID_ARGUMENT
    # a short or misaligned workspace
    need = L.tkv_amq_walk_paths_ws_bytes(4)
    assert call(L, ws_bytes=need - 1, **good) == abi.INVALID_ARGUMENT
    assert call(L, ws_bytes=0, **good) == abi.INVALID_ARGUMENT
    assert call(L, **{**good, "ws": p + 8}) == abi.INVALID_ARGUMENT


def test_valid_calls_without_a_device(L, some):
    _, p = some
    good = good_args(p)
    empty = dict(n_nodes=0, n_segs=0, n_kids=0, n_bounds=0, n_pk=0, n_queries=0, capacity=0)
    if L.tkv_amq_device_count() != 0:
        # a device is visible: an empty batch with no outputs is simply OK (tests/test_gpu_walk.py runs the rest)
        assert call(L, **empty) == abi.OK
        return
    assert call(L, **empty) == abi.UNAVAILABLE
    assert call(L, **good) == abi.UNAVAILABLE
    assert call(L, page=p, flushed=p, where=p, needed=p + 8, **good) == abi.UNAVAILABLE
    assert call(L, pkstride=24, qstride=24, **{**good, "pk": p + 8, "q": p + 4}) == abi.UNAVAILABLE
    assert call(L, pkstride=0, pkoffs=p, **good) == abi.UNAVAILABLE
    assert call(L, qstride=0, qoffs=p, **good) == abi.UNAVAILABLE
    # a count of zero needs no buffer
    for name, count in (("nodes", "n_nodes"), ("segs", "n_segs"), ("kids", "n_kids"), ("bounds", "n_bounds"),
                        ("pk", "n_pk"), ("leaf", "capacity")):
        assert call(L, **{**good, name: None, count: 0}) == abi.UNAVAILABLE, name
    import turtle_kv_amd as amq
    with pytest.raises(amq.TkvAmqError) as e:
        amq.walk_paths(amq.TreeIndex.from_description(small_tree()), None)
    assert e.value.status == abi.UNAVAILABLE


# ---------------------------------------------------------------------------------------
# TreeIndex on the host
# ---------------------------------------------------------------------------------------
def key(i):
    return int(i).to_bytes(4, "big") + b"\x00" * 12


def leaf(i):
    return {"leaf": i, "page_id": 1000 + i}


def small_tree():
    """Height 2: a root of 2 pivots with two levels, over a node of 3 leaves and a node of 1."""
    a = {"pivot_keys": [key(0), key(10), key(20), key(30)], "children": [leaf(0), leaf(1), leaf(2)],
         "levels": [[{"leaf": 7, "page_id": 1007, "active": 0b101, "flushed": {0: 5, 2: 9}}]], "page_id": 501}
    b = {"pivot_keys": [key(30), key(99)], "children": [leaf(3)], "levels": [], "page_id": 502}
    return {"pivot_keys": [key(0), key(30), key(99)], "children": [a, b], "page_id": 0,
            "levels": [[{"leaf": 8, "page_id": 1008, "active": 0b11, "flushed": {}},
                        {"leaf": 9, "page_id": 1009, "active": 0b10, "flushed": {1: 77}}],
                       [],
                       [{"leaf": 10, "page_id": 1010, "active": 0b01, "flushed": {}}]]}


def test_tree_index_round_trips_a_description():
    import turtle_kv_amd as amq
    d = small_tree()
    t = amq.TreeIndex.from_description(d)
    assert len(t.nodes) == 3 and len(t.segments) == 4 and len(t.children) == 6
    root = t.nodes[0]
    assert (root["pivot_count"], root["height"], root["level_count"]) == (2, 2, 3)
    assert list(root["level_start"]) == [0, 2, 2, 3, 3, 3, 3, 3]
    assert (root["pivot_key_begin"], root["seg_begin"], root["child_begin"]) == (0, 0, 0)
    assert [int(c["index"]) for c in t.children] == [1, 2, 0, 1, 2, 3]
    assert [int(c["page_id"]) for c in t.children] == [501, 502, 1000, 1001, 1002, 1003]
    assert t.pivot_keys == d["pivot_keys"] + d["children"][0]["pivot_keys"] + d["children"][1]["pivot_keys"]
    # flushed bounds are stored in pivot order behind flushed_begin
    assert list(t.flushed_bounds) == [77, 5, 9]
    assert [int(s["flushed_pivots"]) for s in t.segments] == [0, 0b10, 0, 0b101]
    assert [int(s["flushed_begin"]) for s in t.segments] == [0, 0, 1, 1]
    assert t.describe() == d
    u = amq.TreeIndex.from_description(t.describe())
    for name in ("nodes", "segments", "children", "flushed_bounds"):
        assert getattr(u, name).tobytes() == getattr(t, name).tobytes(), name
    assert u.pivot_keys == t.pivot_keys


def wide_node(n_pivots, levels):
    return {"pivot_keys": [key(i) for i in range(n_pivots + 1)], "children": [leaf(i) for i in range(n_pivots)],
            "levels": levels}


def test_tree_index_keeps_the_packed_node_page_limits():
    import turtle_kv_amd as amq
    seg = {"leaf": 1, "page_id": 1, "active": 1, "flushed": {}}
    # the limits themselves pass
    t = amq.TreeIndex.from_description(wide_node(64, [[seg] * 9] * 7))
    assert t.nodes[0]["pivot_count"] == 64 and t.nodes[0]["level_count"] == 7 and len(t.segments) == 63
    for bad in (wide_node(65, []), wide_node(4, [[seg]] * 8), wide_node(4, [[seg] * 32, [seg] * 32]),
                wide_node(0, [])):
        with pytest.raises(ValueError):
            amq.TreeIndex.from_description(bad)
    # a bit or a flushed bound for a pivot the node does not have; a key too few; mixed children
    with pytest.raises(ValueError):
        amq.TreeIndex.from_description(wide_node(4, [[dict(seg, active=1 << 4)]]))
    with pytest.raises(ValueError):
        amq.TreeIndex.from_description(wide_node(4, [[dict(seg, flushed={4: 1})]]))
    short = wide_node(4, [])
    short["pivot_keys"].pop()
    with pytest.raises(ValueError):
        amq.TreeIndex.from_description(short)
    mixed = wide_node(2, [])
    mixed["children"][1] = wide_node(2, [])
    with pytest.raises(ValueError):
        amq.TreeIndex.from_description(mixed)
