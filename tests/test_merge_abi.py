"""tkv_amq_merge_leaves and tkv_amq_gather_merged as far as they go without a device: the symbols
bind, the records are 16, 56 and 64 bytes with their fields where the header puts them, the three host
functions' values and monotonicity, every InvalidArgument case of include/tkv_amq.h judged on host
pointers that are never dereferenced, and the answer without a GPU.  tests/test_gpu_merge.py holds the
device code to a merge model."""
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


def run(p, **kw):
    """A run in the fixed forms (16-byte keys, 5-byte values) of 10 items, every pointer `p`."""
    f = dict(keys=p, key_offsets=None, values=p, value_offsets=None, d_begin=p, n_items=10, values_bytes=50,
             key_stride=16, value_stride=5)
    f.update(kw)
    return abi.MergeRun(**f)


def merge(L, p, newer="run", older="run", n_jobs=2, flags=0, begin="p", items="p", capacity=20, needed=None,
          counts=None, ws="p", ws_bytes=None):
    v = ctypes.c_void_p
    pick = lambda x: p if x == "p" else x
    newer, older = (run(p) if r == "run" else r for r in (newer, older))
    if ws_bytes is None:
        ws_bytes = L.tkv_amq_merge_leaves_ws_bytes(min(n_jobs, 0xffffffff), 10, 10)
    ref = lambda r: None if r is None else ctypes.byref(r)
    return L.tkv_amq_merge_leaves(ref(newer), ref(older), n_jobs, flags, v(pick(begin)), v(pick(items)), capacity,
                                  v(needed), v(counts), v(pick(ws)), ws_bytes, None)


def gather(L, p, newer="run", older="run", items="p", begin="p", n_jobs=2, capacity=20, keys="p", key_stride=16,
           koffs=None, k_cap=320, values="p", voffs="p", v_cap=100, needed=None, ws="p", ws_bytes=None):
    v = ctypes.c_void_p
    pick = lambda x: p if x == "p" else x
    newer, older = (run(p) if r == "run" else r for r in (newer, older))
    if ws_bytes is None:
        ws_bytes = L.tkv_amq_gather_merged_ws_bytes(capacity)
    ref = lambda r: None if r is None else ctypes.byref(r)
    return L.tkv_amq_gather_merged(v(pick(items)), v(pick(begin)), n_jobs, capacity, ref(newer), ref(older),
                                   v(pick(keys)), key_stride, v(pick(koffs)), k_cap, v(pick(values)), v(pick(voffs)),
                                   v_cap, v(needed), v(pick(ws)), ws_bytes, None)


def test_symbols_exist_and_bind(L):
    for name in ("tkv_amq_merge_leaves_ws_bytes", "tkv_amq_merge_leaves", "tkv_amq_merge_values_bound",
                 "tkv_amq_gather_merged_ws_bytes", "tkv_amq_gather_merged"):
        assert name in abi.EXPORTS and hasattr(L, name)
    import turtle_kv_amd as amq
    for name in ("merge_leaves", "merge_leaves_device", "gather_merged_device", "MergeResult", "MergeCounts"):
        assert hasattr(amq, name) and name in amq.__all__


def test_record_sizes_and_field_offsets():
    assert abi.MERGE_ITEM_DTYPE.itemsize == 16                    # sizeof(tkv_amq_merge_item)
    assert [abi.MERGE_ITEM_DTYPE.fields[n][1] for n in ("src", "i32", "op", "flags", "reserved")] == [0, 8, 12, 13, 14]
    assert abi.MERGE_COUNTS_DTYPE.itemsize == 56 and abi.MERGE_COUNTS_FIELDS[-1] == "out_count"
    assert ctypes.sizeof(abi.MergeRun) == 64
    assert [getattr(abi.MergeRun, n).offset for n in ("keys", "key_offsets", "values", "value_offsets", "d_begin",
                                                      "n_items", "values_bytes", "key_stride", "value_stride")] == \
        [0, 8, 16, 24, 32, 40, 48, 56, 60]
    assert (abi.MERGE_DECAY_TO_ITEMS, abi.MERGE_SRC_OLDER) == (1, 1 << 63)


def test_header_declares_the_records_and_keeps_the_abi_version():
    with open(os.path.join(abi._build.ROOT, "include", "tkv_amq.h")) as f:
        src = f.read()
    assert re.search(r"#define TKV_AMQ_ABI_VERSION 3\b", src)      # additive: the version stays
    assert re.search(r"#define TKV_AMQ_MERGE_DECAY_TO_ITEMS 0x1u", src)
    item = re.search(r"typedef struct tkv_amq_merge_item \{(.*?)\} tkv_amq_merge_item;", src, re.S).group(1)
    assert re.findall(r"^\s*\w+ (\w+);", item, re.M) == ["src", "i32", "op", "flags", "reserved"]
    counts = re.search(r"typedef struct tkv_amq_merge_counts \{(.*?)\} tkv_amq_merge_counts;", src, re.S).group(1)
    assert tuple(re.findall(r"uint64_t (\w+);", counts)) == abi.MERGE_COUNTS_FIELDS
    fields = re.search(r"typedef struct tkv_amq_merge_run \{(.*?)\} tkv_amq_merge_run;", src, re.S).group(1)
    assert re.findall(r"^\s*(?:const )?\w+\*? (\w+);", fields, re.M) == [n for n, _ in abi.MergeRun._fields_]


def test_host_functions(L):
    ws = L.tkv_amq_merge_leaves_ws_bytes
    assert ws(0, 0, 0) >= 16 and ws(0, 0, 0) % 16 == 0
    grid = (0, 1, 2, 255, 256, 1024, 1025, 100_000, 4096 * 1024, 4096 * 1024 + 1, 6104 * 1024)
    for fixed in grid[:5]:
        for sizes in ([ws(n, fixed, fixed) for n in grid], [ws(fixed, n, fixed) for n in grid],
                      [ws(fixed, fixed, n) for n in grid]):
            assert all(a <= b for a, b in zip(sizes, sizes[1:])) and all(s >= 16 and s % 16 == 0 for s in sizes)
    # two words per item at least: its bound in the other run and its place among the kept
    assert ws(6104, 6104 * 1024, 6104 * 16384) >= 8 * 6104 * (1024 + 16384)
    # counts the call refuses
    assert ws(1 << 32, 0, 0) == 0 and ws(1, 1 << 32, 0) == 0 and ws(1, 0, 1 << 32) == 0
    assert ws(1, 0xffffffff, 1) == 0 and ws(1, 0xfffffffe, 1) > 0 and ws(0xffffffff, 0, 0) > 0
    gws = L.tkv_amq_gather_merged_ws_bytes
    sizes = [gws(n) for n in (0, 1, 1023, 1024, 1025, 1 << 20, 0xffffffff, 1 << 40)]
    assert sizes[0] >= 16 and all(a <= b for a, b in zip(sizes, sizes[1:])) and all(s % 16 == 0 for s in sizes)
    bound = L.tkv_amq_merge_values_bound
    assert bound(0, 0, 0) == 0 and bound(10, 20, 3) == 42 and bound(1 << 33, 1 << 34, 0xffffffff) == \
        (1 << 33) + (1 << 34) + 4 * 0xffffffff
    assert bound(11, 20, 3) > bound(10, 20, 3) < bound(10, 21, 3) and bound(10, 20, 4) > bound(10, 20, 3)


# (a bad call is InvalidArgument with or without a device: the arguments are judged first)
def test_merge_leaves_invalid_arguments(L, some):
    _, p = some
    bad = abi.INVALID_ARGUMENT
    assert merge(L, p, flags=2) == bad and merge(L, p, flags=0x80000001) == bad            # unknown flag bits
    assert merge(L, p, newer=None) == bad and merge(L, p, older=None) == bad
    assert merge(L, p, n_jobs=1 << 32, ws_bytes=1 << 40) == bad
    assert merge(L, p, newer=run(p, n_items=1 << 32), ws_bytes=1 << 40) == bad
    assert merge(L, p, older=run(p, n_items=1 << 32), ws_bytes=1 << 40) == bad
    assert merge(L, p, newer=run(p, n_items=1 << 31), older=run(p, n_items=1 << 31), ws_bytes=1 << 40) == bad
    for side in ("newer", "older"):                                                         # a null required buffer
        assert merge(L, p, **{side: run(p, keys=None)}) == bad, side
        assert merge(L, p, **{side: run(p, values=None)}) == bad, side
        assert merge(L, p, **{side: run(p, d_begin=None)}) == bad, side
        assert merge(L, p, **{side: run(p, key_stride=0)}) == bad, side                     # a fixed form, stride 0
        assert merge(L, p, **{side: run(p, value_stride=0)}) == bad, side
    assert merge(L, p, begin=None) == bad and merge(L, p, items=None) == bad and merge(L, p, ws=None) == bad
    assert merge(L, p, items=p + 8) == bad                                                  # not 16-byte aligned
    assert merge(L, p, needed=p + 4) == bad and merge(L, p, counts=p + 12) == bad           # not 8-byte aligned
    assert merge(L, p, ws=p + 8) == bad
    assert merge(L, p, ws_bytes=L.tkv_amq_merge_leaves_ws_bytes(2, 10, 10) - 1) == bad and merge(L, p, ws_bytes=0) == bad


def test_gather_merged_invalid_arguments(L, some):
    _, p = some
    bad = abi.INVALID_ARGUMENT
    assert gather(L, p, newer=None) == bad and gather(L, p, older=None) == bad
    assert gather(L, p, begin=None) == bad and gather(L, p, voffs=None) == bad and gather(L, p, ws=None) == bad
    assert gather(L, p, n_jobs=1 << 32) == bad
    assert gather(L, p, newer=run(p, n_items=1 << 32)) == bad
    assert gather(L, p, newer=run(p, n_items=1 << 31), older=run(p, n_items=1 << 31)) == bad
    for side in ("newer", "older"):
        assert gather(L, p, **{side: run(p, keys=None)}) == bad, side
        assert gather(L, p, **{side: run(p, values=None)}) == bad, side
        assert gather(L, p, **{side: run(p, key_stride=0)}) == bad, side
        assert gather(L, p, **{side: run(p, value_stride=0)}) == bad, side
        # the fixed key form only when both runs are fixed with that stride
        assert gather(L, p, **{side: run(p, key_offsets=p, key_stride=0)}) == bad, side
        assert gather(L, p, **{side: run(p, key_stride=24)}) == bad, side
    assert gather(L, p, key_stride=24) == bad
    assert gather(L, p, key_stride=0, koffs=None) == bad                                    # the offsets form needs them
    assert gather(L, p, items=None) == bad and gather(L, p, items=p + 8) == bad
    assert gather(L, p, keys=None) == bad and gather(L, p, values=None) == bad              # with a capacity > 0
    assert gather(L, p, key_stride=0, koffs=p + 4) == bad and gather(L, p, voffs=p + 4) == bad
    assert gather(L, p, needed=p + 4) == bad and gather(L, p, ws=p + 8) == bad
    assert gather(L, p, ws_bytes=L.tkv_amq_gather_merged_ws_bytes(20) - 1) == bad


def test_valid_calls_without_a_device(L, some):
    _, p = some
    if L.tkv_amq_device_count() != 0:
        return                                                    # (tests/test_gpu_merge.py runs them)
    un = abi.UNAVAILABLE
    assert merge(L, p) == un and merge(L, p, flags=abi.MERGE_DECAY_TO_ITEMS, needed=p + 8, counts=p + 16) == un
    assert merge(L, p, newer=run(p, key_offsets=p, key_stride=0, value_offsets=p, value_stride=0)) == un
    assert merge(L, p, newer=run(p, keys=p + 3, key_stride=11), older=run(p, keys=p + 5, key_stride=24)) == un
    # a count of zero needs no buffer
    assert merge(L, p, newer=run(p, keys=None, values=None, n_items=0)) == un
    assert merge(L, p, older=run(p, values=None, values_bytes=0)) == un
    assert merge(L, p, items=None, capacity=0) == un
    assert merge(L, p, n_jobs=0, ws=None, ws_bytes=0, newer=run(p, d_begin=None), older=run(p, d_begin=None)) == un
    assert gather(L, p) == un and gather(L, p, key_stride=0, koffs=p, needed=p + 8) == un
    assert gather(L, p, newer=run(p, key_offsets=p, key_stride=0), key_stride=0, koffs=p) == un
    assert gather(L, p, keys=None, k_cap=0, values=None, v_cap=0) == un
    assert gather(L, p, items=None, capacity=0) == un
    import turtle_kv_amd as amq
    with pytest.raises(amq.TkvAmqError) as e:
        amq.merge_leaves(None, None, [0], None, None, [0])
    assert e.value.status == un
    with pytest.raises(amq.TkvAmqError) as e:
        amq.merge_leaves_device(run(p), run(p), 2, None, None, 0, None)
    assert e.value.status == un
