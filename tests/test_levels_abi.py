"""tkv_amq_merge_levels and tkv_amq_gather_levels as far as they go without a device: the symbols bind,
the header declares them and keeps the ABI version and the records' sizes, the three host functions'
values and monotonicity, every InvalidArgument case of include/tkv_amq.h judged on host pointers that are
never dereferenced, and the answer without a GPU.  tests/test_gpu_levels.py holds the device code to a
merge model."""
import ctypes
import os
import re

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


def table(p, n_runs=3, changed=None):
    """n_runs runs; changed: {index: run}."""
    return [(changed or {}).get(s, run(p)) for s in range(n_runs)]


def array(runs):
    return None if runs is None else (abi.MergeRun * max(len(runs), 1))(*runs)


def merge(L, p, runs="table", n_runs=None, n_jobs=2, flags=0, begin="p", items="p", capacity=30, needed=None,
          counts=None, ws="p", ws_bytes=None):
    v = ctypes.c_void_p
    pick = lambda x: p if x == "p" else x
    runs = table(p) if runs == "table" else runs
    n_runs = (0 if runs is None else len(runs)) if n_runs is None else n_runs
    if ws_bytes is None:
        ws_bytes = L.tkv_amq_merge_levels_ws_bytes(min(n_jobs, 0xffffffff), max(1, min(n_runs, 8)), 80) or 1 << 20
    return L.tkv_amq_merge_levels(array(runs), n_runs, n_jobs, flags, v(pick(begin)), v(pick(items)), capacity,
                                  v(needed), v(counts), v(pick(ws)), ws_bytes, None)


def gather(L, p, runs="table", n_runs=None, items="p", begin="p", n_jobs=2, capacity=30, keys="p", key_stride=16,
           koffs=None, k_cap=480, values="p", voffs="p", v_cap=150, needed=None, ws="p", ws_bytes=None):
    v = ctypes.c_void_p
    pick = lambda x: p if x == "p" else x
    runs = table(p) if runs == "table" else runs
    n_runs = (0 if runs is None else len(runs)) if n_runs is None else n_runs
    if ws_bytes is None:
        ws_bytes = L.tkv_amq_gather_levels_ws_bytes(capacity)
    return L.tkv_amq_gather_levels(v(pick(items)), v(pick(begin)), n_jobs, capacity, array(runs), n_runs, v(pick(keys)),
                                   key_stride, v(pick(koffs)), k_cap, v(pick(values)), v(pick(voffs)), v_cap, v(needed),
                                   v(pick(ws)), ws_bytes, None)


def test_symbols_exist_and_bind(L):
    for name in ("tkv_amq_merge_levels_ws_bytes", "tkv_amq_merge_levels", "tkv_amq_merge_levels_values_bound",
                 "tkv_amq_gather_levels_ws_bytes", "tkv_amq_gather_levels"):
        assert name in abi.EXPORTS and hasattr(L, name)
    import turtle_kv_amd as amq
    for name in ("merge_levels", "merge_levels_device", "gather_levels_device", "merge_levels_workspace_bytes",
                 "gather_levels_workspace_bytes", "merge_levels_values_bound"):
        assert hasattr(amq, name) and name in amq.__all__
    assert (abi.MERGE_MAX_RUNS, abi.LEVELS_SRC_SHIFT) == (8, 56)


def test_header_declares_the_new_names_and_keeps_the_abi_version_and_the_sizes():
    with open(os.path.join(abi._build.ROOT, "include", "tkv_amq.h")) as f:
        src = f.read()
    assert re.search(r"#define TKV_AMQ_ABI_VERSION 3\b", src)      # additive: the version stays
    assert re.search(r"#define TKV_AMQ_MERGE_MAX_RUNS 8u", src) and re.search(r"#define TKV_AMQ_LEVELS_SRC_SHIFT 56\b", src)
    for name in ("tkv_amq_merge_levels_ws_bytes", "tkv_amq_merge_levels", "tkv_amq_merge_levels_values_bound",
                 "tkv_amq_gather_levels_ws_bytes", "tkv_amq_gather_levels"):
        assert re.search(r"^(?:int|uint64_t) %s\(" % name, src, re.M), name
    assert re.search(r"int tkv_amq_merge_levels\(const tkv_amq_merge_run\* runs, uint32_t n_runs, uint64_t n_jobs", src)
    assert "merge_compact_edits over K levels" in src and "InMemoryNode::push_levels_to_merge" in src
    # the structs are the leaf merge's, unchanged
    assert "/* 64 bytes; a host struct" in src and "typedef struct tkv_amq_merge_item { /* 16 bytes */" in src
    assert "typedef struct tkv_amq_merge_counts { /* 56 bytes" in src
    assert ctypes.sizeof(abi.MergeRun) == 64 and abi.MERGE_ITEM_DTYPE.itemsize == 16
    assert abi.MERGE_COUNTS_DTYPE.itemsize == 56


def test_host_functions(L):
    ws = L.tkv_amq_merge_levels_ws_bytes
    assert ws(0, 1, 0) >= 16 and ws(0, 1, 0) % 16 == 0
    grid = (0, 1, 2, 255, 256, 1024, 1025, 100_000, 4096 * 1024, 4096 * 1024 + 1, 6104 * 1024)
    for fixed in grid[:5]:
        for k in range(1, 9):
            for sizes in ([ws(n, k, fixed) for n in grid], [ws(fixed, k, n) for n in grid]):
                assert all(a <= b for a, b in zip(sizes, sizes[1:])) and all(s >= 16 and s % 16 == 0 for s in sizes)
        for n in grid:
            sizes = [ws(fixed, k, n) for k in range(1, 9)] + [ws(n, k, fixed) for k in range(1, 9)]
            assert all(a <= b for a, b in zip(sizes[:8], sizes[1:8])) and all(a <= b for a, b in zip(sizes[8:], sizes[9:]))
    # per item its bound in every other run, its place among the kept and its folded integer
    assert ws(6104, 4, 6104 * 23552) >= 4 * (3 + 2) * 6104 * 23552
    # counts the call refuses
    assert ws(1, 0, 1) == 0 and ws(1, 9, 1) == 0 and ws(1, 1 << 31, 1) == 0
    assert ws(1 << 32, 2, 0) == 0 and ws(1, 2, 1 << 32) == 0
    assert ws(0xffffffff, 8, 0) > 0 and ws(1, 8, 0xffffffff) > 0
    gws = L.tkv_amq_gather_levels_ws_bytes
    sizes = [gws(n) for n in (0, 1, 1023, 1024, 1025, 1 << 20, 0xffffffff, 1 << 40)]
    assert sizes[0] >= 16 and all(a <= b for a, b in zip(sizes, sizes[1:])) and all(s % 16 == 0 for s in sizes)
    assert sizes == [L.tkv_amq_gather_merged_ws_bytes(n) for n in (0, 1, 1023, 1024, 1025, 1 << 20, 0xffffffff, 1 << 40)]
    bound = L.tkv_amq_merge_levels_values_bound
    assert bound(0, 0) == 0 and bound(30, 3) == 42 and bound(1 << 35, 0xffffffff) == (1 << 35) + 4 * 0xffffffff
    assert bound(31, 3) > bound(30, 3) < bound(30, 4)
    # two runs: the leaf merge's bound
    assert bound(10 + 20, 3) == L.tkv_amq_merge_values_bound(10, 20, 3)


# (a bad call is InvalidArgument with or without a device: the arguments are judged first)
def test_merge_levels_invalid_arguments(L, some):
    _, p = some
    bad = abi.INVALID_ARGUMENT
    assert merge(L, p, n_runs=0) == bad and merge(L, p, runs=table(p, 9)) == bad and merge(L, p, n_runs=1 << 31) == bad
    assert merge(L, p, runs=None, n_runs=3) == bad
    assert merge(L, p, flags=2) == bad and merge(L, p, flags=0x80000001) == bad            # unknown flag bits
    assert merge(L, p, n_jobs=1 << 32, ws_bytes=1 << 40) == bad
    for n_runs in (1, 2, 3, 8):
        for s in sorted({0, n_runs // 2, n_runs - 1}):                                      # every run is checked
            one = lambda **kw: merge(L, p, runs=table(p, n_runs, {s: run(p, **kw)}), ws_bytes=1 << 40)
            assert one(n_items=1 << 32) == bad, (n_runs, s)
            assert one(keys=None) == bad and one(values=None) == bad and one(d_begin=None) == bad, (n_runs, s)
            assert one(key_stride=0) == bad and one(value_stride=0) == bad, (n_runs, s)     # a fixed form, stride 0
    # the items in all
    assert merge(L, p, runs=table(p, 2, {0: run(p, n_items=1 << 31), 1: run(p, n_items=1 << 31)}), ws_bytes=1 << 40) == bad
    assert merge(L, p, runs=[run(p, n_items=1 << 29)] * 8, ws_bytes=1 << 40) == bad
    assert merge(L, p, begin=None) == bad and merge(L, p, items=None) == bad and merge(L, p, ws=None) == bad
    assert merge(L, p, items=p + 8) == bad and merge(L, p, begin=p + 4) == bad              # alignment
    assert merge(L, p, needed=p + 4) == bad and merge(L, p, counts=p + 12) == bad
    assert merge(L, p, ws=p + 8) == bad
    assert merge(L, p, ws_bytes=L.tkv_amq_merge_levels_ws_bytes(2, 3, 30) - 1) == bad and merge(L, p, ws_bytes=0) == bad


def test_gather_levels_invalid_arguments(L, some):
    _, p = some
    bad = abi.INVALID_ARGUMENT
    assert gather(L, p, n_runs=0) == bad and gather(L, p, runs=table(p, 9)) == bad and gather(L, p, runs=None, n_runs=2) == bad
    assert gather(L, p, begin=None) == bad and gather(L, p, voffs=None) == bad and gather(L, p, ws=None) == bad
    assert gather(L, p, n_jobs=1 << 32) == bad
    assert gather(L, p, runs=[run(p, n_items=1 << 29)] * 8) == bad
    for s in range(3):
        one = lambda **kw: gather(L, p, runs=table(p, 3, {s: run(p, **kw)}))
        assert one(n_items=1 << 32) == bad and one(keys=None) == bad and one(values=None) == bad, s
        assert one(key_stride=0) == bad and one(value_stride=0) == bad, s
        # the fixed key form only when every run is fixed with that stride
        assert one(key_offsets=p, key_stride=0) == bad and one(key_stride=24) == bad, s
    assert gather(L, p, key_stride=24) == bad
    assert gather(L, p, key_stride=0, koffs=None) == bad                                    # the offsets form needs them
    assert gather(L, p, items=None) == bad and gather(L, p, items=p + 8) == bad
    assert gather(L, p, keys=None) == bad and gather(L, p, values=None) == bad              # with a capacity > 0
    assert gather(L, p, key_stride=0, koffs=p + 4) == bad and gather(L, p, voffs=p + 4) == bad
    assert gather(L, p, needed=p + 4) == bad and gather(L, p, ws=p + 8) == bad
    assert gather(L, p, ws_bytes=L.tkv_amq_gather_levels_ws_bytes(30) - 1) == bad


def test_valid_calls_without_a_device(L, some):
    _, p = some
    if L.tkv_amq_device_count() != 0:
        return                                                    # (tests/test_gpu_levels.py runs them)
    un = abi.UNAVAILABLE
    for n_runs in range(1, 9):
        assert merge(L, p, runs=table(p, n_runs)) == un and gather(L, p, runs=table(p, n_runs)) == un, n_runs
    assert merge(L, p, flags=abi.MERGE_DECAY_TO_ITEMS, needed=p + 8, counts=p + 16) == un
    assert merge(L, p, runs=table(p, 3, {1: run(p, key_offsets=p, key_stride=0, value_offsets=p, value_stride=0)})) == un
    assert merge(L, p, runs=table(p, 3, {0: run(p, keys=p + 3, key_stride=11), 2: run(p, keys=p + 5, key_stride=24)})) == un
    # a count of zero needs no buffer
    assert merge(L, p, runs=table(p, 3, {1: run(p, keys=None, values=None, n_items=0)})) == un
    assert merge(L, p, runs=table(p, 3, {2: run(p, values=None, values_bytes=0)})) == un
    assert merge(L, p, items=None, capacity=0) == un
    assert merge(L, p, n_jobs=0, ws=None, ws_bytes=0, runs=[run(p, d_begin=None)] * 4) == un
    assert gather(L, p, key_stride=0, koffs=p, needed=p + 8) == un
    assert gather(L, p, runs=table(p, 3, {1: run(p, key_offsets=p, key_stride=0)}), key_stride=0, koffs=p) == un
    assert gather(L, p, keys=None, k_cap=0, values=None, v_cap=0) == un
    assert gather(L, p, items=None, capacity=0) == un
    import turtle_kv_amd as amq
    with pytest.raises(amq.TkvAmqError) as e:
        amq.merge_levels([(None, None, [0])] * 3)
    assert e.value.status == un
    with pytest.raises(amq.TkvAmqError) as e:
        amq.merge_levels_device([run(p)] * 3, 2, None, None, 0, None)
    assert e.value.status == un
