"""tkv_amq_find_keys as far as it goes without a device: the symbol binds, the records are 16 and
32 bytes with their fields where the header puts them, the constants, every InvalidArgument case
of include/tkv_amq.h judged on host pointers that are never dereferenced, and the answer without
a GPU.  tests/test_gpu_find.py holds the device code to a dict-lookup model."""
import ctypes

import numpy as np
import pytest

from turtle_kv_amd import abi

BLOOM, VQF = 0, 1


class FindResult(ctypes.Structure):
    """tkv_amq_find_result as the header declares it."""
    _fields_ = [("key_index", ctypes.c_uint64), ("leaf", ctypes.c_uint32), ("cand", ctypes.c_uint32)]


class FindCounts(ctypes.Structure):
    """tkv_amq_find_counts as the header declares it."""
    _fields_ = [(n, ctypes.c_uint64) for n in ("leaf_search_count", "found_count", "absent_count",
                                               "unsearchable_count")]


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


def call(L, kind=BLOOM, filters=None, segs=None, n_segs=1, queries=None, qoffs=None, qstride=16, n_queries=4,
         cand_begin=None, cand_leaf=None, cand_entry=None, n_cand=4, leaf_keys=None, koffs=None, kstride=16,
         n_leaf_keys=8, key_begin=None, flags=0, result=None, state=None, opts=None, counts=None):
    v = ctypes.c_void_p
    return L.tkv_amq_find_keys(kind, v(filters), v(segs), n_segs, v(queries), v(qoffs), qstride, n_queries,
                               v(cand_begin), v(cand_leaf), v(cand_entry), n_cand, v(leaf_keys), v(koffs),
                               kstride, n_leaf_keys, v(key_begin), flags, v(result), v(state),
                               None if opts is None else ctypes.byref(opts), v(counts), None)


def test_symbols_exist_and_bind(L):
    assert "tkv_amq_find_keys" in abi.EXPORTS and hasattr(L, "tkv_amq_find_keys")
    assert L.tkv_amq_find_keys.restype is ctypes.c_int and len(L.tkv_amq_find_keys.argtypes) == 23
    assert ctypes.sizeof(FindResult) == 16 == abi.FIND_RESULT_DTYPE.itemsize
    assert [abi.FIND_RESULT_DTYPE.fields[n][1] for n in ("key_index", "leaf", "cand")] == [0, 8, 12]
    assert [getattr(FindResult, n).offset for n in ("key_index", "leaf", "cand")] == [0, 8, 12]
    assert ctypes.sizeof(FindCounts) == 32 == abi.FIND_COUNTS_DTYPE.itemsize
    assert [abi.FIND_COUNTS_DTYPE.fields[n][1] for n in ("leaf_search_count", "found_count", "absent_count",
                                                         "unsearchable_count")] == [0, 8, 16, 24]
    assert abi.FIND_ALL == 1
    assert (abi.CAND_ABSENT, abi.CAND_FOUND, abi.CAND_NOT_SEARCHED, abi.CAND_UNSEARCHABLE) == (0, 1, 2, 3)
    import turtle_kv_amd as amq
    for name in ("find_keys", "find_keys_device"):
        assert hasattr(amq, name) and name in amq.__all__


def test_header_constants_and_abi_version():
    import os
    import re
    with open(os.path.join(abi._build.ROOT, "include", "tkv_amq.h")) as f:
        src = f.read()
    assert "#define TKV_AMQ_ABI_VERSION 3\n" in src
    want = {"TKV_AMQ_FIND_ALL": 1, "TKV_AMQ_CAND_ABSENT": 0, "TKV_AMQ_CAND_FOUND": 1,
            "TKV_AMQ_CAND_NOT_SEARCHED": 2, "TKV_AMQ_CAND_UNSEARCHABLE": 3}
    for name, value in want.items():
        m = re.search(r"#define %s (0x[0-9a-f]+|\d+)u\b" % name, src)
        assert m and int(m.group(1), 0) == value, name


# (a bad call is InvalidArgument with or without a device: the arguments are judged first)
def test_invalid_arguments(L, some):
    _, p = some
    good = dict(segs=p, queries=p, cand_begin=p, cand_leaf=p, leaf_keys=p, result=p)
    # unknown kind, with and without work
    assert call(L, kind=2, **good) == abi.INVALID_ARGUMENT
    assert call(L, kind=-1, n_segs=0, n_queries=0, n_cand=0, n_leaf_keys=0) == abi.INVALID_ARGUMENT
    # unknown flag bits
    for flags in (2, 3, 0x80000000):
        assert call(L, flags=flags, **good) == abi.INVALID_ARGUMENT, flags
    # n_queries or n_cand above 0xffffffff
    assert call(L, n_queries=1 << 32, **good) == abi.INVALID_ARGUMENT
    assert call(L, n_cand=1 << 32, **good) == abi.INVALID_ARGUMENT
    # a null required buffer with a non-zero count
    for name in ("cand_begin", "result", "queries", "cand_leaf", "segs", "leaf_keys"):
        assert call(L, **{**good, name: None}) == abi.INVALID_ARGUMENT, name
        assert call(L, kind=VQF, **{**good, name: None}) == abi.INVALID_ARGUMENT, name
    # a fixed form with stride 0, on either side (offsets carry no stride)
    assert call(L, qstride=0, **good) == abi.INVALID_ARGUMENT
    assert call(L, kstride=0, **good) == abi.INVALID_ARGUMENT
    assert call(L, qstride=0, kstride=0, qoffs=p, **good) == abi.INVALID_ARGUMENT
    # d_query_page_id without d_cand_entry or without d_filters
    opts = abi.ProbeOpts(p, None, None)
    assert call(L, opts=opts, filters=p, **good) == abi.INVALID_ARGUMENT
    assert call(L, opts=opts, cand_entry=p, **good) == abi.INVALID_ARGUMENT
    assert call(L, opts=opts, **good) == abi.INVALID_ARGUMENT
    # d_result not 16-byte aligned, d_counts not 8-byte aligned
    assert call(L, **{**good, "result": p + 8}) == abi.INVALID_ARGUMENT
    assert call(L, counts=p + 4, **good) == abi.INVALID_ARGUMENT
    assert call(L, n_queries=0, n_cand=0, result=p + 8) == abi.INVALID_ARGUMENT
    assert call(L, n_queries=0, n_cand=0, counts=p + 4) == abi.INVALID_ARGUMENT


def test_valid_calls_without_a_device(L, some):
    _, p = some
    good = dict(segs=p, queries=p, cand_begin=p, cand_leaf=p, leaf_keys=p, result=p)
    if L.tkv_amq_device_count() != 0:
        # a device is visible: an empty batch is simply OK (tests/test_gpu_find.py runs the rest)
        assert call(L, n_segs=0, n_queries=0, n_cand=0, n_leaf_keys=0) == abi.OK
        return
    # an empty call with null buffers is judged before the device is looked for
    assert call(L, n_segs=0, n_queries=0, n_cand=0, n_leaf_keys=0) == abi.UNAVAILABLE
    # valid calls: either kind, each key form on each side, with and without the optional buffers
    assert call(L, **good) == abi.UNAVAILABLE
    assert call(L, kind=VQF, flags=abi.FIND_ALL, **good) == abi.UNAVAILABLE
    assert call(L, qstride=24, kstride=24, **{**good, "queries": p + 8, "leaf_keys": p + 4}) == abi.UNAVAILABLE
    assert call(L, qstride=0, qoffs=p, **good) == abi.UNAVAILABLE
    assert call(L, kstride=0, koffs=p, **good) == abi.UNAVAILABLE
    assert call(L, key_begin=p, state=p, counts=p + 8, cand_entry=p, **good) == abi.UNAVAILABLE
    assert call(L, n_leaf_keys=0, **{**good, "leaf_keys": None}) == abi.UNAVAILABLE
    assert call(L, n_cand=0, **{**good, "cand_leaf": None}) == abi.UNAVAILABLE
    assert call(L, n_segs=0, **{**good, "segs": None}) == abi.UNAVAILABLE
    # metrics alone need no filter bytes; page ids need them and the entries
    assert call(L, opts=abi.ProbeOpts(None, None, p), **good) == abi.UNAVAILABLE
    assert call(L, opts=abi.ProbeOpts(p, p, p), filters=p, cand_entry=p, **good) == abi.UNAVAILABLE
    import turtle_kv_amd as amq
    with pytest.raises(amq.TkvAmqError) as e:
        amq.find_keys(amq.plan_filters(amq.BLOOM, [100], 10), None, None, None, None)
    assert e.value.status == abi.UNAVAILABLE


def test_dtype_round_trip():
    raw = np.zeros(2, dtype=abi.FIND_RESULT_DTYPE)
    raw["key_index"] = [abi.NOT_FOUND, 5]
    raw["leaf"] = [abi.NO_LEAF, 3]
    raw["cand"] = [abi.NO_LEAF, 9]
    r = (FindResult * 2).from_buffer_copy(raw.tobytes())
    assert (r[0].key_index, r[0].leaf, r[0].cand) == (2**64 - 1, 2**32 - 1, 2**32 - 1)
    assert (r[1].key_index, r[1].leaf, r[1].cand) == (5, 3, 9)
    c = np.zeros(1, dtype=abi.FIND_COUNTS_DTYPE)
    c["absent_count"] = 7
    assert FindCounts.from_buffer_copy(c.tobytes()).absent_count == 7
