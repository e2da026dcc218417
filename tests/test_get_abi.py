"""tkv_amq_get_keys as far as it goes without a device: the symbol binds, the two records are 16
and 48 bytes with their fields where the header puts them, every InvalidArgument case of
include/tkv_amq.h is judged on host pointers that are never dereferenced, a valid call answers
Unavailable without a GPU, and the ABI version is unchanged.  tests/test_gpu_get.py holds the device
code to a model."""
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


def call(L, kind=0, filters=None, segs=None, n_segs=2, nodes=None, n_nodes=2, tsegs=None, n_tsegs=3, kids=None,
         n_kids=4, bounds=None, n_bounds=2, pk=None, pkoffs=None, pkstride=16, n_pk=5, q=None, qoffs=None, qstride=16,
         n_queries=4, keys=None, koffs=None, kstride=16, n_keys=9, key_begin=None, flags=0, result=None, visits=None,
         metrics=None, counts=None):
    v = ctypes.c_void_p
    return L.tkv_amq_get_keys(kind, v(filters), v(segs), n_segs, v(nodes), n_nodes, v(tsegs), n_tsegs, v(kids), n_kids,
                              v(bounds), n_bounds, v(pk), v(pkoffs), pkstride, n_pk, v(q), v(qoffs), qstride, n_queries,
                              v(keys), v(koffs), kstride, n_keys, v(key_begin), flags, v(result), v(visits), v(metrics),
                              v(counts), None)


def good_args(p):
    return dict(filters=p, segs=p, nodes=p, tsegs=p, kids=p, bounds=p, pk=p, q=p, keys=p, result=p)


def test_symbol_exists_and_binds(L):
    assert "tkv_amq_get_keys" in abi.EXPORTS and hasattr(L, "tkv_amq_get_keys")
    assert L.tkv_amq_get_keys.restype is ctypes.c_int and len(L.tkv_amq_get_keys.argtypes) == 31
    import turtle_kv_amd as amq
    for name in ("get_keys", "get_keys_device", "GetResult", "GetCounts"):
        assert hasattr(amq, name) and name in amq.__all__


def test_record_sizes_and_the_header():
    assert abi.GET_RESULT_DTYPE.itemsize == 16 and abi.GET_COUNTS_DTYPE.itemsize == 48
    assert [abi.GET_RESULT_DTYPE.fields[n][1] for n in ("key_index", "leaf", "where")] == [0, 8, 12]
    assert abi.GET_COUNTS_FIELDS == ("visit_count", "leaf_search_count", "found_count", "absent_count",
                                     "unsearchable_count", "flushed_count")
    with open(os.path.join(abi._build.ROOT, "include", "tkv_amq.h")) as f:
        src = f.read()
    assert "#define TKV_AMQ_ABI_VERSION 3\n" in src
    m = re.search(r"#define TKV_AMQ_GET_CHECK_PAGE_ID (0x[0-9a-f]+)u\b", src)
    assert m and int(m.group(1), 0) == abi.GET_CHECK_PAGE_ID == 1
    for name in ("tkv_amq_get_result", "tkv_amq_get_counts"):
        assert re.search(r"typedef struct %s \{" % name, src), name
    # the counters in the header's order
    body = re.search(r"typedef struct tkv_amq_get_counts \{(.*?)\} tkv_amq_get_counts;", src, re.S).group(1)
    assert tuple(re.findall(r"uint64_t (\w+);", body)) == abi.GET_COUNTS_FIELDS
    body = re.search(r"typedef struct tkv_amq_get_result \{(.*?)\} tkv_amq_get_result;", src, re.S).group(1)
    assert re.findall(r"uint(?:64|32)_t (\w+);", body) == ["key_index", "leaf", "where"]


# (a bad call is InvalidArgument with or without a device: the arguments are judged first)
def test_invalid_arguments(L, some):
    _, p = some
    good = good_args(p)
    assert call(L, kind=2, **good) == abi.INVALID_ARGUMENT
    assert call(L, kind=-1, **good) == abi.INVALID_ARGUMENT
    for flags in (2, 3, 0x80000000):
        assert call(L, flags=flags, **good) == abi.INVALID_ARGUMENT, flags
    # counts above 0xffffffff
    for name in ("n_nodes", "n_tsegs", "n_kids", "n_bounds", "n_pk", "n_queries"):
        assert call(L, **{**good, name: 1 << 32}) == abi.INVALID_ARGUMENT, name
    # a null buffer with a non-zero count
    for name in ("filters", "segs", "nodes", "tsegs", "kids", "bounds", "pk", "q", "keys", "result"):
        assert call(L, **{**good, name: None}) == abi.INVALID_ARGUMENT, name
    # a fixed key form with stride 0, on any of the three key sides (offsets carry no stride)
    for stride in ("pkstride", "qstride", "kstride"):
        assert call(L, **{**good, stride: 0}) == abi.INVALID_ARGUMENT, stride
        others = {"pkstride": "qoffs", "qstride": "koffs", "kstride": "pkoffs"}
        assert call(L, **{**good, stride: 0, others[stride]: p}) == abi.INVALID_ARGUMENT, stride
    # misaligned tree records or d_result (16 bytes), d_metrics or d_counts (8), d_query_visits (4)
    for name in ("nodes", "tsegs", "kids", "result"):
        for off in (4, 8):
            assert call(L, **{**good, name: p + off}) == abi.INVALID_ARGUMENT, (name, off)
    for name in ("metrics", "counts"):
        assert call(L, **{**good, name: p + 4}) == abi.INVALID_ARGUMENT, name
    assert call(L, visits=p + 2, **good) == abi.INVALID_ARGUMENT
    # fixed 16-byte queries that are not 16-byte aligned: the path probe's rule
    assert call(L, **{**good, "q": p + 8}) == abi.INVALID_ARGUMENT
    # and bad arguments of an empty batch are still bad
    assert call(L, n_queries=0, flags=2, **good) == abi.INVALID_ARGUMENT
    assert call(L, n_queries=0, **{**good, "filters": None}) == abi.INVALID_ARGUMENT


def test_valid_calls_without_a_device(L, some):
    _, p = some
    good = good_args(p)
    empty = dict(n_segs=0, n_nodes=0, n_tsegs=0, n_kids=0, n_bounds=0, n_pk=0, n_queries=0, n_keys=0)
    if L.tkv_amq_device_count() != 0:
        # a device is visible: an empty batch is simply OK (tests/test_gpu_get.py runs the rest)
        assert call(L, **empty) == abi.OK
        return
    assert call(L, **empty) == abi.UNAVAILABLE
    assert call(L, **good) == abi.UNAVAILABLE
    assert call(L, kind=1, flags=abi.GET_CHECK_PAGE_ID, visits=p + 4, metrics=p + 8, counts=p + 56, key_begin=p,
                **good) == abi.UNAVAILABLE
    # other key shapes: 24-byte keys at any alignment, offsets on any side
    assert call(L, pkstride=24, qstride=24, kstride=24, **{**good, "pk": p + 8, "q": p + 4, "keys": p + 1}) == \
        abi.UNAVAILABLE
    for stride, offs in (("pkstride", "pkoffs"), ("qstride", "qoffs"), ("kstride", "koffs")):
        assert call(L, **{**good, stride: 0, offs: p}) == abi.UNAVAILABLE, stride
    # misaligned pivot keys or leaf keys only choose the general compare
    assert call(L, **{**good, "pk": p + 4, "keys": p + 4}) == abi.UNAVAILABLE
    # a count of zero needs no buffer
    for name, count in (("nodes", "n_nodes"), ("tsegs", "n_tsegs"), ("kids", "n_kids"), ("bounds", "n_bounds"),
                        ("pk", "n_pk"), ("keys", "n_keys")):
        assert call(L, **{**good, name: None, count: 0}) == abi.UNAVAILABLE, name
    assert call(L, **{**good, "filters": None, "segs": None, "n_segs": 0}) == abi.UNAVAILABLE
    assert call(L, **{**good, "q": None, "result": None, "n_queries": 0}) == abi.UNAVAILABLE
    import turtle_kv_amd as amq
    with pytest.raises(amq.TkvAmqError) as e:
        amq.get_keys(None, None, None, None, None)
    assert e.value.status == abi.UNAVAILABLE
