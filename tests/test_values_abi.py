"""tkv_amq_get_values and tkv_amq_gather_values as far as they go without a device: the symbols
bind, the two records are 32 and 64 bytes with their fields where the header puts them, the op and
flag constants are the header's, every InvalidArgument case of include/tkv_amq.h is judged on host
pointers that are never dereferenced, a valid call answers Unavailable without a GPU, and the ABI
version is unchanged.  tests/test_gpu_values.py holds the device code to a model."""
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
         n_queries=4, keys=None, koffs=None, kstride=16, n_keys=9, key_begin=None, values=None, voffs=None, vstride=5,
         vbytes=45, flags=0, result=None, visits=None, metrics=None, counts=None):
    v = ctypes.c_void_p
    return L.tkv_amq_get_values(kind, v(filters), v(segs), n_segs, v(nodes), n_nodes, v(tsegs), n_tsegs, v(kids),
                                n_kids, v(bounds), n_bounds, v(pk), v(pkoffs), pkstride, n_pk, v(q), v(qoffs), qstride,
                                n_queries, v(keys), v(koffs), kstride, n_keys, v(key_begin), v(values), v(voffs),
                                vstride, vbytes, flags, v(result), v(visits), v(metrics), v(counts), None)


def gather(L, result=None, n_queries=4, values=None, voffs=None, vstride=5, vbytes=45, n_keys=9, out=None,
           out_stride=8, lens=None):
    v = ctypes.c_void_p
    return L.tkv_amq_gather_values(v(result), n_queries, v(values), v(voffs), vstride, vbytes, n_keys, v(out),
                                   out_stride, v(lens), None)


def good_args(p):
    return dict(filters=p, segs=p, nodes=p, tsegs=p, kids=p, bounds=p, pk=p, q=p, keys=p, values=p, result=p)


def test_symbols_exist_and_bind(L):
    for name, n_args in (("tkv_amq_get_values", 35), ("tkv_amq_gather_values", 11)):
        assert name in abi.EXPORTS and hasattr(L, name), name
        fn = getattr(L, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == n_args, name
    import turtle_kv_amd as amq
    for name in ("get_values", "get_values_device", "gather_values_device", "ValueResult", "ValueCounts"):
        assert hasattr(amq, name) and name in amq.__all__, name


def test_record_sizes_and_the_header():
    assert abi.VALUE_RESULT_DTYPE.itemsize == 32 and abi.VALUE_COUNTS_DTYPE.itemsize == 64
    names = ("key_index", "last_index", "leaf", "where", "i32", "op", "flags", "n_items")
    assert abi.VALUE_RESULT_DTYPE.names == names
    assert [abi.VALUE_RESULT_DTYPE.fields[n][1] for n in names] == [0, 8, 16, 20, 24, 28, 29, 30]
    assert abi.VALUE_RESULT_DTYPE["i32"] == "<i4" and abi.VALUE_RESULT_DTYPE["n_items"] == "<u2"
    assert abi.VALUE_COUNTS_FIELDS == abi.GET_COUNTS_FIELDS + ("item_count", "bad_combine_count")
    with open(os.path.join(abi._build.ROOT, "include", "tkv_amq.h")) as f:
        src = f.read()
    assert "#define TKV_AMQ_ABI_VERSION 3\n" in src
    body = re.search(r"typedef struct tkv_amq_value_counts \{(.*?)\} tkv_amq_value_counts;", src, re.S).group(1)
    assert tuple(re.findall(r"uint64_t (\w+);", body)) == abi.VALUE_COUNTS_FIELDS
    body = re.search(r"typedef struct tkv_amq_value_result \{(.*?)\} tkv_amq_value_result;", src, re.S).group(1)
    fields = re.findall(r"(u?int(?:64|32|16|8)_t) (\w+);", body)
    assert [f[1] for f in fields] == list(names)
    assert [f[0] for f in fields] == ["uint64_t", "uint64_t", "uint32_t", "uint32_t", "int32_t", "uint8_t", "uint8_t",
                                      "uint16_t"]
    # the ops are the reference's (core/value_view.hpp:27-33), the flags two bits
    want = {"OP_DELETE": 0, "OP_NOOP": 1, "OP_WRITE": 2, "OP_ADD_I32": 3, "OP_PAGE_SLICE": 4, "OP_NONE": 0xFF,
            "VALUE_COMBINED": 1, "VALUE_BAD_COMBINE": 2}
    for name, value in want.items():
        m = re.search(r"#define TKV_AMQ_%s (0x[0-9a-f]+|\d+)u\b" % name, src)
        assert m and int(m.group(1), 0) == value == getattr(abi, name), name


# (a bad call is InvalidArgument with or without a device: the arguments are judged first)
def test_get_values_refuses_what_get_keys_refuses(L, some):
    _, p = some
    good = good_args(p)
    assert call(L, kind=2, **good) == abi.INVALID_ARGUMENT
    assert call(L, kind=-1, **good) == abi.INVALID_ARGUMENT
    for flags in (2, 3, 0x80000000):
        assert call(L, flags=flags, **good) == abi.INVALID_ARGUMENT, flags
    for name in ("n_nodes", "n_tsegs", "n_kids", "n_bounds", "n_pk", "n_queries"):
        assert call(L, **{**good, name: 1 << 32}) == abi.INVALID_ARGUMENT, name
    for name in ("filters", "segs", "nodes", "tsegs", "kids", "bounds", "pk", "q", "keys", "result"):
        assert call(L, **{**good, name: None}) == abi.INVALID_ARGUMENT, name
    for stride in ("pkstride", "qstride", "kstride"):
        assert call(L, **{**good, stride: 0}) == abi.INVALID_ARGUMENT, stride
    for name in ("nodes", "tsegs", "kids"):
        for off in (4, 8):
            assert call(L, **{**good, name: p + off}) == abi.INVALID_ARGUMENT, (name, off)
    for name in ("metrics", "counts"):
        assert call(L, **{**good, name: p + 4}) == abi.INVALID_ARGUMENT, name
    assert call(L, visits=p + 2, **good) == abi.INVALID_ARGUMENT
    assert call(L, **{**good, "q": p + 8}) == abi.INVALID_ARGUMENT
    assert call(L, n_queries=0, flags=2, **good) == abi.INVALID_ARGUMENT


def test_get_values_own_invalid_arguments(L, some):
    _, p = some
    good = good_args(p)
    # d_result not 16-byte aligned
    for off in (4, 8):
        assert call(L, **{**good, "result": p + off}) == abi.INVALID_ARGUMENT, off
    # null leaf_values with keys and bytes to read
    assert call(L, **{**good, "values": None}) == abi.INVALID_ARGUMENT
    assert call(L, **{**good, "values": None, "voffs": p}) == abi.INVALID_ARGUMENT
    # the fixed form with stride 0 while there are keys
    assert call(L, **{**good, "vstride": 0}) == abi.INVALID_ARGUMENT
    # ... and both of an empty batch
    assert call(L, n_queries=0, **{**good, "values": None}) == abi.INVALID_ARGUMENT
    assert call(L, n_queries=0, **{**good, "vstride": 0}) == abi.INVALID_ARGUMENT


def test_gather_invalid_arguments(L, some):
    _, p = some
    good = dict(result=p, values=p, out=p, lens=p)
    assert gather(L, **{**good, "n_queries": 1 << 32}) == abi.INVALID_ARGUMENT
    for name in ("result", "lens", "out", "values"):
        assert gather(L, **{**good, name: None}) == abi.INVALID_ARGUMENT, name
    for off in (4, 8):
        assert gather(L, **{**good, "result": p + off}) == abi.INVALID_ARGUMENT, off
    assert gather(L, **{**good, "lens": p + 2}) == abi.INVALID_ARGUMENT
    assert gather(L, **{**good, "vstride": 0}) == abi.INVALID_ARGUMENT
    assert gather(L, n_queries=0, **{**good, "vstride": 0}) == abi.INVALID_ARGUMENT


def test_valid_calls_without_a_device(L, some):
    _, p = some
    good = good_args(p)
    empty = dict(n_segs=0, n_nodes=0, n_tsegs=0, n_kids=0, n_bounds=0, n_pk=0, n_queries=0, n_keys=0, vbytes=0)
    if L.tkv_amq_device_count() != 0:
        # a device is visible: an empty batch is simply OK (tests/test_gpu_values.py runs the rest)
        assert call(L, **empty) == abi.OK
        assert gather(L, n_queries=0, n_keys=0, vbytes=0) == abi.OK
        return
    assert call(L, **empty) == abi.UNAVAILABLE
    assert call(L, **good) == abi.UNAVAILABLE
    assert call(L, kind=1, flags=abi.GET_CHECK_PAGE_ID, visits=p + 4, metrics=p + 8, counts=p + 72, key_begin=p,
                **good) == abi.UNAVAILABLE
    # values at any byte address, in either form; a stride of 0 beside offsets
    assert call(L, **{**good, "values": p + 3}) == abi.UNAVAILABLE
    assert call(L, **{**good, "voffs": p, "vstride": 0}) == abi.UNAVAILABLE
    # no bytes or no keys need no buffer
    assert call(L, **{**good, "values": None, "vbytes": 0}) == abi.UNAVAILABLE
    assert call(L, **{**good, "values": None, "keys": None, "n_keys": 0, "vstride": 0}) == abi.UNAVAILABLE
    assert call(L, **{**good, "q": None, "result": None, "n_queries": 0}) == abi.UNAVAILABLE
    gg = dict(result=p, values=p, out=p, lens=p)
    assert gather(L, **gg) == abi.UNAVAILABLE
    assert gather(L, **{**gg, "values": p + 1, "out": p + 3, "out_stride": 101}) == abi.UNAVAILABLE
    assert gather(L, **{**gg, "out": None, "out_stride": 0}) == abi.UNAVAILABLE
    assert gather(L, **{**gg, "voffs": p, "vstride": 0}) == abi.UNAVAILABLE
    assert gather(L, n_queries=0, n_keys=0, vbytes=0) == abi.UNAVAILABLE
    import turtle_kv_amd as amq
    with pytest.raises(amq.TkvAmqError) as e:
        amq.get_values(None, None, None, None, None, None)
    assert e.value.status == abi.UNAVAILABLE
