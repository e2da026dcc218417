"""tkv_amq_verify_members as far as it goes without a device: the symbols bind, the result record
is 16 bytes, the workspace size, every InvalidArgument case of include/tkv_amq.h, and the answer
without a GPU.  tests/test_gpu_verify.py holds the device code to the oracle."""
import ctypes

import numpy as np
import pytest

from turtle_kv_amd import abi

BLOOM, VQF = 0, 1


class MemberCheck(ctypes.Structure):
    """tkv_amq_member_check as the header declares it."""
    _fields_ = [("first_missing", ctypes.c_uint64), ("missing", ctypes.c_uint32), ("flags", ctypes.c_uint32)]


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


def call(L, kind=BLOOM, filters=None, segs=None, n_segs=1, hint=0, keys=None, offs=None, stride=16, n_keys=4,
         key_begin=None, result=None, total=None, ws=None, ws_bytes=None):
    v = ctypes.c_void_p
    if ws_bytes is None:
        ws_bytes = L.tkv_amq_verify_members_ws_bytes(n_segs)
    return L.tkv_amq_verify_members(kind, v(filters), v(segs), n_segs, hint, v(keys), v(offs), stride, n_keys,
                                    v(key_begin), v(result), v(total), v(ws), ws_bytes, None)


def test_symbols_exist_and_bind(L):
    for name in ("tkv_amq_verify_members_ws_bytes", "tkv_amq_verify_members"):
        assert name in abi.EXPORTS
        assert hasattr(L, name)
    assert L.tkv_amq_verify_members.restype is ctypes.c_int and len(L.tkv_amq_verify_members.argtypes) == 15
    assert ctypes.sizeof(MemberCheck) == 16 == abi.MEMBER_CHECK_DTYPE.itemsize
    assert [abi.MEMBER_CHECK_DTYPE.fields[n][1] for n in ("first_missing", "missing", "flags")] == [0, 8, 12]
    assert (abi.VERIFY_NO_FILTER, abi.VERIFY_ID_MISMATCH) == (1, 2)
    import turtle_kv_amd as amq
    for name in ("verify_members", "verify_members_device", "verify_members_workspace_bytes"):
        assert hasattr(amq, name) and name in amq.__all__
    assert amq.verify_members_workspace_bytes(7) == L.tkv_amq_verify_members_ws_bytes(7)


def test_abi_version_unchanged():
    import os
    with open(os.path.join(abi._build.ROOT, "include", "tkv_amq.h")) as f:
        assert "#define TKV_AMQ_ABI_VERSION 3\n" in f.read()


def test_ws_bytes(L):
    f = L.tkv_amq_verify_members_ws_bytes
    ns = (0, 1, 2, 255, 256, 6104, 6105, 1 << 20, 0xFFFFFFFF)
    v = [f(n) for n in ns]
    assert all(x >= 16 and x % 16 == 0 for x in v)
    assert v == sorted(v) and v[-1] > v[0]
    assert all(f(n) >= 8 * (n + 1) for n in ns)  # the unit prefix: n_segs + 1 u64


# (a bad call is InvalidArgument with or without a device: the arguments are judged first)
def test_invalid_arguments(L, some):
    _, p = some
    good = dict(filters=p, segs=p, keys=p, result=p, ws=p)
    # unknown kind, with and without work
    assert call(L, kind=2, **good) == abi.INVALID_ARGUMENT
    assert call(L, kind=-1, n_segs=0, n_keys=0) == abi.INVALID_ARGUMENT
    # a null required buffer with a non-zero count
    for name in ("filters", "segs", "result", "ws", "keys"):
        assert call(L, **{**good, name: None}) == abi.INVALID_ARGUMENT, name
        assert call(L, kind=VQF, **{**good, name: None}) == abi.INVALID_ARGUMENT, name
    # fixed keys with stride 0 (variable-length keys carry none)
    assert call(L, stride=0, **good) == abi.INVALID_ARGUMENT
    # misaligned d_filters / d_result (16 bytes)
    assert call(L, **{**good, "filters": p + 8}) == abi.INVALID_ARGUMENT
    assert call(L, **{**good, "result": p + 8}) == abi.INVALID_ARGUMENT
    assert call(L, n_segs=0, n_keys=0, filters=p + 4) == abi.INVALID_ARGUMENT
    assert call(L, n_segs=0, n_keys=0, result=p + 8) == abi.INVALID_ARGUMENT
    # a short or misaligned workspace
    need = L.tkv_amq_verify_members_ws_bytes(1)
    assert call(L, ws_bytes=need - 1, **good) == abi.INVALID_ARGUMENT
    assert call(L, ws_bytes=0, **good) == abi.INVALID_ARGUMENT
    assert call(L, ws_bytes=need + 8, **{**good, "ws": p + 8}) == abi.INVALID_ARGUMENT
    need = L.tkv_amq_verify_members_ws_bytes(1000)
    assert call(L, n_segs=1000, ws_bytes=need - 16, **good) == abi.INVALID_ARGUMENT


def test_valid_calls_without_a_device(L, some):
    _, p = some
    good = dict(filters=p, segs=p, keys=p, result=p, ws=p)
    if L.tkv_amq_device_count() != 0:
        # a device is visible: an empty batch is simply OK (tests/test_gpu_verify.py runs the rest)
        assert call(L, n_segs=0, n_keys=0) == abi.OK
        return
    # n_segs == 0 with null buffers is judged before the device is looked for
    assert call(L, n_segs=0, n_keys=0) == abi.UNAVAILABLE
    assert call(L, kind=VQF, n_segs=0, n_keys=0, ws_bytes=0) == abi.UNAVAILABLE
    # valid calls: either kind, each key form, with and without the optional buffers
    assert call(L, **good) == abi.UNAVAILABLE
    assert call(L, kind=VQF, hint=509, **good) == abi.UNAVAILABLE
    assert call(L, stride=24, keys=p + 8, **{k: v for k, v in good.items() if k != "keys"}) == abi.UNAVAILABLE
    assert call(L, stride=0, offs=p, **good) == abi.UNAVAILABLE
    assert call(L, key_begin=p, total=p, **good) == abi.UNAVAILABLE
    assert call(L, n_keys=0, **{**good, "keys": None}) == abi.UNAVAILABLE
    import turtle_kv_amd as amq
    with pytest.raises(amq.TkvAmqError) as e:
        amq.verify_members(amq.plan_filters(amq.BLOOM, [100], 10), None, None)
    assert e.value.status == abi.UNAVAILABLE


def test_member_check_dtype_round_trip():
    raw = np.zeros(2, dtype=abi.MEMBER_CHECK_DTYPE)
    raw["first_missing"] = [abi.NONE_MISSING, 5]
    raw["missing"] = [0, 3]
    raw["flags"] = [abi.VERIFY_NO_FILTER, abi.VERIFY_ID_MISMATCH]
    m = (MemberCheck * 2).from_buffer_copy(raw.tobytes())
    assert (m[0].first_missing, m[0].missing, m[0].flags) == (2**64 - 1, 0, 1)
    assert (m[1].first_missing, m[1].missing, m[1].flags) == (5, 3, 2)
