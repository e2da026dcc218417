"""The path probe's entry points as far as they go without a device: the workspace size, the
export list, and the answer without a GPU (include/tkv_amq.h; the header-versus-EXPORTS check
of test_abi.py covers the declarations)."""
import numpy as np
import pytest

from turtle_kv_amd import abi


@pytest.fixture(scope="module")
def L():
    return abi.lib()


def test_ws_bytes(L):
    f = L.tkv_amq_path_probe_ws_bytes
    for nq, ne in ((0, 0), (1, 1), (70001, 226597)):
        assert f(nq, ne) >= 16
    # monotone in both arguments
    qs = (0, 1, 255, 256, 257, 70001, 1 << 20, 0xffffffff)
    es = (0, 1, 15, 16, 17, 226597, 1 << 24, 0xffffffff)
    for ne in es:
        v = [f(nq, ne) for nq in qs]
        assert v == sorted(v)
    for nq in qs:
        v = [f(nq, ne) for ne in es]
        assert v == sorted(v)
    assert f(70001, 226597) > f(70001, 0) and f(70001, 226597) > f(0, 226597)
    # counts the probe refuses
    assert f(0x100000000, 1) == 0 and f(1, 0x100000000) == 0


def test_exports_list_the_new_entry_points():
    for name in ("tkv_amq_path_probe_ws_bytes", "tkv_amq_path_probe"):
        assert name in abi.EXPORTS


def test_path_probe_unavailable_without_a_device(L):
    # (with a device visible the same call is refused for its null buffers instead)
    st = L.tkv_amq_path_probe(0, None, None, 1, None, None, 16, 1, None, None, 1, None, None, None, None,
                              None, None, 0, None)
    assert st == (abi.UNAVAILABLE if L.tkv_amq_device_count() == 0 else abi.INVALID_ARGUMENT)


def test_probe_paths_raises_without_a_device(L):
    import turtle_kv_amd as amq
    plan = amq.plan_filters(amq.BLOOM, [100], 10)
    if L.tkv_amq_device_count() != 0:
        amq.filters._require_device()   # a device is visible: tests/test_gpu_path_probe.py runs it
        return
    with pytest.raises(amq.TkvAmqError) as e:
        amq.probe_paths(plan, None, None, np.zeros(2, np.int32), np.zeros(0, np.int32))
    assert e.value.status == abi.UNAVAILABLE
