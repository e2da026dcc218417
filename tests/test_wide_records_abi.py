"""The wide-record entry points that need no device: records per key, the any-shape route's
workspace size, and its answer without a GPU (include/tkv_amq.h; the header-versus-EXPORTS
check of test_abi.py covers their declarations)."""
import pytest

from turtle_kv_amd import abi


@pytest.fixture(scope="module")
def L():
    return abi.lib()


def test_records_per_key(L):
    assert [L.tkv_amq_bloom_records_per_key(k) for k in (0, 1, 8, 9, 16, 17)] == [0, 1, 1, 2, 2, 0]


def test_route_any_ws_bytes(L):
    f = L.tkv_amq_bloom_route_records_any_ws_bytes
    for n_parts in (0, 2049):
        assert f(1000, n_parts, 11) == 0
    for k in (0, 17):
        assert f(1000, 4, k) == 0
    for n, n_parts, k in ((0, 1, 1), (1000, 4, 8), (1000, 4, 9), (5_000_000, 2048, 16)):
        assert f(n, n_parts, k) > 0


def test_route_any_unavailable_without_a_device(L):
    # (with a device visible the same call is refused for its null segment instead)
    st = L.tkv_amq_bloom_route_records_any(None, None, 24, 0, None, 1, 11, 1, None, None, None, 0, None)
    assert st == (abi.UNAVAILABLE if L.tkv_amq_device_count() == 0 else abi.INVALID_ARGUMENT)


def test_exports_list_the_new_entry_points():
    for name in ("tkv_amq_bloom_records_per_key", "tkv_amq_bloom_route_records_any_ws_bytes",
                 "tkv_amq_bloom_route_records_any"):
        assert name in abi.EXPORTS
