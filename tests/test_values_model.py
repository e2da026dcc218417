"""The Python model of the value rule (tests/test_gpu_values.py: `unpack`, `as_i32`, `Fold`), which the
GPU tests hold the kernel to, itself held to a table written by hand from include/tkv_amq.h: every
ordered pair of ops, the six data lengths with negative integers, the wrap at 0x7fffffff + 1, and a
bad combination on the first item taken at its depth against one on a later item.  No device."""
import pytest

from test_gpu_values import (ADD, BAD_COMBINE, COMBINED, DELETE, NOOP, OP_NONE, PAGE_SLICE, WRITE, Fold, Values, as_i32,
                             signed, unpack)
from test_gpu_walk import LEAF_LEVEL

NOT_FOUND, NO_LEAF = (1 << 64) - 1, 0xFFFFFFFF


def v(op, x=None, width=4):
    return bytes([op]) + (b"" if x is None else int(x).to_bytes(width, "little", signed=True))


def test_unpack_and_the_empty_value():
    assert unpack(b"") == (NOOP, b"")
    assert unpack(bytes([WRITE])) == (WRITE, b"")
    assert unpack(bytes([ADD, 1, 2, 3])) == (ADD, b"\x01\x02\x03")
    assert unpack(bytes([9]) + b"zz") == (9, b"zz")
    assert (DELETE, NOOP, WRITE, ADD, PAGE_SLICE) == (0, 1, 2, 3, 4)


@pytest.mark.parametrize("data,want", [
    (b"", 0),
    (b"\x05", 5), (b"\x7f", 127), (b"\x80", -128), (b"\xff", -1),
    (b"\x2c\x01", 300), (b"\xff\x7f", 32767), (b"\x00\x80", -32768), (b"\xfe\xff", -2),
    (b"\x70\x11\x01", 70000), (b"\xff\xff\x7f", (1 << 23) - 1), (b"\x00\x00\x80", -(1 << 23)), (b"\xfd\xff\xff", -3),
    (b"\x01\x00\x00\x00", 1), (b"\xff\xff\xff\x7f", 0x7FFFFFFF), (b"\x00\x00\x00\x80", -(1 << 31)),
    (b"\xfc\xff\xff\xff", -4),
    (b"\x15\xcd\x5b\x07\xaa\xbb\xcc\xdd", 123456789), (b"\xfb\xff\xff\xff\x00\x00\x00\x00", -5),
    (b"\x00\x00\x00\x80\xff\xff\xff\x7f", -(1 << 31)), (b"\xff\xff\xff\x7f\xff\xff\xff\xff", 0x7FFFFFFF),
])
def test_as_i32_by_data_length(data, want):
    assert as_i32(data) == want


# (first op, second op) -> (resolved op, flags, accumulator, what the descent does after the second item) with the
# first item ADD 10 where it is an ADD, the second item's integer 7, both in one node
PAIRS_AFTER_ADD = {DELETE: (WRITE, COMBINED, 10, "stop"), NOOP: (ADD, BAD_COMBINE, 10, "leave"),
                   WRITE: (WRITE, COMBINED, 17, "stop"), ADD: (ADD, COMBINED, 17, "leave"),
                   PAGE_SLICE: (ADD, BAD_COMBINE, 10, "leave")}


@pytest.mark.parametrize("first", [DELETE, NOOP, WRITE, ADD, PAGE_SLICE])
@pytest.mark.parametrize("second", [DELETE, NOOP, WRITE, ADD, PAGE_SLICE])
def test_every_ordered_pair_of_ops(first, second):
    f = Fold()
    assert f.record() == (NOT_FOUND, NOT_FOUND, NO_LEAF, NO_LEAF, 0, OP_NONE, 0, 0)
    step = f.take(v(first, 10), 41, 3, 0 << 8 | 0)
    if first != ADD:
        # the value becomes the item and ends the lookup: a second item is never taken
        assert step == "stop" and f.record() == (41, 41, 3, 0, 0, first, 0, 1)
        return
    assert step == "leave" and f.record() == (41, 41, 3, 0, 10, ADD, 0, 1)
    step = f.take(v(second, 7), 77, 5, 0 << 8 | 2)
    op, flags, acc, want_step = PAIRS_AFTER_ADD[second]
    assert step == want_step
    # key_index, leaf and where stay the first item's; last_index is the second's
    assert f.record() == (41, 77, 3, 0, acc, op, flags, 2)
    assert f.bad == (1 if flags & BAD_COMBINE else 0)


def test_wrap_and_negative_sums():
    f = Fold()
    f.take(v(ADD, 0x7FFFFFFF), 1, 0, 0)
    assert f.take(v(ADD, 1), 2, 0, 1) == "leave"
    assert f.record()[4] == -(1 << 31) and f.record()[5] == ADD
    assert f.take(v(WRITE, -1), 3, 0, 2) == "stop"
    assert f.record()[4:7] == (0x7FFFFFFF, WRITE, COMBINED)
    f = Fold()
    f.take(v(ADD, -128, 1), 1, 0, 0)                              # one data byte, sign-extended
    f.take(v(ADD, -2, 2), 2, 0, 1)
    f.take(v(ADD, -(1 << 23), 3), 3, 0, 2)
    f.take(bytes([ADD]), 4, 0, 3)                                 # no data: 0
    f.take(bytes([WRITE]) + (5).to_bytes(4, "little") + b"\xff\xff", 5, 0, 4)   # six bytes: the first four
    assert f.record() == (1, 5, 0, 0, -128 - 2 - (1 << 23) + 5, WRITE, COMBINED, 5)
    assert signed(0x80000000) == -(1 << 31) and signed(-1) == -1 and signed(0x1_0000_0005) == 5
    # DELETE after sums: WRITE of the accumulator
    f = Fold()
    f.take(v(ADD, -9), 1, 0, 0)
    f.take(v(ADD, 4), 2, 0, 1)
    assert f.take(v(DELETE), 3, 0, 1 << 8) == "stop" and f.record() == (1, 3, 0, 0, -5, WRITE, COMBINED, 3)


def test_a_bad_combination_on_the_first_item_at_its_depth_ends_the_lookup():
    # ADD in the root (depth 0), NOOP the first item taken in the child node (depth 1): the child's whole answer,
    # which the parent's combine rejects -- nothing deeper is visited, the ADD stays pending
    f = Fold()
    assert f.take(v(ADD, 6), 10, 2, 0 << 8 | 1) == "leave"
    assert f.take(v(NOOP), 20, 5, 1 << 8 | 0) == "stop"
    assert f.record() == (10, 20, 2, 1, 6, ADD, BAD_COMBINE, 2) and f.bad == 1
    # the same NOOP after another item of the same node: the lookup goes on, and a WRITE below resolves it
    f = Fold()
    f.take(v(ADD, 6), 10, 2, 0 << 8 | 1)
    assert f.take(v(ADD, 1), 15, 4, 1 << 8 | 0) == "leave"
    assert f.take(v(NOOP), 20, 5, 1 << 8 | 1) == "leave"
    assert f.take(v(WRITE, 100), 30, 0, 1 << 8 | LEAF_LEVEL) == "stop"
    assert f.record() == (10, 30, 2, 1, 107, WRITE, COMBINED | BAD_COMBINE, 4) and f.bad == 1
    # in the node of the first item: never the first there
    f = Fold()
    f.take(v(ADD, 6), 10, 2, 0 << 8 | 0)
    assert f.take(v(PAGE_SLICE), 11, 3, 0 << 8 | 3) == "leave"
    # the child leaf is a depth of its own: its item is the first taken there even behind an item of its parent
    f = Fold()
    f.take(v(ADD, 6), 10, 2, 1 << 8 | 0)
    assert f.take(v(PAGE_SLICE), 11, 0, 1 << 8 | LEAF_LEVEL) == "stop"
    assert f.record() == (10, 11, 2, 1 << 8, 6, ADD, BAD_COMBINE, 2)
    # two bad items in one lookup: a later one in the root, then the first of the child
    f = Fold()
    f.take(v(ADD, 70), 1, 2, 0)
    assert f.take(v(PAGE_SLICE), 2, 4, 2) == "leave" and f.take(v(NOOP), 3, 5, 1 << 8) == "stop"
    assert f.bad == 2 and f.record()[4:] == (70, ADD, BAD_COMBINE, 3)
    # an op the reference does not define behaves as any other that cannot be combined
    f = Fold()
    f.take(v(ADD, 1), 1, 0, 0)
    assert f.take(bytes([9, 1, 2]), 2, 0, 1) == "leave" and f.record()[5:7] == (ADD, BAD_COMBINE)
    f = Fold()
    assert f.take(bytes([9, 1, 2]), 2, 0, 1) == "stop" and f.record()[5:] == (9, 0, 1)


def test_the_value_array_clamps():
    """Values.get without a device: the clamps of include/tkv_amq.h on a host copy."""
    class Host(Values):
        def __init__(self, blob, offs=None, stride=0, n_bytes=None):
            self.blob, self.offs, self.stride = bytes(blob), offs, stride
            self.n_bytes = len(blob) if n_bytes is None else n_bytes

    blob = bytes(range(20))
    h = Host(blob, offs=[0, 5, 5, 3, 12, 1 << 40, 20])
    assert h.get(0) == blob[0:5] and h.get(1) == b"" and h.get(2) == b"" and h.get(3) == blob[3:12]
    assert h.get(4) == blob[12:20] and h.get(5) == b""            # begin past the size: empty at the end
    h = Host(blob, offs=[0, 5, 10, 15, 20], n_bytes=12)
    assert h.get(1) == blob[5:10] and h.get(2) == blob[10:12] and h.get(3) == b""
    h = Host(blob, stride=6)
    assert h.get(2) == blob[12:18] and h.get(3) == blob[18:20] and h.get(4) == b"" and h.get(1 << 62) == b""
    h = Host(blob, stride=6, n_bytes=0)
    assert h.get(0) == b""
