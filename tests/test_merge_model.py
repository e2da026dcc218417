"""The Python model of the leaf merge (tests/test_gpu_merge.py: `stable_merge`, `fold_group`,
`model_merge`, `job_ranges`), which the GPU tests hold the kernels to, itself held to a table written by
hand from include/tkv_amq.h: every ordered (newer, older) pair of the five ops, a newer ADD over an
unknown op and over an empty value, each with and without decay; the six data lengths of as_i32 with
negative integers; the wrap at 0x7fffffff + 1; the clamps of the jobs' ranges; and that merging three
levels as ((0, 1), 2), decaying in the last call only, equals the fold of their three-way stable merge.
No device."""
import numpy as np
import pytest

from test_gpu_merge import (ADD, BAD_COMBINE, COMBINED, DELETE, NOOP, OLDER, PAGE_SLICE, UNKNOWN, WRITE, fold_group,
                            job_ranges, model_merge, stable_merge)
from test_gpu_values import as_i32, unpack

A, B = 1000, -58                                                  # the newer and the older item's integers
KEPT, GONE = True, False


def v(op, x=None, width=4):
    if op is None:
        return b""
    return bytes([op]) + (b"" if x is None else int(x).to_bytes(width, "little", signed=True))


# (newer op, older op) -> (resolved op, flags, i32, kept under decay); None: the empty value
TABLE = {
    (DELETE, DELETE): (DELETE, 0, 0, GONE), (DELETE, NOOP): (DELETE, 0, 0, GONE), (DELETE, WRITE): (DELETE, 0, 0, GONE),
    (DELETE, ADD): (DELETE, 0, 0, GONE), (DELETE, PAGE_SLICE): (DELETE, 0, 0, GONE),
    (NOOP, DELETE): (NOOP, 0, 0, GONE), (NOOP, NOOP): (NOOP, 0, 0, GONE), (NOOP, WRITE): (NOOP, 0, 0, GONE),
    (NOOP, ADD): (NOOP, 0, 0, GONE), (NOOP, PAGE_SLICE): (NOOP, 0, 0, GONE),
    (WRITE, DELETE): (WRITE, 0, 0, KEPT), (WRITE, NOOP): (WRITE, 0, 0, KEPT), (WRITE, WRITE): (WRITE, 0, 0, KEPT),
    (WRITE, ADD): (WRITE, 0, 0, KEPT), (WRITE, PAGE_SLICE): (WRITE, 0, 0, KEPT),
    (ADD, DELETE): (WRITE, COMBINED, A, KEPT), (ADD, NOOP): (ADD, BAD_COMBINE, 0, KEPT),
    (ADD, WRITE): (WRITE, COMBINED, A + B, KEPT), (ADD, ADD): (ADD, COMBINED, A + B, KEPT),
    (ADD, PAGE_SLICE): (ADD, BAD_COMBINE, 0, KEPT),
    (PAGE_SLICE, DELETE): (PAGE_SLICE, 0, 0, KEPT), (PAGE_SLICE, NOOP): (PAGE_SLICE, 0, 0, KEPT),
    (PAGE_SLICE, WRITE): (PAGE_SLICE, 0, 0, KEPT), (PAGE_SLICE, ADD): (PAGE_SLICE, 0, 0, KEPT),
    (PAGE_SLICE, PAGE_SLICE): (PAGE_SLICE, 0, 0, KEPT),
    (ADD, UNKNOWN): (ADD, BAD_COMBINE, 0, KEPT), (ADD, None): (ADD, BAD_COMBINE, 0, KEPT),
}


@pytest.mark.parametrize("decay", [False, True])
@pytest.mark.parametrize("pair", sorted(TABLE, key=str))
def test_the_op_table(pair, decay):
    newer_op, older_op = pair
    op, flags, i32, kept = TABLE[pair]
    key = b"k" * 16
    recs, c = model_merge([(key, v(newer_op, A), 3)], [(b"a", v(WRITE, 1), OLDER | 6), (key, v(older_op, B), OLDER | 7)], decay)
    want = [(OLDER | 6, 0, WRITE, 0)] + ([(3, i32, op, flags)] if kept or not decay else [])
    assert recs == want
    assert c == {"newer_count": 1, "older_count": 2, "pair_count": 1, "combined_count": int(flags == COMBINED),
                 "bad_combine_count": int(flags == BAD_COMBINE), "dropped_count": int(decay and not kept),
                 "out_count": len(want)}


def test_an_unknown_op_and_an_empty_value_stand_as_they_are_and_decay():
    for value, op in ((v(UNKNOWN, 5), UNKNOWN), (b"", NOOP)):
        for older in ([], [(b"k", v(WRITE, 1), OLDER | 0)]):
            assert model_merge([(b"k", value, 0)], older, False)[0] == [(0, 0, op, 0)]
            recs, c = model_merge([(b"k", value, 0)], older, True)
            assert recs == [] and c["dropped_count"] == 1 and c["pair_count"] == len(older)
    # an older item that nothing shadows is judged by its own op
    assert model_merge([], [(b"k", v(DELETE), OLDER | 4)], False)[0] == [(OLDER | 4, 0, DELETE, 0)]
    assert model_merge([], [(b"k", v(DELETE), OLDER | 4)], True)[0] == []
    assert model_merge([], [(b"k", v(ADD, 9), OLDER | 4)], True)[0] == [(OLDER | 4, 0, ADD, 0)]


@pytest.mark.parametrize("width,x", [(0, 0), (1, -128), (1, -1), (2, -32768), (2, -2), (3, -(1 << 23)), (3, -3),
                                     (4, -(1 << 31)), (4, -4), (8, -5)])
def test_as_i32_widths_in_the_fold(width, x):
    data = b"" if width == 0 else (int(x).to_bytes(4, "little", signed=True) + b"\x00\xff\xff\x7f")[:width] \
        if width > 4 else int(x).to_bytes(width, "little", signed=True)
    assert as_i32(data) == x
    assert fold_group([bytes([ADD]) + data, v(WRITE, 100)]) == (WRITE, x + 100, COMBINED, 0)
    assert fold_group([v(ADD, 100), bytes([ADD]) + data]) == (ADD, 100 + x, COMBINED, 0)


def test_sums_wrap_modulo_2_32():
    assert fold_group([v(ADD, 0x7FFFFFFF), v(WRITE, 1)]) == (WRITE, -(1 << 31), COMBINED, 0)
    assert fold_group([v(ADD, -(1 << 31)), v(ADD, -1)]) == (ADD, 0x7FFFFFFF, COMBINED, 0)
    assert fold_group([v(ADD, 0x7FFFFFFF), v(DELETE)]) == (WRITE, 0x7FFFFFFF, COMBINED, 0)


def test_the_stable_merge_orders_as_string_views_and_puts_the_newer_first():
    newer = [(b"a", "n0"), (b"ab", "n1"), (b"b", "n2")]
    older = [(b"", "o0"), (b"a", "o1"), (b"aa", "o2"), (b"b", "o3"), (b"ba", "o4")]
    assert [t for _, t in stable_merge([newer, older])] == ["o0", "n0", "o1", "o2", "n1", "n2", "o3", "o4"]


def test_job_ranges_clamp_and_never_read_more_than_the_run_holds():
    assert job_ranges([0, 3, 10], 10) == [(0, 3), (3, 10)]
    assert job_ranges([2, 50, 1 << 63], 10) == [(2, 10), (10, 10)]      # ends past the count
    assert job_ranges([4, 2, 9], 10) == [(4, 4), (2, 9)]                 # an end below its begin
    assert job_ranges([0, 10, 0, 10], 10) == [(0, 10), (10, 10), (0, 0)]  # ranges that overlap: ten items in all
    assert job_ranges([0, 6, 2, 10], 10) == [(0, 6), (6, 6), (2, 6)]


def materialise(recs, newer, older):
    """The kept items as (key, packed value): a COMBINED record's value is its op byte and integer."""
    by_src = {s: (k, val) for k, val, s in newer + older}
    return [(by_src[src][0], bytes([op]) + int(i32).to_bytes(4, "little", signed=True) if flags & COMBINED
             else by_src[src][1]) for src, i32, op, flags in recs]


def test_three_levels_merged_pairwise_equal_the_three_way_fold():
    rng = np.random.default_rng(7)
    levels = []
    for _ in range(3):
        keys = sorted(int(x) for x in rng.choice(400, 220, replace=False))
        levels.append([(b"%05d" % k, v(int(rng.choice([WRITE, DELETE, ADD, ADD])), int(rng.integers(-1 << 31, 1 << 31))))
                       for k in keys])
    tag = lambda items, bit: [(k, val, bit | i) for i, (k, val) in enumerate(items)]
    first = model_merge(tag(levels[0], 0), tag(levels[1], OLDER), False)[0]
    upper = materialise(first, tag(levels[0], 0), tag(levels[1], OLDER))
    last = model_merge(tag(upper, 0), tag(levels[2], OLDER), True)[0]
    got = materialise(last, tag(upper, 0), tag(levels[2], OLDER))
    merged, want, at = stable_merge(levels), [], 0
    while at < len(merged):
        end = at + 1
        while end < len(merged) and merged[end][0] == merged[at][0]:
            end += 1
        op, i32, flags, bad = fold_group([m[1] for m in merged[at:end]])
        assert bad == 0
        if op in (WRITE, ADD):
            want.append((merged[at][0], bytes([op]) + int(i32).to_bytes(4, "little", signed=True) if flags & COMBINED
                         else merged[at][1]))
        at = end
    assert len(want) > 200 and sum(1 for m in merged if unpack(m[1])[0] == ADD) > 200
    assert got == want
