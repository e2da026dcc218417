"""The Python model of the K-way merge (tests/test_gpu_levels.py: `model_levels`), which the GPU tests
hold tkv_amq_merge_levels to, itself held to a table written by hand from include/tkv_amq.h: for three
levels every ordered triple of the seven value kinds whose outcome is not the two-level table's of its
first two (the fold reaches the third item), a head in the middle level, the counts of a group of four,
and on two levels the leaf merge's model.  No device."""
import numpy as np
import pytest

from test_gpu_levels import SHIFT, model_levels
from test_gpu_merge import (ADD, BAD_COMBINE, COMBINED, DELETE, NOOP, OLDER, OPS, PAGE_SLICE, UNKNOWN, WRITE, model_merge,
                            random_value)
from test_merge_model import A, B, TABLE, v

C = 7                                                              # the levels' integers, the newest first: A, B, C
BOTH = COMBINED | BAD_COMBINE
BADS = (NOOP, PAGE_SLICE, UNKNOWN, None)

# (newest, middle, oldest) -> (resolved op, flags, i32, bad combinations): the triples whose third item changes what
# the first two give, i.e. the fold is still an ADD_I32 when it reaches it
THREE = {(ADD, ADD, WRITE): (WRITE, COMBINED, A + B + C, 0), (ADD, ADD, DELETE): (WRITE, COMBINED, A + B, 0),
         (ADD, ADD, ADD): (ADD, COMBINED, A + B + C, 0)}
for bad in BADS:
    THREE[(ADD, ADD, bad)] = (ADD, BOTH, A + B, 1)                 # COMBINED, then a bad combination
    THREE[(ADD, bad, WRITE)] = (WRITE, BOTH, A + C, 1)             # BAD, then COMBINED: both flags
    THREE[(ADD, bad, DELETE)] = (WRITE, BOTH, A, 1)
    THREE[(ADD, bad, ADD)] = (ADD, BOTH, A + C, 1)
    for worse in BADS:
        THREE[(ADD, bad, worse)] = (ADD, BAD_COMBINE, 0, 2)        # counted once each


def level(key, op, x, src):
    return [(key, v(op, x), src)]


def one_group(ops, decay):
    key = b"k" * 16
    levels = [level(key, op, x, s << SHIFT | (5 + s)) for s, (op, x) in enumerate(zip(ops, (A, B, C, -3)))]
    return model_levels(levels, decay)


@pytest.mark.parametrize("decay", [False, True])
def test_three_levels_where_the_fold_reaches_the_third(decay):
    assert len(THREE) == 3 + 4 * 4 + 16
    for ops, (op, flags, x, bad) in THREE.items():
        recs, c = one_group(ops, decay)
        assert recs == [(5, x, op, flags)], ops                    # the head is the newest run's item; never dropped
        assert c == {"newer_count": 1, "older_count": 2, "pair_count": 2, "combined_count": int(bool(flags & COMBINED)),
                     "bad_combine_count": bad, "dropped_count": 0, "out_count": 1}, ops


@pytest.mark.parametrize("decay", [False, True])
def test_every_other_triple_is_the_two_level_table_of_its_first_two(decay):
    seen = 0
    for a in OPS:
        for b in OPS:
            for c_op in OPS:
                if (a, b, c_op) in THREE:
                    continue
                seen += 1
                recs, c = one_group((a, b, c_op), decay)
                if (a, b) in TABLE:
                    op, flags, x, kept = TABLE[(a, b)]
                else:                                               # a head that is no ADD_I32 stands as it is
                    op, flags, x, kept = (NOOP if a is None else a), 0, 0, a in (WRITE, PAGE_SLICE)
                assert a != ADD or op == WRITE                      # (ADD/WRITE/x, ADD/DELETE/x: the fold stops there)
                assert recs == ([(5, x, op, flags)] if kept or not decay else []), (a, b, c_op)
                assert c["pair_count"] == 2 and c["dropped_count"] == int(decay and not kept)
                assert c["bad_combine_count"] == 0 and c["combined_count"] == int(flags == COMBINED)
    assert seen == 343 - len(THREE)


def test_the_fold_stops_at_a_write_and_starts_at_the_head():
    assert one_group((ADD, WRITE, ADD), False)[0] == [(5, A + B, WRITE, COMBINED)]
    assert one_group((WRITE, ADD, ADD), False)[0] == [(5, 0, WRITE, 0)]
    assert one_group((DELETE, ADD, ADD), True)[0] == []


def test_a_head_in_the_middle_level():
    key = b"k" * 16
    newest = [(b"a", v(WRITE, 1), 0 << SHIFT | 0), (b"z", v(DELETE), 0 << SHIFT | 1)]
    middle, oldest = level(key, ADD, B, 1 << SHIFT | 9), level(key, WRITE, C, 2 << SHIFT | 4)
    recs, c = model_levels([newest, middle, oldest], True)
    assert recs == [(0, 0, WRITE, 0), (1 << SHIFT | 9, B + C, WRITE, COMBINED)]
    assert c == {"newer_count": 2, "older_count": 2, "pair_count": 1, "combined_count": 1, "bad_combine_count": 0,
                 "dropped_count": 1, "out_count": 2}
    # the same key in the oldest level alone: its own op judges it
    assert model_levels([newest, [], oldest], True)[0] == [(0, 0, WRITE, 0), (2 << SHIFT | 4, 0, WRITE, 0)]


def test_the_counts_of_a_group_of_four():
    recs, c = one_group((ADD, NOOP, ADD, WRITE), False)
    assert recs == [(5, A + C - 3, WRITE, BOTH)]
    assert c == {"newer_count": 1, "older_count": 3, "pair_count": 3, "combined_count": 1, "bad_combine_count": 1,
                 "dropped_count": 0, "out_count": 1}
    recs, c = one_group((ADD, ADD, DELETE, ADD), True)              # the fourth item is shadowed and not folded
    assert recs == [(5, A + B, WRITE, COMBINED)] and c["pair_count"] == 3 and c["combined_count"] == 1
    recs, c = one_group((NOOP, ADD, ADD, ADD), True)
    assert recs == [] and c["pair_count"] == 3 and c["dropped_count"] == 1 and c["combined_count"] == 0


@pytest.mark.parametrize("decay", [False, True])
def test_two_levels_are_the_leaf_merge(decay):
    rng = np.random.default_rng(19)
    for _ in range(30):
        keys = sorted(int(x) for x in rng.choice(300, int(rng.integers(0, 120)), replace=False))
        pick = rng.random(len(keys))
        newer = [(b"%05d" % k, random_value(rng, "offsets")) for k, p in zip(keys, pick) if p < 0.6]
        older = [(b"%05d" % k, random_value(rng, "offsets")) for k, p in zip(keys, pick) if p > 0.4]
        pair = model_merge([(k, val, i) for i, (k, val) in enumerate(newer)],
                           [(k, val, OLDER | i) for i, (k, val) in enumerate(older)], decay)
        table = model_levels([[(k, val, i) for i, (k, val) in enumerate(newer)],
                              [(k, val, 1 << SHIFT | i) for i, (k, val) in enumerate(older)]], decay)
        assert table[1] == pair[1]
        assert [(s >> SHIFT << 63 | s & ((1 << SHIFT) - 1), x, op, f) for s, x, op, f in table[0]] == pair[0]
