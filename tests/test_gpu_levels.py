"""tkv_amq_merge_levels and tkv_amq_gather_levels on the device against a Python model written from
include/tkv_amq.h: `model_levels` is the K-way stable merge of one job's runs (`stable_merge`), the
sequential fold of every group of equal keys (`fold_group`) and the keep rule, with the header's counts
(tests/test_levels_model.py holds it to a table written by hand).  Every comparison is exact, every
output sits between canary guards."""
import numpy as np
import pytest

from test_gpu_merge import (ADD, CANARY, COMBINED, COUNTS, DELETE, NOOP, OPS, PAGE_SLICE, SHAPES, STAYS,
                            UNKNOWN, WRITE, Run, begins, edge_jobs, flat, fold_group, i32, job_ranges, launch_gather,
                            launch_merge, pool, random_jobs, random_value, read_gather, read_merge, record_array, same_gather,
                            same_merge, stable_merge, table_value)
from test_gpu_values import as_i32, signed, unpack
from test_gpu_walk import dev, guarded, key16, leaf

pytestmark = pytest.mark.gpu

SHIFT = 56                                                        # TKV_AMQ_LEVELS_SRC_SHIFT
INDEX = (1 << SHIFT) - 1


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available()
    return t


# ---------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------
def model_levels(levels, decay):
    """levels: one job's runs, the newest first, as lists of (key, packed value, src).  The records of
    the kept groups, in key order, as (src, i32, op, flags), and the job's counts."""
    merged = stable_merge(levels)
    recs, c = [], dict.fromkeys(COUNTS, 0)
    c["newer_count"], c["older_count"] = len(levels[0]), sum(len(lv) for lv in levels[1:])
    at = 0
    while at < len(merged):
        end = at + 1
        while end < len(merged) and merged[end][0] == merged[at][0]:
            end += 1
        op, x, flags, bad = fold_group([m[1] for m in merged[at:end]])
        c["pair_count"] += end - at - 1
        c["combined_count"] += bool(flags & COMBINED)
        c["bad_combine_count"] += bad
        if decay and op not in STAYS:
            c["dropped_count"] += 1
        else:
            recs.append((merged[at][2], x, op, flags))
        at = end
    c["out_count"] = len(recs)
    return recs, c


def model_batch(runs, bs, decay):
    """The whole call over `runs` (Run objects, the newest first) and their begin arrays."""
    recs, begin, total = [], [0], dict.fromkeys(COUNTS, 0)
    ranges = [job_ranges(b, r.n) for r, b in zip(runs, bs)]
    for j in range(len(bs[0]) - 1):
        levels = [[(r.keys[i], r.values[i], s << SHIFT | i) for i in range(*ranges[s][j])] for s, r in enumerate(runs)]
        got, c = model_levels(levels, decay)
        recs += got
        begin.append(len(recs))
        for name in COUNTS:
            total[name] += c[name]
    return recs, np.array(begin, np.int64), total


def model_gather(recs, runs):
    """The key and the packed value of every record; a run or an index past the table gives an empty item."""
    keys, values = [], []
    for src, x, op, flags in recs:
        s, i = src >> SHIFT, src & INDEX
        if s >= len(runs) or i >= runs[s].n:
            keys.append(b"")
            values.append(b"")
            continue
        keys.append(runs[s].keys[i])
        values.append(bytes([op]) + i32(x) if flags & COMBINED else runs[s].values[i])
    return keys, values


# ---------------------------------------------------------------------------------------
# the device side
# ---------------------------------------------------------------------------------------
def launch_levels(amq, torch, runs, bs, decay, capacity, bufs=None, stream=None):
    n_jobs = len(bs[0]) - 1
    if bufs is None:
        total = sum(r.n for r in runs)
        bufs = {"begin": guarded(torch, n_jobs + 1, torch.int64), "items": guarded(torch, 16 * capacity, torch.uint8),
                "needed": guarded(torch, 1, torch.int64), "counts": guarded(torch, len(COUNTS), torch.int64),
                "ws": (None, torch.empty(amq.merge_levels_workspace_bytes(n_jobs, len(runs), total), dtype=torch.uint8,
                                         device="cuda")),
                "b": [dev(torch, np.asarray(b, np.uint64).view(np.int64)) for b in bs]}
        bufs["counts"][1].zero_()
    assert bufs["items"][1].data_ptr() % 16 == 0
    amq.merge_levels_device([r.run(amq, b) for r, b in zip(runs, bufs["b"])], n_jobs, bufs["begin"][1], bufs["items"][1],
                            capacity, bufs["ws"][1], bufs["needed"][1], amq.abi.MERGE_DECAY_TO_ITEMS if decay else 0,
                            bufs["counts"][1], stream)
    return bufs


def fixed_out(runs):
    return all(r.kb.offsets is None and r.kb.stride == runs[0].kb.stride for r in runs)


def launch_gather_levels(amq, torch, d_items, d_begin, n_jobs, capacity, runs, fixed, k_cap, v_cap, bufs=None, stream=None):
    """tkv_amq_gather_levels into guarded outputs; the value bytes start one byte past an aligned address."""
    if bufs is None:
        whole_v = torch.full((v_cap + 2 * 256 + 1,), CANARY, dtype=torch.uint8, device="cuda")
        bufs = {"keys": guarded(torch, k_cap, torch.uint8), "values": (whole_v, whole_v[257:257 + v_cap]),
                "koffs": None if fixed else guarded(torch, capacity + 1, torch.int64),
                "voffs": guarded(torch, capacity + 1, torch.int64), "needed": guarded(torch, 2, torch.int64),
                "ws": (None, torch.empty(amq.gather_levels_workspace_bytes(capacity), dtype=torch.uint8, device="cuda"))}
    amq.gather_levels_device(d_items, d_begin, n_jobs, capacity, [r.run(amq) for r in runs], bufs["keys"][1],
                             runs[0].kb.stride if fixed else 0, None if fixed else bufs["koffs"][1], k_cap,
                             bufs["values"][1], bufs["voffs"][1], v_cap, bufs["ws"][1], bufs["needed"][1], stream)
    return bufs


def check(amq, torch, runs, bs, decay, capacity=None, k_cap=None, v_cap=None):
    """Merge and gather against the model; the capacities default to what holds everything."""
    want = model_batch(runs, bs, decay)
    recs = want[0]
    capacity = len(recs) + 3 if capacity is None else capacity
    bufs = launch_levels(amq, torch, runs, bs, decay, capacity)
    same_merge(amq, read_merge(amq, torch, bufs), want, capacity)
    keys, values = model_gather(recs[:capacity], runs)
    fixed = fixed_out(runs)
    k_cap = sum(len(k) for k in keys) + 5 if k_cap is None else k_cap
    v_cap = sum(len(v) for v in values) + 5 if v_cap is None else v_cap
    g = launch_gather_levels(amq, torch, bufs["items"][1], bufs["begin"][1], len(bs[0]) - 1, capacity, runs, fixed,
                             k_cap, v_cap)
    same_gather(read_gather(torch, g, v_cap), keys, values, k_cap, v_cap, runs[0].kb.stride if fixed else 0)
    return want


def random_levels(rng, keys, n_jobs, n_runs, presence=0.5):
    """Per run and job a sorted slice of the pool: every key is in each level with probability `presence`."""
    out = [[] for _ in range(n_runs)]
    for part in np.array_split(np.arange(len(keys)), n_jobs):
        pick = rng.random((n_runs, len(part))) < presence
        for s in range(n_runs):
            out[s].append([keys[i] for i, p in zip(part, pick[s]) if p])
    return out


def mostly_adds(rng):
    op = int(rng.choice([ADD, ADD, ADD, ADD, ADD, WRITE, DELETE, NOOP, PAGE_SLICE, UNKNOWN]))
    return bytes([op]) + i32(int(rng.integers(-1 << 31, 1 << 31)))


# ---------------------------------------------------------------------------------------
# 1. the op table
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("decay", [False, True])
def test_the_op_table_on_the_device(amq, torch, decay):
    """One job, three runs: every ordered triple of the five ops, an unknown op and the empty value on a key of
    its own -- 343 groups of three."""
    triples = [(a, b, c) for a in OPS for b in OPS for c in OPS]
    keys = [key16(3 * j) for j in range(len(triples))]
    runs = [Run(amq, torch, keys, [table_value(t[s], (1000, -40, 77)[s] + 7 * j) for j, t in enumerate(triples)])
            for s in range(3)]
    recs, begin, counts = check(amq, torch, runs, [[0, len(keys)]] * 3, decay)
    assert counts["pair_count"] == 2 * len(triples)
    # ADD over {WRITE, DELETE, ADD} directly (21 triples), or over a bad middle and then one of them (4 * 3)
    assert counts["combined_count"] == 3 * 7 + 4 * 3
    # a bad middle (4 * 7), and a bad last under an ADD or a bad middle ((1 + 4) * 4)
    assert counts["bad_combine_count"] == 4 * 7 + 5 * 4
    assert counts["dropped_count"] == (4 * 49 if decay else 0)


# ---------------------------------------------------------------------------------------
# 2. two runs: the leaf merge
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["k16", "var", "fixed_over_var"])
def test_two_runs_equal_merge_leaves(amq, torch, shape):
    which, nf, of, shift = SHAPES[shape]
    rng = np.random.default_rng(70 + sorted(SHAPES).index(shape))
    newer, older = random_jobs(rng, pool(which, rng, 1300), 4)
    N = Run(amq, torch, flat(newer), [random_value(rng, "offsets") for _ in flat(newer)], nf, "offsets", shift)
    O = Run(amq, torch, flat(older), [random_value(rng, "stride") for _ in flat(older)], of, "stride")
    nb, ob = begins([len(r) for r in newer]), begins([len(r) for r in older])
    capacity, fixed = N.n + O.n, shape == "k16"
    k_cap, v_cap = sum(map(len, N.keys + O.keys)), sum(map(len, N.values + O.values)) + 4 * N.n
    assert v_cap == amq.merge_levels_values_bound(sum(map(len, N.values + O.values)), N.n)
    for decay in (False, True):
        pair = launch_merge(amq, torch, N, O, nb, ob, decay, capacity)
        a = read_merge(amq, torch, pair)
        table = launch_levels(amq, torch, [N, O], [nb, ob], decay, capacity)
        b = read_merge(amq, torch, table)
        assert a["begin"][-1] > 500 and a["counts"][2] > 50 and a["counts"][3] > 0 and a["counts"][4] > 0
        for name in ("begin", "needed", "counts"):
            assert np.array_equal(a[name], b[name]), name
        n = int(a["needed"][0])
        for name in ("i32", "op", "flags", "reserved"):
            assert np.array_equal(a["rec"][name][:n], b["rec"][name][:n]), name
        src = a["rec"]["src"][:n]
        assert np.array_equal((src >> np.uint64(63)) << np.uint64(SHIFT) | (src & np.uint64((1 << 63) - 1)), b["rec"]["src"][:n])
        assert (b["rec"][n:].view(np.uint8) == CANARY).all()
        ga = read_gather(torch, launch_gather(amq, torch, pair["items"][1], pair["begin"][1], 4, capacity, N, O, fixed,
                                              k_cap, v_cap), v_cap)
        gb = read_gather(torch, launch_gather_levels(amq, torch, table["items"][1], table["begin"][1], 4, capacity, [N, O],
                                                     fixed, k_cap, v_cap), v_cap)
        assert sorted(ga) == sorted(gb)
        for name in ga:
            assert np.array_equal(ga[name], gb[name]), name


# ---------------------------------------------------------------------------------------
# 3. every run count
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_runs", range(1, 9))
def test_every_run_count(amq, torch, n_runs):
    rng = np.random.default_rng(100 + n_runs)
    keys = [key16(5 * x) for x in range(1600)]
    levels = random_levels(rng, keys, 40, n_runs)
    runs = [Run(amq, torch, flat(lv), [mostly_adds(rng) for _ in flat(lv)], value_form="stride") for lv in levels]
    bs = [begins([len(j) for j in lv]) for lv in levels]
    if n_runs >= 4:
        # the inputs hold what the test is about: a group of four items or more whose fold reaches its last item
        deep = 0
        for j in range(40):
            merged = stable_merge([[(r.keys[i], r.values[i]) for i in range(int(b[j]), int(b[j + 1]))]
                                   for r, b in zip(runs, bs)])
            by_key = {}
            for k, v in merged:
                by_key.setdefault(k, []).append(v)
            deep += sum(1 for vs in by_key.values()
                        if len(vs) >= 4 and all(unpack(v)[0] == ADD for v in vs[:-1]) and unpack(vs[-1])[0] in (ADD, WRITE))
        assert deep > 0
    for decay in (False, True):
        recs, begin, counts = check(amq, torch, runs, bs, decay)
        assert counts["out_count"] > 300
        if n_runs == 1:                                           # the decay filter alone
            assert counts["pair_count"] == counts["combined_count"] == counts["older_count"] == 0
            assert counts["out_count"] + counts["dropped_count"] == runs[0].n and (counts["dropped_count"] > 0) == decay
        else:
            assert counts["pair_count"] > 100 and counts["combined_count"] > 50 and counts["bad_combine_count"] > 0


# ---------------------------------------------------------------------------------------
# 4. key and value shapes
# ---------------------------------------------------------------------------------------
TABLES = {  # name: (pool, per run (key form, shift)); the value forms alternate run by run
    "k16": ("k16", [("fixed", 0)] * 3), "k24": ("k24", [("fixed", 0)] * 3), "k11": ("k11", [("fixed", 0)] * 3),
    "var": ("var", [("var", 0)] * 3),
    "var_among_fixed": ("k16", [("fixed", 0), ("var", 0), ("fixed", 0)]),
    "var_oldest": ("k24", [("fixed", 0), ("fixed", 0), ("var", 0)]),
    "k16_misaligned": ("k16", [("fixed", 0), ("fixed", 0), ("fixed", 8)]),
    "k24_misaligned": ("k24", [("fixed", 4), ("fixed", 0), ("fixed", 0)]),
}


@pytest.mark.parametrize("first_form", ["offsets", "stride"])
@pytest.mark.parametrize("table", sorted(TABLES))
def test_key_and_value_shapes(amq, torch, table, first_form):
    which, forms = TABLES[table]
    assert {SHAPES[s][0] for s in SHAPES} >= {which}                # the pools of the two-run shapes
    rng = np.random.default_rng(200 + 2 * sorted(TABLES).index(table) + (first_form == "stride"))
    levels = random_levels(rng, pool(which, rng, 1300), 4, 3)
    value_forms = [("offsets", "stride")[(s + (first_form == "stride")) % 2] for s in range(3)]
    runs = [Run(amq, torch, flat(lv), [random_value(rng, vf) for _ in flat(lv)], kf, vf, shift)
            for lv, (kf, shift), vf in zip(levels, forms, value_forms)]
    assert fixed_out(runs) == all(kf == "fixed" for kf, _ in forms)
    bs = [begins([len(j) for j in lv]) for lv in levels]
    for decay in (False, True):
        recs, begin, counts = check(amq, torch, runs, bs, decay)
        assert counts["pair_count"] > 100 and counts["combined_count"] > 0 and counts["bad_combine_count"] > 0


# ---------------------------------------------------------------------------------------
# 5. unit and round boundaries
# ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def boundary_case(amq, torch):
    """One job with runs of 2,500 / 1,100 / 300 / 0 / 5,000 items over a pool of 6,000 keys (a unit is 1,024
    items, a round 256: groups span units of different runs), among 40 small jobs: empty ones, jobs with one
    non-empty run, and jobs of exactly 256, 257, 1,024 and 1,025 items in one run."""
    rng = np.random.default_rng(301)
    big_pool = [key16(10 ** 6 + x) for x in range(6000)]
    big = [sorted(big_pool[i] for i in rng.choice(6000, n, replace=False)) for n in (2500, 1100, 300, 0, 5000)]
    jobs = []                                                       # per job: five lists of keys
    exact = {3: (0, 256), 9: (2, 257), 17: (4, 1024), 25: (1, 1025)}
    for j in range(40):
        base = 10 ** 4 * j
        if j % 10 == 0:
            jobs.append([[] for _ in range(5)])
        elif j in exact:
            s, n = exact[j]
            lone = [key16(base + 2 * x) for x in range(n)]
            jobs.append([lone if t == s else [key16(base + 7 * x) for x in range(int(rng.integers(0, 60)))] if j != 17
                         else [] for t in range(5)])
        elif j % 10 == 5:                                           # one run non-empty
            s = j // 10
            jobs.append([[key16(base + x) for x in range(int(rng.integers(1, 90)))] if t == s else [] for t in range(5)])
        else:
            small = [key16(base + x) for x in range(120)]
            jobs.append([[k for k in small if rng.random() < 0.4] for _ in range(5)])
    jobs.insert(20, big)
    assert [len(x) for x in jobs[20]] == [2500, 1100, 300, 0, 5000] and len(jobs) == 41
    levels = [[job[s] for job in jobs] for s in range(5)]
    ops = [DELETE, WRITE, ADD, ADD, ADD, NOOP, PAGE_SLICE]
    runs = [Run(amq, torch, flat(lv), [bytes([ops[(j + s) % 7]]) + i32(j - 1000 * s) for j in range(len(flat(lv)))],
                value_form="stride") for s, lv in enumerate(levels)]
    return runs, [begins([len(j) for j in lv]) for lv in levels]


@pytest.mark.parametrize("decay", [False, True])
def test_groups_across_unit_and_round_boundaries(amq, torch, boundary_case, decay):
    runs, bs = boundary_case
    recs, begin, counts = check(amq, torch, runs, bs, decay)
    sizes = np.diff(begin)
    assert sizes[0] == 0 and sizes[10] == 0 and sizes[21] == 0 and sizes[20] > (2500 if decay else 5000)
    assert counts["pair_count"] > 2000 and counts["combined_count"] > 300   # (the inputs hold what the test is about)


# ---------------------------------------------------------------------------------------
# 6. edges of the jobs
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("decay", [False, True])
def test_edges_of_the_jobs(amq, torch, decay):
    """The two-run edge jobs over three runs (runs 1 and 2 both hold the older side's keys, with values of their own),
    and per run two more jobs: an end below its begin (empty), then one that reaches back into the last job's items
    -- an overlapping range -- and past the run's end: it reads what the run's item count leaves it."""
    rng = np.random.default_rng(411)
    jobs = edge_jobs(rng)
    tail = [key16(500 + x) for x in range(6)]
    per_run = [(0, 2, 6), (1, 3, 4), (1, 3, 5)]                       # (keys of, values by, items behind the last job)
    runs, bs = [], []
    for s, (ki, vi, extra) in enumerate(per_run):
        keys = flat(j[ki] for j in jobs) + tail[:extra]
        vals = [j[vi](k) for j in jobs for k in j[ki]] + [bytes([ADD, s + 1])] * extra
        runs.append(Run(amq, torch, keys, vals))
        b = begins([len(j[ki]) for j in jobs])
        bs.append(np.array([int(x) for x in b] + [int(b[-1]) - 2 - s, (1 << 40, (1 << 64) - 1, 1 << 63)[s]], np.uint64))
    want = check(amq, torch, runs, bs, decay)
    sizes = np.diff(want[1])
    assert sizes[-2] == 0 and sizes[-1] > 0
    far = np.full(len(bs[0]), 1 << 50, np.int64)
    recs, begin, counts = check(amq, torch, runs, [far] * 3, decay)
    assert not recs and counts["newer_count"] == 0 and counts["older_count"] == 0


def test_no_jobs(amq, torch):
    N = Run(amq, torch, [key16(1)], [b"\x02a"])
    got = read_merge(amq, torch, launch_levels(amq, torch, [N, N, N], [[0]] * 3, False, 4))
    assert int(got["begin"][0]) == 0 and int(got["needed"][0]) == 0 and not got["counts"].any()
    assert (got["rec"].view(np.uint8) == CANARY).all()


# ---------------------------------------------------------------------------------------
# 7. short capacities
# ---------------------------------------------------------------------------------------
def test_short_capacities(amq, torch):
    rng = np.random.default_rng(531)
    levels = random_levels(rng, pool("var", rng, 900), 5, 3)
    runs = [Run(amq, torch, flat(lv), [random_value(rng, "offsets") for _ in flat(lv)], "var") for lv in levels]
    bs = [begins([len(j) for j in lv]) for lv in levels]
    recs, begin, counts = model_batch(runs, bs, False)
    keys, values = model_gather(recs, runs)
    check(amq, torch, runs, bs, False, capacity=len(recs) // 2)
    check(amq, torch, runs, bs, False, k_cap=sum(map(len, keys)) // 2)
    check(amq, torch, runs, bs, False, v_cap=sum(map(len, values)) // 2)
    check(amq, torch, runs, bs, False, capacity=0, k_cap=0, v_cap=0)
    # the fixed key form: slots below the capacity, whole
    rng = np.random.default_rng(532)
    levels = random_levels(rng, pool("k11", rng, 300), 2, 3)
    runs = [Run(amq, torch, flat(lv), [random_value(rng, "stride") for _ in flat(lv)], value_form="stride") for lv in levels]
    check(amq, torch, runs, [begins([len(j) for j in lv]) for lv in levels], True, k_cap=11 * 100 + 5)


# ---------------------------------------------------------------------------------------
# 8. records the gather does not trust
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("fixed", [False, True])
def test_forged_records_give_empty_items(amq, torch, fixed):
    keys = [key16(x) for x in range(6)]
    runs = [Run(amq, torch, keys[:3], [b"\x02new%d" % j for j in range(3)], "fixed" if fixed else "var"),
            Run(amq, torch, keys[:4], [b"\x02mid%d" % j for j in range(4)]),
            Run(amq, torch, keys, [b"\x02older%d" % j for j in range(6)])]
    S = lambda s, i: s << SHIFT | i
    recs = [(S(0, 0), 0, WRITE, 0), (S(0, 3), 0, WRITE, 0), (S(1, 3), 0, WRITE, 0), (S(1, 4), 0, WRITE, 0),
            (S(2, 5), 0, WRITE, 0), (S(2, 6), 0, WRITE, 0), (S(3, 0), 0, WRITE, 0), (S(8, 1), 0, WRITE, 0),
            (S(255, 0), 7, WRITE, COMBINED), (S(0, INDEX), 7, WRITE, COMBINED), (S(2, 1 << 55), 0, ADD, 0),
            (S(1, 2), -9, ADD, COMBINED), ((1 << 64) - 1, 0, DELETE, 0)]
    d_items = dev(torch, np.frombuffer(record_array(amq, recs).tobytes(), np.uint8).copy())
    d_begin = dev(torch, np.array([0, 2, len(recs)], np.int64))
    want_k, want_v = model_gather(recs, runs)
    assert [k != b"" for k in want_k] == [True, False, True, False, True, False, False, False, False, False, False, True, False]
    assert want_v[8] == b"" and want_v[11] == bytes([ADD]) + i32(-9)
    k_cap = 16 * len(recs) + 3
    g = launch_gather_levels(amq, torch, d_items, d_begin, 2, len(recs), runs, fixed, k_cap, 100)
    same_gather(read_gather(torch, g, 100), want_k, want_v, k_cap, 100, 16 if fixed else 0)
    # a forged total: no more records are gathered than the capacity, or than the runs have items
    d_begin = dev(torch, np.array([0, 2, 1 << 40], np.int64))
    g = launch_gather_levels(amq, torch, d_items, d_begin, 2, len(recs) - 1, runs, fixed, k_cap, 100)
    same_gather(read_gather(torch, g, 100), want_k[:-1], want_v[:-1], k_cap, 100, 16 if fixed else 0)
    g = launch_gather_levels(amq, torch, d_items, d_begin, 2, len(recs), runs[:1], fixed, k_cap, 100)    # 3 items in all
    same_gather(read_gather(torch, g, 100), *model_gather(recs[:3], runs[:1]), k_cap, 100, 16 if fixed else 0)


# ---------------------------------------------------------------------------------------
# 9. runs that are not sorted
# ---------------------------------------------------------------------------------------
def test_unsorted_runs_stay_inside_their_jobs(amq, torch):
    """No merge answer is asserted: the call returns, nothing outside the outputs is written, the counts add up and
    every record that was written names an item of its own job."""
    rng = np.random.default_rng(641)
    sizes = [[int(x) for x in rng.integers(0, hi, 12)] for hi in (900, 1400, 300, 3000)]
    runs = [Run(amq, torch, [key16(int(x)) for x in rng.integers(0, 500, sum(sz))], [bytes([(ADD, ADD, WRITE, ADD)[s], 1])] * sum(sz))
            for s, sz in enumerate(sizes)]
    bs = [begins(sz) for sz in sizes]
    total = sum(r.n for r in runs)
    for decay in (False, True):
        bufs = launch_levels(amq, torch, runs, bs, decay, total)
        got = read_merge(amq, torch, bufs)
        begin, c = got["begin"], dict(zip(COUNTS, (int(v) for v in got["counts"])))
        assert begin[0] == 0 and (np.diff(begin) >= 0).all() and begin[-1] == got["needed"][0] == c["out_count"] <= total
        assert c["newer_count"] == runs[0].n and c["older_count"] == total - runs[0].n
        assert c["out_count"] == total - c["pair_count"] - c["dropped_count"]
        for j in range(12):
            rec = got["rec"][begin[j]:begin[j + 1]]
            written = rec[(rec.view(np.uint8).reshape(-1, 16) != CANARY).any(axis=1)]
            idx, s = written["src"] & np.uint64(INDEX), (written["src"] >> np.uint64(SHIFT)).astype(np.int64)
            assert (s < 4).all()
            lo, hi = np.array([b[j] for b in bs])[s], np.array([b[j + 1] for b in bs])[s]
            assert ((idx >= lo) & (idx < hi)).all()
        assert (got["rec"][begin[-1]:].view(np.uint8) == CANARY).all()
        g = launch_gather_levels(amq, torch, bufs["items"][1], dev(torch, begin.copy()), 12, total, runs, True,
                                 16 * total, 8 * total)
        read_gather(torch, g, 8 * total)


# ---------------------------------------------------------------------------------------
# 10. one K-way call against the pairwise chain
# ---------------------------------------------------------------------------------------
def test_four_levels_equal_the_pairwise_chain(amq, torch):
    """merge_levels + gather_levels over four levels against three rounds of merge_leaves + gather_merged, the
    newest two first, decaying in the last round only: the device form of
    test_merge_model.py::test_three_levels_merged_pairwise_equal_the_three_way_fold."""
    rng = np.random.default_rng(707)
    keys = [key16(3 * x) for x in range(2400)]
    levels = random_levels(rng, keys, 6, 4, presence=0.55)

    def value():
        op = int(rng.choice([WRITE, DELETE, ADD, ADD, ADD, NOOP]))
        return bytes([op]) + bytes(rng.integers(0, 256, int(rng.integers(0, 7)), dtype=np.uint8))

    runs = [Run(amq, torch, flat(lv), [value() for _ in flat(lv)]) for lv in levels]
    bs = [begins([len(j) for j in lv]) for lv in levels]
    one = amq.merge_levels([(r.kb, r.vb, b) for r, b in zip(runs, bs)], decay=True)
    step = amq.merge_leaves(runs[0].kb, runs[0].vb, bs[0], runs[1].kb, runs[1].vb, bs[1])
    step = amq.merge_leaves(step.keys, step.values, step.out_begin, runs[2].kb, runs[2].vb, bs[2])
    last = amq.merge_leaves(step.keys, step.values, step.out_begin, runs[3].kb, runs[3].vb, bs[3], decay=True)
    assert one.counts["out_count"] == last.counts["out_count"] > 1500 and one.counts["dropped_count"] > 50
    assert one.counts["combined_count"] > 300
    assert torch.equal(one.out_begin, last.out_begin)
    assert one.keys.stride == last.keys.stride == 16 and torch.equal(one.keys.data, last.keys.data)
    n_bytes = int(one.values.offsets[-1])
    assert torch.equal(one.values.offsets, last.values.offsets)
    assert torch.equal(one.values.data[:n_bytes], last.values.data[:n_bytes])
    # and both are the model's answer
    recs, begin, counts = model_batch(runs, bs, True)
    want_k, want_v = model_gather(recs, runs)
    assert one.counts == counts and np.array_equal(one.out_begin.cpu().numpy(), begin)
    assert bytes(one.keys.data.cpu().numpy().tobytes()) == b"".join(want_k)
    assert bytes(one.values.data[:n_bytes].cpu().numpy().tobytes()) == b"".join(want_v)


# ---------------------------------------------------------------------------------------
# 11. graph capture: the merge and the gather as one linear chain
# ---------------------------------------------------------------------------------------
def test_merge_and_gather_replay_in_a_graph(amq, torch):
    rng = np.random.default_rng(851)
    levels = random_levels(rng, pool("k16", rng, 1200), 6, 3)
    vals = [[bytes([(ADD, ADD, WRITE, DELETE)[(j + s) % 4]]) + i32(5 * j - s) for j, _ in enumerate(flat(lv))]
            for s, lv in enumerate(levels)]
    runs = [Run(amq, torch, flat(lv), v, value_form="stride" if s != 1 else "offsets") for s, (lv, v) in enumerate(zip(levels, vals))]
    bs = [begins([len(j) for j in lv]) for lv in levels]
    total = sum(r.n for r in runs)
    capacity, k_cap, v_cap = total, 16 * total, 9 * total
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    bufs = launch_levels(amq, torch, runs, bs, False, capacity, stream=s)
    g = launch_gather_levels(amq, torch, bufs["items"][1], bufs["begin"][1], 6, capacity, runs, True, k_cap, v_cap, stream=s)
    s.synchronize()

    def both():
        launch_levels(amq, torch, runs, bs, False, capacity, bufs, s)
        launch_gather_levels(amq, torch, bufs["items"][1], bufs["begin"][1], 6, capacity, runs, True, k_cap, v_cap, g, s)

    def verify():
        want = model_batch(runs, bs, False)
        same_merge(amq, read_merge(amq, torch, bufs), want, capacity)
        keys, values = model_gather(want[0], runs)
        same_gather(read_gather(torch, g, v_cap), keys, values, k_cap, v_cap, 16)

    verify()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        both()
    for turn in range(2):                                         # the inputs changed in place, the outputs refilled
        N = runs[0]
        swap = [bytes([(WRITE, ADD, DELETE)[(j + turn) % 3]]) + i32(turn - j) for j in range(N.n)]
        N.values = swap
        N.vb.data.copy_(torch.from_numpy(np.frombuffer(b"".join(swap), np.uint8).copy()).view(N.n, 5))
        O = runs[2]
        moved = sorted(levels[2][turn])[:-1] + [b"\xff" * 15 + bytes([turn])]   # one job's oldest run gets another last key
        at = int(bs[2][turn])
        O.keys[at:at + len(moved)] = moved
        O.kb.data[at:at + len(moved)].copy_(torch.from_numpy(np.frombuffer(b"".join(moved), np.uint8).copy()).view(-1, 16))
        bufs["counts"][1].zero_()
        for name in ("begin", "items", "needed"):
            bufs[name][1].view(torch.uint8).fill_(CANARY)
        for name in ("keys", "values", "voffs", "needed"):
            g[name][1].view(torch.uint8).fill_(CANARY)
        torch.cuda.synchronize()
        graph.replay()
        verify()


# ---------------------------------------------------------------------------------------
# 12. closing the loop: three levels -> merged leaves -> filters -> verified -> looked up, all on the device
# ---------------------------------------------------------------------------------------
def test_closing_the_loop(amq, torch):
    rng = np.random.default_rng(961)
    leaves = [[key16(1000 * li + 2 * x) for x in range(500 - 7 * li)] for li in range(3)]
    old_vals = [[bytes([WRITE]) + i32(int(rng.integers(-1000, 1000))) + b"payload-%d" % x for x in range(len(lv))]
                for lv in leaves]
    # two update levels over the leaves: writes, deletes and deltas on keys that exist and keys that do not
    updates = []
    for level in range(2):
        update = [[], [], []]
        for li in ((0, 2), (0, 1, 2))[level]:
            for x in sorted(int(v) for v in rng.choice(1000, 160, replace=False)):
                op = (WRITE, DELETE, ADD, ADD)[(x + level) % 4]
                update[li].append((key16(1000 * li + x), bytes([op]) + (i32(x - 300 - level) if op != DELETE else b"")))
        updates.append(update)
    # what a store holds, applied oldest first: key -> ("delete",) | ("sum", op, n) | ("bytes", value)
    want = {k: ("bytes", v) for lv, vs in zip(leaves, old_vals) for k, v in zip(lv, vs)}
    for update in reversed(updates):
        for k, v in flat(update):
            op, data = unpack(v)
            below = want.get(k)
            if op == WRITE:
                want[k] = ("bytes", v)
            elif op == DELETE:
                want[k] = ("delete",)
            elif below is None:
                want[k] = ("bytes", v)                             # a delta with nothing below it stays a delta
            elif below[0] == "delete":
                want[k] = ("sum", WRITE, signed(as_i32(data)))
            elif below[0] == "sum":
                want[k] = ("sum", below[1], signed(as_i32(data) + below[2]))
            else:
                bop, bdata = unpack(below[1])
                want[k] = ("sum", bop, signed(as_i32(data) + as_i32(bdata)))
    table = [Run(amq, torch, [k for k, v in flat(u)], [v for k, v in flat(u)]) for u in updates]
    table.append(Run(amq, torch, flat(leaves), flat(old_vals)))
    bs = [begins([len(x) for x in u]) for u in updates] + [begins([len(lv) for lv in leaves])]
    r = amq.merge_levels([(t.kb, t.vb, b) for t, b in zip(table, bs)])
    out_begin = r.out_begin.cpu().numpy()
    assert r.counts["out_count"] == len(want) == out_begin[-1] and r.counts["dropped_count"] == 0
    assert r.counts["combined_count"] == sum(1 for w in want.values() if w[0] == "sum") > 40
    assert sum(1 for rec in r.records() if rec["src"] >> np.uint64(SHIFT) == 1 and rec["flags"] & COMBINED) > 10
    assert r.keys.stride == 16 and r.keys.n == len(want)
    tree = amq.TreeIndex.from_description({"pivot_keys": [key16(0), key16(1000), key16(2000), key16(1 << 40)],
                                           "children": [leaf(0), leaf(1), leaf(2)], "levels": []})
    absent = [k for k in (key16(1000 * li + 2 * x + 1) for li in range(3) for x in range(600, 640)) if k not in want]
    queries = sorted(want) + absent
    qb = amq.KeyBatch.from_host(queries)
    for kind, bpk in ((amq.BLOOM, 10), (amq.VQF, 12)):
        plan = amq.plan_filters(kind, np.diff(out_begin), bpk, payload_capacity=32704 if kind else 0,
                                src_page_ids=[7000, 7001, 7002])
        filt = amq.build_all_filters(plan, r.keys)
        checks = amq.verify_members(plan, filt, r.keys, key_begin=r.out_begin)
        assert int(checks["missing"].sum()) == 0 and not checks["flags"].any()
        got = amq.get_values(plan, filt, tree, qb, r.keys, r.values, key_begin=r.out_begin, gather=64)
        rec, slots, lens = got.records(), got.slots.cpu().numpy(), got.lengths.cpu().numpy()
        vals = r.values.data.cpu().numpy()
        voffs = r.values.offsets.cpu().numpy()
        for q, (key, one) in enumerate(zip(queries, rec)):
            if key not in want:
                assert one["op"] == 0xFF and one["key_index"] == (1 << 64) - 1
                continue
            ki = int(one["key_index"])
            stored = bytes(vals[voffs[ki]:voffs[ki + 1]])
            state = want[key]
            if state[0] == "delete":
                assert one["op"] == DELETE and lens[q] == 0
            elif state[0] == "sum":                               # read from the gathered 5-byte value
                assert stored == bytes([state[1]]) + i32(state[2]) and one["op"] == state[1]
                assert lens[q] == 4 and bytes(slots[q][:4]) == i32(state[2])
            else:
                assert stored == state[1] and one["op"] == state[1][0]
                assert lens[q] == len(state[1]) - 1 and bytes(slots[q][:lens[q]]) == state[1][1:]
