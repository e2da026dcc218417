"""tkv_amq_merge_leaves and tkv_amq_gather_merged on the device against a Python model written from
include/tkv_amq.h: `model_merge` is a literal stable merge of the two runs followed by the sequential
fold of every group of equal keys and the keep rule (tests/test_merge_model.py holds the model to a
table written by hand).  Every comparison is exact, every output sits between canary guards."""
import numpy as np
import pytest

from test_gpu_values import as_i32, signed, unpack
from test_gpu_walk import CANARY, GUARD, dev, fixed_batch, guarded, key16, leaf

pytestmark = pytest.mark.gpu

DELETE, NOOP, WRITE, ADD, PAGE_SLICE = range(5)
UNKNOWN = 9
COMBINED, BAD_COMBINE = 1, 2
OLDER = 1 << 63
COUNTS = ("newer_count", "older_count", "pair_count", "combined_count", "bad_combine_count", "dropped_count",
          "out_count")
STAYS = (WRITE, ADD, PAGE_SLICE)


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available()
    return t


# ---------------------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------------------
def stable_merge(levels):
    """levels: lists of (key, ...) items, each ascending, the newest level first.  The stable merge in
    key order: among equal keys the item of the newer level comes first."""
    out = list(levels[0])
    for older in levels[1:]:
        merged, i, j = [], 0, 0
        while i < len(out) or j < len(older):
            if j == len(older) or (i < len(out) and out[i][0] <= older[j][0]):
                merged.append(out[i])
                i += 1
            else:
                merged.append(older[j])
                j += 1
        out = merged
    return out


def fold_group(values):
    """The packed values of a group of equal keys, newest first, folded as run_compact folds them: the
    first stands and is combined with the later ones while it is an ADD_I32.  (op, i32, flags, bad
    combinations); i32 is the folded integer of a COMBINED value, else 0."""
    op, data = unpack(values[0])
    acc, flags, bad = as_i32(data), 0, 0
    for v in values[1:]:
        if op != ADD:
            break
        o, d = unpack(v)
        if o == WRITE:
            op, acc, flags = WRITE, acc + as_i32(d), flags | COMBINED
        elif o == DELETE:
            op, flags = WRITE, flags | COMBINED
        elif o == ADD:
            acc, flags = acc + as_i32(d), flags | COMBINED
        else:
            flags, bad = flags | BAD_COMBINE, bad + 1
    return op, (signed(acc) if flags & COMBINED else 0), flags, bad


def model_merge(newer, older, decay):
    """newer, older: one job's runs as lists of (key, packed value, src).  The records of the kept
    groups, in order, as (src, i32, op, flags), and the job's counts."""
    merged = stable_merge([newer, older])
    recs, c = [], dict.fromkeys(COUNTS, 0)
    c["newer_count"], c["older_count"] = len(newer), len(older)
    at = 0
    while at < len(merged):
        end = at + 1
        while end < len(merged) and merged[end][0] == merged[at][0]:
            end += 1
        op, i32, flags, bad = fold_group([m[1] for m in merged[at:end]])
        if not merged[at][2] & OLDER:
            c["pair_count"] += end - at - 1
        c["combined_count"] += bool(flags & COMBINED)
        c["bad_combine_count"] += bad
        if decay and op not in STAYS:
            c["dropped_count"] += 1
        else:
            recs.append((merged[at][2], i32, op, flags))
        at = end
    c["out_count"] = len(recs)
    return recs, c


def job_ranges(begin, n):
    """The items each job reads of a run of n items: both ends clamped to n, an end below its begin
    empty, and no more than n items in all."""
    out, used = [], 0
    for j in range(len(begin) - 1):
        b, e = min(int(begin[j]), n), min(int(begin[j + 1]), n)
        count = min(max(e - b, 0), n - used)
        used += count
        out.append((b, b + count))
    return out


def model_batch(N, O, nb, ob, decay):
    """The whole call: records (a MERGE_ITEM_DTYPE-shaped list), out_begin and the counts."""
    recs, begin, total = [], [0], dict.fromkeys(COUNTS, 0)
    for (n0, n1), (o0, o1) in zip(job_ranges(nb, N.n), job_ranges(ob, O.n)):
        r, c = model_merge([(N.keys[i], N.values[i], i) for i in range(n0, n1)],
                           [(O.keys[i], O.values[i], OLDER | i) for i in range(o0, o1)], decay)
        recs += r
        begin.append(len(recs))
        for name in COUNTS:
            total[name] += c[name]
    return recs, np.array(begin, np.int64), total


def record_array(amq, recs):
    a = np.zeros(len(recs), amq.abi.MERGE_ITEM_DTYPE)
    for p, (src, i32, op, flags) in enumerate(recs):
        a[p] = (src, i32, op, flags, 0)
    return a


def model_gather(recs, N, O):
    """The key and the packed value of every record; a src past its run gives an empty item."""
    keys, values = [], []
    for src, i32, op, flags in recs:
        run, i = (O if src & OLDER else N), src & (OLDER - 1)
        if i >= run.n:
            keys.append(b"")
            values.append(b"")
            continue
        keys.append(run.keys[i])
        values.append(bytes([op]) + int(i32).to_bytes(4, "little", signed=True) if flags & COMBINED else run.values[i])
    return keys, values


# ---------------------------------------------------------------------------------------
# the device side
# ---------------------------------------------------------------------------------------
def bytes_batch(amq, torch, items):
    """Offsets form of any list of byte strings (empty ones and an empty list included)."""
    offs = np.zeros(len(items) + 1, np.int64)
    offs[1:] = np.cumsum([len(x) for x in items])
    blob = np.frombuffer(b"".join(items), np.uint8)
    data = dev(torch, blob.copy()) if len(blob) else torch.zeros(0, dtype=torch.uint8, device="cuda")
    return amq.KeyBatch.variable(data, dev(torch, offs))


class Run:
    """One side of a merge: the host's keys and values and their device arrays.  key_form: "fixed"
    (every key of one length, `shift` bytes past an aligned address) or "var"; value_form: "offsets"
    or "stride" (every value of one length)."""

    def __init__(self, amq, torch, keys, values, key_form="fixed", value_form="offsets", shift=0):
        assert len(keys) == len(values)
        self.keys, self.values, self.n = list(keys), list(values), len(keys)
        if key_form == "fixed":
            (length,) = {len(k) for k in keys}
            self.kb = fixed_batch(amq, torch, self.keys, length, shift)
        else:
            self.kb = bytes_batch(amq, torch, self.keys)
        if value_form == "stride":
            (length,) = {len(v) for v in values}
            self.vb = fixed_batch(amq, torch, self.values, length)
        else:
            self.vb = bytes_batch(amq, torch, self.values)

    def run(self, amq, d_begin=None):
        return amq.merge_run(self.kb, self.vb, d_begin)


def read_guarded(pair, name=""):
    raw = pair[0].cpu().numpy()
    bts, g = raw.view(np.uint8), GUARD * raw.itemsize
    assert (bts[:g] == CANARY).all() and (bts[len(bts) - g:] == CANARY).all(), name
    return raw[GUARD:len(raw) - GUARD]


def launch_merge(amq, torch, N, O, nb, ob, decay, capacity, bufs=None, stream=None):
    n_jobs = len(nb) - 1
    if bufs is None:
        bufs = {"begin": guarded(torch, n_jobs + 1, torch.int64), "items": guarded(torch, 16 * capacity, torch.uint8),
                "needed": guarded(torch, 1, torch.int64), "counts": guarded(torch, len(COUNTS), torch.int64),
                "ws": (None, torch.empty(amq.merge_leaves_workspace_bytes(n_jobs, N.n, O.n), dtype=torch.uint8,
                                         device="cuda")),
                "nb": (None, dev(torch, np.asarray(nb, np.uint64).view(np.int64))),
                "ob": (None, dev(torch, np.asarray(ob, np.uint64).view(np.int64)))}
        bufs["counts"][1].zero_()
    assert bufs["items"][1].data_ptr() % 16 == 0
    amq.merge_leaves_device(N.run(amq, bufs["nb"][1]), O.run(amq, bufs["ob"][1]), n_jobs, bufs["begin"][1],
                            bufs["items"][1], capacity, bufs["ws"][1], bufs["needed"][1],
                            amq.abi.MERGE_DECAY_TO_ITEMS if decay else 0, bufs["counts"][1], stream)
    return bufs


def read_merge(amq, torch, bufs):
    torch.cuda.synchronize()
    got = {name: read_guarded(bufs[name], name) for name in ("begin", "items", "needed", "counts")}
    got["rec"] = got.pop("items").view(amq.abi.MERGE_ITEM_DTYPE)
    return got


def same_merge(amq, got, want, capacity):
    recs, begin, counts = want
    rec = record_array(amq, recs)
    w = min(len(rec), capacity)
    assert np.array_equal(got["begin"], begin)                   # exact whatever the capacity
    assert int(got["needed"][0]) == len(rec)
    assert dict(zip(COUNTS, (int(v) for v in got["counts"]))) == counts
    for name in ("src", "i32", "op", "flags", "reserved"):
        assert np.array_equal(got["rec"][name][:w], rec[name][:w]), name
    assert (got["rec"][w:].view(np.uint8) == CANARY).all()        # nothing at or past min(total, capacity)


def launch_gather(amq, torch, d_items, d_begin, n_jobs, capacity, N, O, fixed, k_cap, v_cap, bufs=None, stream=None):
    """tkv_amq_gather_merged into guarded outputs.  The value bytes start one byte past an aligned address, so the
    mover's byte tail runs; the key bytes start aligned."""
    if bufs is None:
        whole_v = torch.full((v_cap + 2 * 256 + 1,), CANARY, dtype=torch.uint8, device="cuda")
        bufs = {"keys": guarded(torch, k_cap, torch.uint8), "values": (whole_v, whole_v[257:257 + v_cap]),
                "koffs": None if fixed else guarded(torch, capacity + 1, torch.int64),
                "voffs": guarded(torch, capacity + 1, torch.int64), "needed": guarded(torch, 2, torch.int64),
                "ws": (None, torch.empty(amq.gather_merged_workspace_bytes(capacity), dtype=torch.uint8, device="cuda"))}
    amq.gather_merged_device(d_items, d_begin, n_jobs, capacity, N.run(amq), O.run(amq), bufs["keys"][1],
                             N.kb.stride if fixed else 0, None if fixed else bufs["koffs"][1], k_cap, bufs["values"][1],
                             bufs["voffs"][1], v_cap, bufs["ws"][1], bufs["needed"][1], stream)
    return bufs


def read_gather(torch, bufs, v_cap):
    torch.cuda.synchronize()
    got = {name: read_guarded(bufs[name], name) for name in ("keys", "koffs", "voffs", "needed") if bufs[name] is not None}
    raw = bufs["values"][0].cpu().numpy()
    assert (raw[:257] == CANARY).all() and (raw[257 + v_cap:] == CANARY).all()
    got["values"] = raw[257:257 + v_cap]
    return got


def same_bytes(out, offs, items, cap, stride=0):
    """Items wholly below `cap` are written where the exact offsets put them; no other byte is."""
    want = np.full(len(out), CANARY, np.uint8)
    at = 0
    for p, item in enumerate(items):
        if offs is not None:
            assert int(offs[p]) == at
        elif len(item) != stride:                                 # (a fixed slot takes a key of its size or nothing)
            at += stride
            continue
        if at + len(item) <= cap:
            want[at:at + len(item)] = np.frombuffer(item, np.uint8)
        at += len(item)
    if offs is not None:
        assert int(offs[len(items)]) == at
        assert (offs[len(items) + 1:].view(np.uint8) == CANARY).all()
    assert np.array_equal(out, want)
    return at


def same_gather(got, keys, values, k_cap, v_cap, stride=0):
    k_total = same_bytes(got["keys"], got.get("koffs"), keys, k_cap, stride)
    v_total = same_bytes(got["values"], got["voffs"], values, v_cap)
    assert [int(x) for x in got["needed"]] == [k_total, v_total]


def fixed_out(N, O):
    return N.kb.offsets is None and O.kb.offsets is None and N.kb.stride == O.kb.stride


def check(amq, torch, N, O, nb, ob, decay, capacity=None, k_cap=None, v_cap=None):
    """Merge and gather against the model; the capacities default to what holds everything."""
    want = model_batch(N, O, nb, ob, decay)
    recs = want[0]
    capacity = len(recs) + 3 if capacity is None else capacity
    bufs = launch_merge(amq, torch, N, O, nb, ob, decay, capacity)
    same_merge(amq, read_merge(amq, torch, bufs), want, capacity)
    keys, values = model_gather(recs[:capacity], N, O)
    fixed = fixed_out(N, O)
    k_cap = sum(len(k) for k in keys) + 5 if k_cap is None else k_cap
    v_cap = sum(len(v) for v in values) + 5 if v_cap is None else v_cap
    g = launch_gather(amq, torch, bufs["items"][1], bufs["begin"][1], len(nb) - 1, capacity, N, O, fixed, k_cap, v_cap)
    same_gather(read_gather(torch, g, v_cap), keys, values, k_cap, v_cap, N.kb.stride if fixed else 0)
    return want


def i32(x, width=4):
    return int(x).to_bytes(width, "little", signed=True)


def begins(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


# ---------------------------------------------------------------------------------------
# 1. the op table
# ---------------------------------------------------------------------------------------
OPS = (DELETE, NOOP, WRITE, ADD, PAGE_SLICE, UNKNOWN, None)       # None: the empty value


def table_value(op, x):
    return b"" if op is None else bytes([op]) + i32(x)


@pytest.mark.parametrize("decay", [False, True])
def test_the_op_table_on_the_device(amq, torch, decay):
    """One job: every ordered (newer, older) pair of the five ops, an unknown op and the empty value on a key of its
    own -- the 27 cases of the header's table among them."""
    pairs = [(a, b) for a in OPS for b in OPS]
    keys = [key16(3 * j) for j in range(len(pairs))]
    N = Run(amq, torch, keys, [table_value(a, 1000 + 7 * j) for j, (a, b) in enumerate(pairs)])
    O = Run(amq, torch, keys, [table_value(b, -40 - j) for j, (a, b) in enumerate(pairs)])
    recs, begin, counts = check(amq, torch, N, O, [0, N.n], [0, O.n], decay)
    assert counts["pair_count"] == len(pairs) and counts["combined_count"] == 3 and counts["bad_combine_count"] == 4
    assert counts["dropped_count"] == (4 * 7 if decay else 0)


# ---------------------------------------------------------------------------------------
# 2. key and value shapes
# ---------------------------------------------------------------------------------------
def pool(shape, rng, n):
    """n distinct sorted keys: fixed lengths, or 1..40 bytes over two letters with every key's proper prefixes
    likely among them (the shorter sorts first)."""
    if shape != "var":
        length = {"k16": 16, "k24": 24, "k11": 11}[shape]
        return sorted({bytes(rng.integers(0, 256, length, dtype=np.uint8)) for _ in range(n)})
    keys = set()
    while len(keys) < n:
        k = bytes(rng.integers(97, 99, int(rng.integers(1, 41)), dtype=np.uint8))
        keys.update((k, k[:max(1, len(k) // 2)], k[:-1] or k))
    return sorted(keys)


def random_value(rng, form):
    op = int(rng.choice([DELETE, NOOP, WRITE, WRITE, ADD, ADD, PAGE_SLICE, UNKNOWN]))
    if form == "stride":
        return bytes([op]) + i32(int(rng.integers(-1 << 31, 1 << 31)))
    if rng.random() < 0.1:
        return b""
    return bytes([op]) + bytes(rng.integers(0, 256, int(rng.integers(0, 9)), dtype=np.uint8))


def random_jobs(rng, keys, n_jobs, share=0.4):
    """Per job a sorted slice of the pool split into a newer and an older run that share about `share` of it."""
    newer, older = [], []
    for part in np.array_split(np.arange(len(keys)), n_jobs):
        pick = rng.random(len(part))
        newer.append([keys[i] for i, p in zip(part, pick) if p < 0.3 + share / 2])
        older.append([keys[i] for i, p in zip(part, pick) if p > 0.3 - share / 2])
    return newer, older


def flat(runs):
    return [k for r in runs for k in r]


SHAPES = {  # name: (pool, newer key form, older key form, newer shift)
    "k16": ("k16", "fixed", "fixed", 0), "k16_misaligned": ("k16", "fixed", "fixed", 8), "k24": ("k24", "fixed", "fixed", 0),
    "k11": ("k11", "fixed", "fixed", 0), "var": ("var", "var", "var", 0), "fixed_over_var": ("k16", "fixed", "var", 0),
    "var_over_fixed": ("k24", "var", "fixed", 0)}


@pytest.mark.parametrize("value_form", ["offsets", "stride"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_key_and_value_shapes(amq, torch, shape, value_form):
    which, nf, of, shift = SHAPES[shape]
    rng = np.random.default_rng(sorted(SHAPES).index(shape) * 2 + (value_form == "stride"))
    newer, older = random_jobs(rng, pool(which, rng, 1300), 4)
    assert all(150 < len(a) + len(b) for a, b in zip(newer, older))
    if shape == "var":
        ks = set(flat(newer)) | set(flat(older))
        assert any(k[:-1] in ks for k in ks if len(k) > 1)          # keys that are prefixes of one another
    # (the newer values in one form, the older in the other: the two sides' forms are independent)
    other = "offsets" if value_form == "stride" else "stride"
    N = Run(amq, torch, flat(newer), [random_value(rng, value_form) for _ in flat(newer)], nf, value_form, shift)
    O = Run(amq, torch, flat(older), [random_value(rng, other) for _ in flat(older)], of, other)
    nb, ob = begins([len(r) for r in newer]), begins([len(r) for r in older])
    for decay in (False, True):
        recs, begin, counts = check(amq, torch, N, O, nb, ob, decay)
        assert counts["pair_count"] > 50 and counts["combined_count"] > 0 and counts["bad_combine_count"] > 0


# ---------------------------------------------------------------------------------------
# 3. edges of the jobs
# ---------------------------------------------------------------------------------------
def edge_jobs(rng):
    """(newer keys, older keys, value of a newer key, value of an older key) per job."""
    rnd = lambda k: random_value(rng, "offsets")
    dele = lambda k: bytes([DELETE])
    noop = lambda k: b""
    wr = lambda k: bytes([WRITE]) + k[13:]
    K = lambda *xs: [key16(x) for x in xs]
    jobs = [(K(), K(1, 2, 3), rnd, rnd), (K(1, 2, 3), K(), rnd, rnd), (K(), K(), rnd, rnd),
            (K(4, 5, 6, 7), K(4, 5, 6, 7), rnd, rnd), (K(1, 3, 5), K(2, 4, 6, 8), rnd, rnd),
            (K(*range(0, 40, 2)), K(3, 4, 33), rnd, rnd),                               # the newer run the longer
            (K(1, 9), K(1, 5, 7), rnd, rnd), (K(2, 9), K(1, 5, 9), rnd, rnd),           # a pair first, a pair last
            (K(5), K(5), rnd, rnd), (K(5), K(), rnd, rnd), (K(), K(5), rnd, rnd),
            (K(1, 2, 3), K(7, 8), wr, wr), (K(1, 4, 6), K(2, 4, 5, 6), dele, noop),     # every item decays ...
            (K(7, 8), K(1, 2, 3), wr, wr)]                                              # ... between non-empty jobs
    for _ in range(26):
        keys = sorted(int(x) for x in rng.choice(200, int(rng.integers(2, 40)), replace=False))
        pick = rng.random(len(keys))
        jobs.append((K(*[x for x, p in zip(keys, pick) if p < 0.6]), K(*[x for x, p in zip(keys, pick) if p > 0.4]),
                     rnd, rnd))
    jobs.append((K(10, 20, 30), K(10, 25, 30, 40), wr, wr))
    return jobs


@pytest.mark.parametrize("decay", [False, True])
def test_edges_of_the_jobs(amq, torch, decay):
    rng = np.random.default_rng(11)
    jobs = edge_jobs(rng)
    tail = [key16(500 + x) for x in range(6)]                         # items behind the last job's
    N = Run(amq, torch, flat(j[0] for j in jobs) + tail, [j[2](k) for j in jobs for k in j[0]] + [bytes([WRITE])] * 6)
    O = Run(amq, torch, flat(j[1] for j in jobs) + tail[:4], [j[3](k) for j in jobs for k in j[1]] + [bytes([ADD, 1])] * 4)
    nb, ob = begins([len(j[0]) for j in jobs]), begins([len(j[1]) for j in jobs])
    # two more jobs: an end below its begin (empty), then one that reaches back into the last job's items and past
    # the run's end -- it reads what the run's item count leaves it
    nb = np.array([int(x) for x in nb] + [int(nb[-1]) - 2, 1 << 40], np.uint64)
    ob = np.array([int(x) for x in ob] + [int(ob[-1]) - 3, (1 << 64) - 1], np.uint64)
    want = check(amq, torch, N, O, nb, ob, decay)
    sizes = np.diff(want[1])
    assert sizes[-2] == 0 and sizes[-1] > 0
    if decay:
        assert sizes[12] == 0 and sizes[11] > 0 and sizes[13] > 0
    # and with the begin arrays past everything: every job empty
    far = np.full(len(nb), 1 << 50, np.int64)
    recs, begin, counts = check(amq, torch, N, O, far, far, decay)
    assert not recs and counts["newer_count"] == 0


def test_no_jobs(amq, torch):
    N = Run(amq, torch, [key16(1)], [b"\x02a"])
    bufs = launch_merge(amq, torch, N, N, [0], [0], False, 4)
    got = read_merge(amq, torch, bufs)
    assert int(got["begin"][0]) == 0 and int(got["needed"][0]) == 0 and not got["counts"].any()
    assert (got["rec"].view(np.uint8) == CANARY).all()


# ---------------------------------------------------------------------------------------
# 4. work unit boundaries
# ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big_case(amq, torch):
    """One job of 60,000 older and 9,000 newer items among 50 small ones; every third newer key of the big job is a
    pair, so pairs straddle the work units whatever their size."""
    rng = np.random.default_rng(23)
    small_n, small_o = random_jobs(rng, [key16(x) for x in range(0, 5000, 3)], 50)
    big_o = [key16(10 ** 6 + 5 * x) for x in range(60000)]

    def newer_key(x):                                             # every third one a multiple of 5, the others not
        v = 33 * x
        if x % 3 == 0:
            return v - v % 5
        return v + 2 if (v + 1) % 5 == 0 else v + 1

    big_n = [key16(10 ** 6 + newer_key(x)) for x in range(9000)]
    assert big_n == sorted(set(big_n)) and 2900 < len(set(big_n) & set(big_o)) < 3100
    newer, older = small_n[:20] + [big_n] + small_n[20:], small_o[:20] + [big_o] + small_o[20:]
    ops = [DELETE, WRITE, ADD, ADD, NOOP, PAGE_SLICE]
    N = Run(amq, torch, flat(newer), [bytes([ops[j % 6]]) + i32(j) for j in range(len(flat(newer)))], value_form="stride")
    O = Run(amq, torch, flat(older), [bytes([ops[j % 5]]) + i32(-j) for j in range(len(flat(older)))], value_form="stride")
    return N, O, begins([len(r) for r in newer]), begins([len(r) for r in older])


@pytest.mark.parametrize("decay", [False, True])
def test_pairs_across_unit_boundaries(amq, torch, big_case, decay):
    N, O, nb, ob = big_case
    recs, begin, counts = check(amq, torch, N, O, nb, ob, decay)
    assert counts["pair_count"] > 3000 and counts["combined_count"] > 100   # (the inputs hold what the test is about)


# ---------------------------------------------------------------------------------------
# 5. short capacities
# ---------------------------------------------------------------------------------------
def test_short_capacities(amq, torch):
    rng = np.random.default_rng(31)
    newer, older = random_jobs(rng, pool("var", rng, 900), 5)
    N = Run(amq, torch, flat(newer), [random_value(rng, "offsets") for _ in flat(newer)], "var")
    O = Run(amq, torch, flat(older), [random_value(rng, "offsets") for _ in flat(older)], "var")
    nb, ob = begins([len(r) for r in newer]), begins([len(r) for r in older])
    recs, begin, counts = model_batch(N, O, nb, ob, False)
    keys, values = model_gather(recs, N, O)
    check(amq, torch, N, O, nb, ob, False, capacity=len(recs) // 2)   # the records: half; the gather: of those
    check(amq, torch, N, O, nb, ob, False, k_cap=sum(map(len, keys)) // 2)
    check(amq, torch, N, O, nb, ob, False, v_cap=sum(map(len, values)) // 2)
    check(amq, torch, N, O, nb, ob, False, capacity=0, k_cap=0, v_cap=0)
    # the fixed key form: slots below the capacity, whole
    rng = np.random.default_rng(32)
    newer, older = random_jobs(rng, pool("k11", rng, 300), 2)
    N = Run(amq, torch, flat(newer), [random_value(rng, "stride") for _ in flat(newer)], value_form="stride")
    O = Run(amq, torch, flat(older), [random_value(rng, "stride") for _ in flat(older)], value_form="stride")
    nb, ob = begins([len(r) for r in newer]), begins([len(r) for r in older])
    check(amq, torch, N, O, nb, ob, True, k_cap=11 * 100 + 5)


# ---------------------------------------------------------------------------------------
# 6. records the gather does not trust
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("fixed", [False, True])
def test_forged_records_give_empty_items(amq, torch, fixed):
    keys = [key16(x) for x in range(5)]
    N = Run(amq, torch, keys[:3], [b"\x02new%d" % j for j in range(3)], "fixed" if fixed else "var")
    O = Run(amq, torch, keys, [b"\x02older%d" % j for j in range(5)])
    recs = [(0, 0, WRITE, 0), (3, 0, WRITE, 0), (OLDER | 4, 0, WRITE, 0), (OLDER | 5, 0, WRITE, 0),
            ((1 << 63) - 1, 7, WRITE, COMBINED), (OLDER | (1 << 62), 0, ADD, 0), (2, -9, ADD, COMBINED),
            ((1 << 64) - 1, 0, DELETE, 0)]
    d_items = dev(torch, np.frombuffer(record_array(amq, recs).tobytes(), np.uint8).copy())
    d_begin = dev(torch, np.array([0, 2, len(recs)], np.int64))
    want_k, want_v = model_gather(recs, N, O)
    assert want_k[1] == want_k[3] == b"" and want_v[4] == b"" and want_v[6] == bytes([ADD]) + i32(-9)
    g = launch_gather(amq, torch, d_items, d_begin, 2, len(recs), N, O, fixed, 16 * len(recs) + 3, 100)
    same_gather(read_gather(torch, g, 100), want_k, want_v, 16 * len(recs) + 3, 100, 16 if fixed else 0)
    # a forged total: no more records are gathered than the capacity, or than the runs have items
    d_begin = dev(torch, np.array([0, 2, 1 << 40], np.int64))
    g = launch_gather(amq, torch, d_items, d_begin, 2, len(recs) - 1, N, O, fixed, 16 * len(recs), 100)
    same_gather(read_gather(torch, g, 100), want_k[:-1], want_v[:-1], 16 * len(recs), 100, 16 if fixed else 0)


# ---------------------------------------------------------------------------------------
# 7. runs that are not sorted
# ---------------------------------------------------------------------------------------
def test_unsorted_runs_stay_inside_their_jobs(amq, torch):
    """No merge answer is asserted: the call returns, nothing outside the outputs is written, the counts add up and
    every record that was written names an item of its own job."""
    rng = np.random.default_rng(41)
    sizes_n, sizes_o = [int(x) for x in rng.integers(0, 900, 12)], [int(x) for x in rng.integers(0, 3000, 12)]
    N = Run(amq, torch, [key16(int(x)) for x in rng.integers(0, 500, sum(sizes_n))], [b"\x03\x01"] * sum(sizes_n))
    O = Run(amq, torch, [key16(int(x)) for x in rng.integers(0, 500, sum(sizes_o))], [b"\x02\x01"] * sum(sizes_o))
    nb, ob = begins(sizes_n), begins(sizes_o)
    capacity = N.n + O.n
    for decay in (False, True):
        got = read_merge(amq, torch, launch_merge(amq, torch, N, O, nb, ob, decay, capacity))
        begin, c = got["begin"], dict(zip(COUNTS, (int(v) for v in got["counts"])))
        assert begin[0] == 0 and (np.diff(begin) >= 0).all() and begin[-1] == got["needed"][0] == c["out_count"] <= capacity
        assert c["newer_count"] == N.n and c["older_count"] == O.n
        assert c["out_count"] == N.n + O.n - c["pair_count"] - c["dropped_count"]
        for j in range(12):
            rec = got["rec"][begin[j]:begin[j + 1]]
            written = rec[(rec.view(np.uint8).reshape(-1, 16) != CANARY).any(axis=1)]
            idx, older = written["src"] & np.uint64(OLDER - 1), (written["src"] >> np.uint64(63)).astype(bool)
            lo, hi = np.where(older, ob[j], nb[j]), np.where(older, ob[j + 1], nb[j + 1])
            assert ((idx >= lo) & (idx < hi)).all()
        assert (got["rec"][begin[-1]:].view(np.uint8) == CANARY).all()
        # and the gather over whatever the records hold
        g = launch_gather(amq, torch, launch_merge(amq, torch, N, O, nb, ob, decay, capacity)["items"][1],
                          dev(torch, begin.copy()), 12, capacity, N, O, True, 16 * capacity, 8 * capacity)
        read_gather(torch, g, 8 * capacity)


# ---------------------------------------------------------------------------------------
# 8. graph capture: the merge and the gather as one linear chain
# ---------------------------------------------------------------------------------------
def test_merge_and_gather_replay_in_a_graph(amq, torch):
    rng = np.random.default_rng(51)
    newer, older = random_jobs(rng, pool("k16", rng, 1200), 6)
    nvals = [bytes([ADD]) + i32(j) for j, _ in enumerate(flat(newer))]
    ovals = [bytes([(WRITE, DELETE, ADD)[j % 3]]) + i32(5 * j) for j, _ in enumerate(flat(older))]
    N, O = Run(amq, torch, flat(newer), nvals, value_form="stride"), Run(amq, torch, flat(older), ovals)
    nb, ob = begins([len(r) for r in newer]), begins([len(r) for r in older])
    capacity, k_cap, v_cap = N.n + O.n, 16 * (N.n + O.n), 9 * (N.n + O.n)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    bufs = launch_merge(amq, torch, N, O, nb, ob, False, capacity, stream=s)
    g = launch_gather(amq, torch, bufs["items"][1], bufs["begin"][1], len(nb) - 1, capacity, N, O, True, k_cap, v_cap,
                      stream=s)
    s.synchronize()

    def both():
        launch_merge(amq, torch, N, O, nb, ob, False, capacity, bufs, s)
        launch_gather(amq, torch, bufs["items"][1], bufs["begin"][1], len(nb) - 1, capacity, N, O, True, k_cap, v_cap, g, s)

    def verify(times):
        recs, begin, counts = want = model_batch(N, O, nb, ob, False)
        want = (recs, begin, {k: v * times for k, v in counts.items()})
        same_merge(amq, read_merge(amq, torch, bufs), want, capacity)
        keys, values = model_gather(recs, N, O)
        same_gather(read_gather(torch, g, v_cap), keys, values, k_cap, v_cap, 16)

    verify(1)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        both()
    for turn in range(2):                                         # the inputs changed in place, the outputs refilled
        swap = [bytes([(WRITE, ADD, DELETE)[(j + turn) % 3]]) + i32(turn - j) for j in range(N.n)]
        N.values = swap
        N.vb.data.copy_(torch.from_numpy(np.frombuffer(b"".join(swap), np.uint8).copy()).view(N.n, 5))
        moved = sorted(older[turn])[:-1] + [b"\xff" * 15 + bytes([turn])]   # one job's older run gets another last key
        at = int(ob[turn])
        O.keys[at:at + len(moved)] = moved
        O.kb.data[at:at + len(moved)].copy_(torch.from_numpy(np.frombuffer(b"".join(moved), np.uint8).copy()).view(-1, 16))
        bufs["counts"][1].zero_()
        for name in ("begin", "items", "needed"):
            bufs[name][1].view(torch.uint8).fill_(CANARY)
        for name in ("keys", "values", "voffs", "needed"):
            g[name][1].view(torch.uint8).fill_(CANARY)
        torch.cuda.synchronize()
        graph.replay()
        verify(1)


# ---------------------------------------------------------------------------------------
# 9. closing the loop: update -> merged leaves -> filters -> verified -> looked up, all on the device
# ---------------------------------------------------------------------------------------
def test_closing_the_loop(amq, torch):
    rng = np.random.default_rng(61)
    leaves = [[key16(1000 * li + 2 * x) for x in range(500 - 7 * li)] for li in range(3)]
    old_vals = [[bytes([WRITE]) + i32(int(rng.integers(-1000, 1000))) + b"payload-%d" % x for x in range(len(lv))]
                for lv in leaves]
    store = {k: v for lv, vs in zip(leaves, old_vals) for k, v in zip(lv, vs)}
    # the update touches leaves 0 and 2: writes, deletes and deltas on keys that exist and keys that do not
    update = [[], [], []]
    for li in (0, 2):
        for x in sorted(int(v) for v in rng.choice(1000, 160, replace=False)):
            op = (WRITE, DELETE, ADD)[x % 3]
            update[li].append((key16(1000 * li + x), bytes([op]) + (i32(x - 300) if op != DELETE else b"")))
    want = {}                                                     # key -> ("delete",) | ("sum", n) | ("bytes", value)
    for k, v in store.items():
        want[k] = ("bytes", v)
    for k, v in flat(update):
        op, data = unpack(v)
        if op == WRITE:
            want[k] = ("bytes", v)
        elif op == DELETE:
            want[k] = ("delete",)
        elif k in store:                                           # a delta over a WRITE
            want[k] = ("sum", signed(as_i32(data) + as_i32(store[k][1:])))
        else:
            want[k] = ("bytes", v)                                 # a delta with nothing below it stays a delta
    N = Run(amq, torch, [k for k, v in flat(update)], [v for k, v in flat(update)])
    O = Run(amq, torch, flat(leaves), flat(old_vals))
    r = amq.merge_leaves(N.kb, N.vb, begins([len(u) for u in update]), O.kb, O.vb, begins([len(lv) for lv in leaves]))
    out_begin = r.out_begin.cpu().numpy()
    assert r.counts["out_count"] == len(want) == out_begin[-1] and r.counts["dropped_count"] == 0
    assert r.counts["combined_count"] == sum(1 for w in want.values() if w[0] == "sum") > 10
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
                assert stored == bytes([WRITE]) + i32(state[1]) and one["op"] == WRITE
                assert lens[q] == 4 and bytes(slots[q][:4]) == i32(state[1])
            else:
                assert stored == state[1] and one["op"] == state[1][0]
                assert lens[q] == len(state[1]) - 1 and bytes(slots[q][:lens[q]]) == state[1][1:]
