"""CPU-only: the route tkv_amq_build / tkv_amq_build_ex take (tkv_amq_build_route), pinned on
both sides of every constant that decides it, and checked against the workspace tkv_amq_plan
sizes.  The expectations restate the rules the builds had before the routes got one chooser
("Build routes"); none is read back from the library.

Blocks are 64 bytes; one workgroup's LDS image holds 2,560 of them (160 KiB), a window as many,
a tile 2,048.  At 10 bits/key n keys make ceil(n * 10 / 512) blocks and k = 7."""
import ctypes

import numpy as np
import pytest

UNLIMITED = 1 << 62
BLOOM, VQF = 0, 1
LDS_BLOCKS = 2560

# key shapes: (stride, has_offsets, aligned8)
SHAPES = {"k16": (16, 0, 1), "k24": (24, 0, 1), "k24u": (24, 0, 0), "k20": (20, 0, 1), "var": (0, 1, 1)}
TILED_KEY_SHAPES = ("k16", "k24")


def route(amq, kind, n_segs, n_keys, max_blocks, shape="k16", ws=UNLIMITED, segs=None):
    """tkv_amq_build_route; ws None: no workspace.  With segs: (route, leaf routes)."""
    A = amq.abi
    stride, var, al = SHAPES[shape]
    out = A.BuildRoute()
    leaves = np.full(n_segs, 255, dtype=np.uint8)
    st = A.lib().tkv_amq_build_route(kind, stride, var, al, n_segs, n_keys, max_blocks,
                                     None if segs is None else segs.ctypes.data_as(ctypes.c_void_p),
                                     0 if ws is None else 1, 0 if ws is None else ws, ctypes.byref(out),
                                     leaves.ctypes.data_as(ctypes.c_void_p))
    assert st == A.OK, st
    return (out, leaves) if segs is not None else out


def blocks(n, bpk):
    return max(1, -(-n * bpk // 512))


def hash_count(bpk):
    return min(32, max(1, int(bpk * 0.69314718055994530942 + 0.5)))


# ---- the parts per leaf, restated from the rules (bloom_split_parts, bloom_window_parts) ----
def split_parts(n_segs, n_keys, mb):
    if n_segs >= 256 or mb > LDS_BLOCKS:
        return 1
    p = min(-(-1024 // n_segs), n_keys // n_segs // 1024, 16)
    return p if p >= 2 else 1


def window_parts(n_segs, n_keys, mb):
    W = -(-mb // LDS_BLOCKS)
    wblk = -(-mb // W)
    G = 256 * (2 if 64 * wblk <= 80 * 1024 else 1)
    max_p = max(1, min(16, n_keys // n_segs // 4096))
    best, best_cost = 1, 1e30
    for p in range(1, max_p + 1):
        cost = -(-(n_segs * W * p) // G) / p + (0.03 * p if p > 1 else 0.0)
        if cost < best_cost - 1e-9:
            best, best_cost = p, cost
    return best


def one(n, bpk):
    """(n_segs, n_keys, max_blocks) of one filter"""
    return 1, n, blocks(n, bpk)


def batch(n_segs, per_leaf, bpk=10):
    return n_segs, n_segs * per_leaf, blocks(per_leaf, bpk)


S, W, L, TK, TR, AT = "SPLIT", "WINDOW", "LDS", "TILED_KEYS", "TILED_RECORDS", "ATOMICS"

# (what the case pins, (n_segs, n_keys, max_blocks), shape, workspace, route, fields)
BLOOM_TABLE = [
    # kBloomSpreadSegs 64: one workgroup per leaf from 64 leaves (1,000 keys each: no split)
    ("spread 63", batch(63, 1000), "k16", UNLIMITED, AT, {}),
    ("spread 64", batch(64, 1000), "k16", UNLIMITED, L, {"threads": 1024}),
    # kBloomSplitSegs 256: below, leaves of >= 2,048 keys are split (1,024 / n_segs workgroups,
    # 1,024 keys each at least); without the workspace they are not
    ("split 255", batch(255, 4096), "var", UNLIMITED, S, {"parts": 4, "ws_bytes": 255 * 4 * 64 * 80}),
    ("split 255 short", batch(255, 4096), "var", 255 * 4 * 64 * 80 - 1, L, {"threads": 1024}),
    ("split 255 none", batch(255, 4096), "var", None, L, {"threads": 1024}),
    ("split 256", batch(256, 4096), "var", UNLIMITED, L, {"threads": 1024, "ws_bytes": 0}),
    # kBloomWideSegs 2048 and kBloomWideLds (512 blocks): 256-thread workgroups
    ("wide 2047", (2047, 2047 * 1000, 512), "k24", UNLIMITED, L, {"threads": 1024}),
    ("wide 2048 x 512", (2048, 2048 * 1000, 512), "k24", UNLIMITED, L, {"threads": 256, "lds_bytes": 32768}),
    ("wide 2048 x 513", (2048, 2048 * 1000, 513), "k24", UNLIMITED, L, {"threads": 1024}),
    # kSplitMinKeys: two parts need 2,048 keys per leaf
    ("min keys 2047", batch(100, 2047), "k16", UNLIMITED, L, {}),
    ("min keys 2048", batch(100, 2048), "k16", UNLIMITED, S, {"parts": 2}),
    ("min keys 2047 one", one(2047, 10), "k16", UNLIMITED, AT, {}),
    ("min keys 2048 one", one(2048, 10), "k16", UNLIMITED, S, {"parts": 2, "ws_bytes": 2 * 64 * 40}),
    ("min keys 2048 one none", one(2048, 10), "k16", None, AT, {}),
    # one LDS image (2,560 blocks) against two windows
    ("image 2560", (300, 300 * 131072, 2560), "k20", UNLIMITED, L, {"threads": 1024, "lds_bytes": 163840}),
    ("image 2561", (300, 300 * 131073, 2561), "k20", UNLIMITED, W,
     {"windows": 2, "parts": window_parts(300, 300 * 131073, 2561), "lds_bytes": 64 * 1281}),
    ("image 2561 none", (300, 300 * 131073, 2561), "k20", None, W, {"windows": 2, "parts": 1, "ws_bytes": 0}),
    ("image 2560 split", (70, 70 * 131072, 2560), "k16", UNLIMITED, S, {"parts": 15}),
    ("image 2561 few", (70, 70 * 131073, 2561), "k16", UNLIMITED, W,
     {"windows": 2, "parts": window_parts(70, 70 * 131073, 2561)}),
    # kWinMaxWindows 16 (40,960 blocks): past it a batch's leaves get device atomics
    ("windows 16", (3, 3 * 2097152, 40960), "var", UNLIMITED, W, {"windows": 16}),
    ("windows 17", (3, 3 * 2097153, 40961), "var", UNLIMITED, AT, {}),
    ("windows 16 k16", (3, 3 * 2097152, 40960), "k16", UNLIMITED, W, {"windows": 16}),
    # one filter of two windows: the tiled build for 16-byte and aligned 24-byte keys, windows
    # for every other shape, and for all without a workspace
    ("one x2 k16", one(200_000, 10), "k16", UNLIMITED, TK, {}),
    ("one x2 k24", one(200_000, 10), "k24", UNLIMITED, TK, {}),
    ("one x2 k24u", one(200_000, 10), "k24u", UNLIMITED, W, {"windows": 2}),
    ("one x2 k20", one(200_000, 10), "k20", UNLIMITED, W, {"windows": 2}),
    ("one x2 var", one(200_000, 10), "var", UNLIMITED, W,
     {"windows": 2, "parts": window_parts(1, 200_000, blocks(200_000, 10))}),
    ("one x2 k16 none", one(200_000, 10), "k16", None, W, {"windows": 2, "parts": 1}),
    ("one x2 k24 none", one(200_000, 10), "k24", None, W, {"windows": 2, "parts": 1}),
    ("one x2 var none", one(200_000, 10), "var", None, W, {"windows": 2, "parts": 1}),
    ("one x2 k16 short", one(200_000, 10), "k16", 1 << 16, W, {"windows": 2, "parts": 1}),
    # one filter past 16 windows: tiled, or device atomics without the workspace
    ("one x17 k16", one(2_097_153, 10), "k16", UNLIMITED, TK, {}),
    ("one x17 k16 none", one(2_097_153, 10), "k16", None, AT, {}),
    ("one x17 var", one(2_097_153, 10), "var", UNLIMITED, TR, {}),
    ("one x17 k20", one(2_097_153, 10), "k20", UNLIMITED, TR, {}),
    ("one x17 k24u", one(2_097_153, 10), "k24u", UNLIMITED, TR, {}),
    ("one x17 var none", one(2_097_153, 10), "var", None, AT, {}),
    ("one x17 var short", one(2_097_153, 10), "var", 1 << 20, AT, {}),
    # kDirectMaxTiles 6,400 tiles (13,107,200 blocks; 671,088,640 keys at 10 bits/key, k = 7)
    ("tiles 6400 k24", one(671_088_640, 10), "k24", UNLIMITED, TK, {}),
    ("tiles 6401 k24", one(671_088_641, 10), "k24", UNLIMITED, TK, {}),   # routed as bit records
    ("tiles 6400 var", one(671_088_640, 10), "var", UNLIMITED, TR, {}),
    ("tiles 6401 var", one(671_088_641, 10), "var", UNLIMITED, AT, {}),
    ("tiles 6400 k20", one(671_088_640, 10), "k20", UNLIMITED, TR, {}),
    ("tiles 6401 k20", one(671_088_641, 10), "k20", UNLIMITED, AT, {}),
    ("tiles 6401 k16", one(671_088_641, 10), "k16", UNLIMITED, TK, {}),
    # routed 24-byte keys travel as eight-bit records: k 8 (12 bits/key) against 9 (13)
    ("routed k24 k8", one(560_000_000, 12), "k24", UNLIMITED, TK, {}),
    ("routed k24 k9", one(560_000_000, 13), "k24", UNLIMITED, AT, {}),
    ("routed k16 k9", one(560_000_000, 13), "k16", UNLIMITED, TK, {}),
    ("direct k24 k9", one(500_000_000, 13), "k24", UNLIMITED, TK, {}),   # 6,199 tiles: from the keys
    # records hold up to 16 bits (two per key): k 16 (23 bits/key) against 17 (24)
    ("records k16", one(2_000_000, 23), "var", UNLIMITED, TR, {}),
    ("records k17", one(2_000_000, 24), "var", UNLIMITED, AT, {}),
    ("records k16 k20", one(2_000_000, 23), "k20", UNLIMITED, TR, {}),
    ("records k17 k20", one(2_000_000, 24), "k20", UNLIMITED, AT, {}),
    ("keys k17 k16", one(2_000_000, 24), "k16", UNLIMITED, TK, {}),
    # a filter's keys are counted in 32 bits
    ("keys 2^32-1", (1, (1 << 32) - 1, 83886080), "k16", UNLIMITED, TK, {}),
    ("keys 2^32", (1, 1 << 32, 83886080), "k16", UNLIMITED, AT, {}),
]


@pytest.mark.parametrize("case", BLOOM_TABLE, ids=[c[0] for c in BLOOM_TABLE])
def test_bloom_route_table(amq, case):
    _, (n_segs, n_keys, mb), shape, ws, want, fields = case
    r = route(amq, BLOOM, n_segs, n_keys, mb, shape, ws)
    assert r.route == getattr(amq.abi, "ROUTE_" + want), (r.route, want)
    for f, v in fields.items():
        assert getattr(r, f) == v, (f, getattr(r, f), v)
    assert ws is None or r.ws_bytes <= ws
    if want == S:
        assert r.parts == split_parts(n_segs, n_keys, mb) and r.ws_bytes == n_segs * r.parts * 64 * mb
    if want == W and ws == UNLIMITED:
        assert r.parts == window_parts(n_segs, n_keys, mb)
        assert r.ws_bytes == (n_segs * r.parts * 64 * mb if r.parts > 1 else 0)


def plan(amq, kind, counts, bpk, cap=0):
    return amq.plan_filters(kind, counts, bpk, payload_capacity=cap)


def test_bloom_batch_leaves(amq):
    """tkv_amq_build_ex: in a batch of 16- or 24-byte keys the leaves past kBatchMonoWindows (5)
    windows (12,800 blocks: 655,360 keys at 10 bits/key) leave the batch kernels, in a batch of
    other keys the leaves past kWinMaxWindows (16: 40,960 blocks, 2,097,152 keys)."""
    A = amq.abi
    p = plan(amq, BLOOM, [655_360, 3000, 655_360], 10)
    assert p.max_seg_blocks == 12800
    for shape in SHAPES:
        r, leaves = route(amq, BLOOM, 3, p.n_keys, 12800, shape, p.workspace_bytes, p.segs)
        assert r.route == A.ROUTE_WINDOW and r.windows == 5 and list(leaves) == [A.LEAF_BATCH] * 3
    p = plan(amq, BLOOM, [655_360, 3000, 655_361, 655_360], 10)
    assert p.max_seg_blocks == 12801
    for shape in SHAPES:
        r, leaves = route(amq, BLOOM, 4, p.n_keys, 12801, shape, p.workspace_bytes, p.segs)
        if shape in TILED_KEY_SHAPES:
            assert list(leaves) == [A.LEAF_BATCH, A.LEAF_BATCH, A.LEAF_MULTI, A.LEAF_BATCH]
            assert r.route == A.ROUTE_WINDOW and r.windows == 5
            assert r.parts == window_parts(3, 2 * 655_360 + 3000, 12800)
        else:
            assert list(leaves) == [A.LEAF_BATCH] * 4 and r.route == A.ROUTE_WINDOW and r.windows == 6
    # without the host plan the batch is tkv_amq_build's: windows for every leaf
    assert route(amq, BLOOM, 4, p.n_keys, 12801, "k16", p.workspace_bytes).windows == 6
    p = plan(amq, BLOOM, [2_097_152, 3000, 2_097_152], 10)
    assert p.max_seg_blocks == 40960
    r, leaves = route(amq, BLOOM, 3, p.n_keys, 40960, "var", p.workspace_bytes, p.segs)
    assert r.route == A.ROUTE_WINDOW and r.windows == 16 and list(leaves) == [A.LEAF_BATCH] * 3
    p = plan(amq, BLOOM, [2_097_152, 3000, 2_097_153, 2_097_152], 10)
    assert p.max_seg_blocks == 40961
    for shape in ("k24u", "k20", "var"):
        r, leaves = route(amq, BLOOM, 4, p.n_keys, 40961, shape, p.workspace_bytes, p.segs)
        assert list(leaves) == [A.LEAF_BATCH, A.LEAF_BATCH, A.LEAF_TILED_RECORDS, A.LEAF_BATCH]
        assert r.route == A.ROUTE_WINDOW and r.windows == 16
    # only the leaf list fits: the batch's leaves one part each, the large leaf device atomics
    r, leaves = route(amq, BLOOM, 4, p.n_keys, 40961, "var", 256, p.segs)
    assert leaves[2] == A.LEAF_ATOMICS and r.route == A.ROUTE_WINDOW and r.parts == 1
    r, leaves = route(amq, BLOOM, 4, p.n_keys, 40961, "k16", p.workspace_bytes, p.segs)
    assert list(leaves) == [A.LEAF_MULTI, A.LEAF_BATCH, A.LEAF_MULTI, A.LEAF_MULTI]
    assert r.route == A.ROUTE_SPLIT and r.parts == 2   # (one 3,000-key leaf left in the batch)
    # k = 17 (24 bits/key): no bit records for other key shapes
    p = plan(amq, BLOOM, [900_000, 3000], 24)
    r, leaves = route(amq, BLOOM, 2, p.n_keys, p.max_seg_blocks, "var", p.workspace_bytes, p.segs)
    assert list(leaves) == [A.LEAF_ATOMICS, A.LEAF_BATCH]
    # past kDirectMaxTiles tiles a leaf is tiled alone (14,000,000 blocks: 6,836 tiles)
    p = plan(amq, BLOOM, [716_800_000, 3000], 10)
    _, leaves = route(amq, BLOOM, 2, p.n_keys, p.max_seg_blocks, "k16", p.workspace_bytes, p.segs)
    assert list(leaves) == [A.LEAF_TILED_KEYS, A.LEAF_BATCH]


R1, R2, RING, DEC, U8, GLB = "RING_PLACE", "RING_PLACE2", "RING", "DECIDE", "BIG_U8", "BIG_GLOBAL"
NONE, F512, F256, SC = "NONE", "FUSED512", "FUSED256", "SCATTER"

# (n_segs, max_blocks, shape, decide stage, place stage, fields)
VQF_TABLE = [
    # vqf_ring_place: 256 leaves of <= 960 blocks, then 512 leaves of <= 420
    (256, 960, "k16", R1, NONE, {"threads": 512}),
    (256, 961, "k16", RING, F512, {}),
    (257, 960, "k16", RING, F512, {}),
    (257, 420, "k16", R2, NONE, {}),
    (512, 420, "var", R2, NONE, {"located": 0}),
    (512, 421, "k16", RING, F512, {}),
    (513, 420, "k16", RING, F512, {}),
    # located keys: fixed sizes up to 32 leaves, variable-length up to 64; never 16-byte or
    # aligned 24-byte keys
    (32, 100, "k20", R1, NONE, {"located": 1}),
    (33, 100, "k20", R1, NONE, {"located": 0}),
    (32, 100, "k24u", R1, NONE, {"located": 1}),
    (64, 100, "var", R1, NONE, {"located": 1}),
    (65, 100, "var", R1, NONE, {"located": 0}),
    (1, 100, "k16", R1, NONE, {"located": 0}),
    (1, 100, "k24", R1, NONE, {"located": 0}),
    # vqf_decide_ring: 768 leaves of prefetched keys, 4,096 of others, 2,048 blocks
    (768, 1000, "k16", RING, F512, {"threads": 512}),
    (769, 1000, "k16", DEC, F512, {"threads": 64}),
    (768, 1000, "k24", RING, F512, {}),
    (769, 1000, "k24", DEC, F512, {}),
    (769, 1000, "k24u", RING, F512, {}),
    (4096, 1000, "var", RING, F512, {}),
    (4097, 1000, "var", DEC, F512, {}),
    (4096, 1000, "k20", RING, F512, {}),
    (4097, 1000, "k20", DEC, F512, {}),
    (600, 2048, "k16", RING, F512, {}),
    (600, 2049, "k16", DEC, F512, {}),
    # the count table: u32 in LDS to 16,384 blocks, u8 to 163,840, then the workspace
    (10, 16384, "k16", DEC, SC, {"lds_bytes": 4 * 16384}),
    (10, 16385, "k16", U8, SC, {"lds_bytes": 16400, "threads": 64}),
    (10, 163840, "var", U8, SC, {"lds_bytes": 163840}),
    (10, 163841, "var", GLB, SC, {"lds_bytes": 16}),
    # fused place up to 4 workgroups of 1,241 blocks per leaf
    (10, 4964, "k16", DEC, F512, {"parts": 4}),
    (10, 4965, "k16", DEC, SC, {"parts": 10}),
    (10, 1241, "k16", RING, F512, {"parts": 1}),
    (10, 1242, "k16", RING, F512, {"parts": 2}),
    # 256-thread fused place for a full batch (past 768 leaves) of leaves up to 512 blocks
    (768, 500, "k16", RING, F512, {}),
    (769, 500, "k16", DEC, F256, {}),
    (769, 512, "k16", DEC, F256, {}),
    (769, 513, "k16", DEC, F512, {}),
    (5000, 500, "var", DEC, F256, {}),
]


@pytest.mark.parametrize("case", VQF_TABLE, ids=[f"{c[0]}x{c[1]}-{c[2]}" for c in VQF_TABLE])
def test_vqf_route_table(amq, case):
    n_segs, mb, shape, decide, place, fields = case
    r = route(amq, VQF, n_segs, n_segs * 1000, mb, shape)
    assert r.route == getattr(amq.abi, "ROUTE_VQF_" + decide), (r.route, decide)
    assert r.place == getattr(amq.abi, "PLACE_" + place), (r.place, place)
    for f, v in fields.items():
        assert getattr(r, f) == v, (f, getattr(r, f), v)


def test_vqf_ring_place_match_tables(amq):
    """kRingTblBlocks: up to 512 blocks a one-per-CU ring place adds 7 producers' match tables,
    16 bytes per block (and the dummy block) each, to its LDS; a block's image and count take
    132 bytes, and the count words come in fours (512 and 513 blocks: as many; 511 and 419: four
    fewer)."""
    lds = {mb: route(amq, VQF, 1, 1000, mb).lds_bytes for mb in (511, 512, 513)}
    assert lds[512] - lds[513] == 16 * 7 * 513 - 132
    assert lds[512] - lds[511] == 16 * 7 + 132 + 16
    assert lds[512] <= 160 * 1024
    two = {mb: route(amq, VQF, 300, 1000, mb).lds_bytes for mb in (419, 420)}   # never tables
    assert two[420] - two[419] == 132 + 16 and two[420] <= 80 * 1024


# ---- the plan's workspace never starves the build ----
def random_plan(amq, rng):
    kind = int(rng.integers(0, 2))
    cls = int(rng.integers(0, 5))
    if kind == BLOOM:
        bpk = int(rng.choice([5, 8, 10, 12, 13, 16, 23, 24, 32]))
        if cls == 0:      # many small leaves
            counts = rng.integers(0, 3000, int(rng.integers(1, 3000)))
        elif cls == 1:    # some leaves around one LDS image
            counts = rng.integers(0, 400_000, int(rng.integers(1, 300)))
        elif cls == 2:    # one filter
            counts = [int(rng.integers(1, 1 << int(rng.integers(8, 27))))]
        elif cls == 3:    # a batch with leaves of many windows
            counts = rng.integers(0, 5000, int(rng.integers(2, 14)))
            for i in rng.integers(0, len(counts), int(rng.integers(1, 4))):
                counts[i] = int(rng.integers(100_000, 6_000_000))
        else:             # a huge leaf, alone or beside a few
            counts = [int(rng.integers(300_000_000, 900_000_000))] + [3000] * int(rng.integers(0, 3))
            bpk = int(rng.choice([8, 10, 12, 13]))
        return kind, plan(amq, kind, [int(c) for c in counts], bpk)
    bpk = int(rng.choice([12, 14, 16, 20]))
    if cls == 0 and rng.random() < 0.5:   # 257..512 leaves of up to 420 blocks
        counts = rng.integers(0, 12_000, int(rng.integers(257, 513)))
    elif cls == 0:
        counts = rng.integers(0, 60_000, int(rng.integers(1, 700)))
    elif cls == 1:
        counts = rng.integers(0, 20_000, int(rng.integers(500, 6000)))
    elif cls == 2:
        counts = rng.integers(0, int(rng.choice([30_000, 250_000])), int(rng.integers(1, 40)))
    elif cls == 3:
        counts = [int(rng.integers(600_000, 6_000_000))] + [5000] * int(rng.integers(0, 5))
    else:
        counts = [int(rng.integers(6_000_000, 9_000_000))]
    return kind, plan(amq, kind, [int(c) for c in counts], bpk, cap=1 << 30)


def test_plan_workspace_never_starves_the_build(amq):
    """Over seeded random plans, for every key shape: the route taken with the workspace
    tkv_amq_plan sizes needs no more than it, and is the route taken with unlimited workspace
    (the plan never pushes a build into a fallback).  Every route and leaf route occurs."""
    A = amq.abi
    rng = np.random.default_rng(20240611)
    seen, seen_place, seen_leaf = set(), set(), set()
    fields = ("route", "place", "parts", "windows", "threads", "located", "ws_bytes", "lds_bytes")
    for _ in range(3000):
        kind, p = random_plan(amq, rng)
        if p.n_segs == 0 or p.max_seg_blocks == 0:
            continue
        for shape in SHAPES:
            for segs in (None, p.segs):
                got = route(amq, kind, p.n_segs, p.n_keys, p.max_seg_blocks, shape,
                            p.workspace_bytes if p.workspace_bytes else None, segs)
                free = route(amq, kind, p.n_segs, p.n_keys, p.max_seg_blocks, shape, UNLIMITED, segs)
                if segs is not None:
                    (got, gl), (free, fl) = got, free
                    assert list(gl) == list(fl), (kind, shape, p.segs["n_keys"], p.bits_per_key)
                    seen_leaf.update(int(x) for x in gl)
                    list_bytes = (64 * p.n_segs + 255) & ~255 if any(gl) else 0
                else:
                    list_bytes = 0
                a, b = [getattr(got, f) for f in fields], [getattr(free, f) for f in fields]
                assert a == b, (kind, shape, list(p.segs["n_keys"]), p.bits_per_key, a, b)
                assert got.ws_bytes + list_bytes <= p.workspace_bytes, (kind, shape, list(p.segs["n_keys"]))
                seen.add(got.route)
                seen_place.add(got.place)
    assert seen >= set(range(6)) | set(range(16, 22)), seen
    assert seen_place == {A.PLACE_NONE, A.PLACE_FUSED512, A.PLACE_FUSED256, A.PLACE_SCATTER}
    assert seen_leaf >= {A.LEAF_BATCH, A.LEAF_MULTI, A.LEAF_TILED_KEYS, A.LEAF_TILED_RECORDS,
                         A.LEAF_ATOMICS}, seen_leaf
