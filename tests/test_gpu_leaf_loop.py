"""The Bloom leaf loops for 16- and 24-byte keys (bloom_keys16_lds, bloom_keysL_lds) run their
full chunks of C = U * NT keys without guards and the rest, under C keys, guarded.  Every caller
of the loops is byte-compared with the CPU oracle, leaf by leaf, at leaf (or part) sizes round
the edges of a wave row and of a chunk: 0, 1, NT - 1, NT, NT + 1, C - 1, C, C + 1 and 2C + 3
keys, for the looped hash count (6 bits per key) and the unrolled k = 7 and k = 8 (10 and 12).

  caller                              NT    C (16-byte keys, U = 4)   C (24-byte keys, U = 2)
  bloom_build_lds, >= 2,048 leaves    256   1,024                     512
  bloom_build_lds, 256 leaves         1024  4,096                     2,048
  bloom_build_split, < 256 leaves     512   2,048                     1,024
  bloom_build_window, one window      1024  4,096                     2,048

The split build hands each workgroup a part [kb, ke) of a leaf of at least 2,048 keys, so there
the sizes are those of the parts (0 and 1 cannot be a part of such a leaf), and the leaf sizes C,
C + 1 and 2C + 3 are added where they reach 2,048 keys.  Every batch has leaves that start at odd key
indices (an odd-sized leaf comes early), and split parts start off the multiples of NT."""
import numpy as np
import pytest

from test_gpu_parity import assert_same, gpu_build, oracle_per_segment

pytestmark = pytest.mark.gpu

SHAPES = {"k16": (16, 4), "k24": (24, 2)}   # stride, U


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need a visible MI355X"
    return t


def edge_sizes(nt, c):
    return [0, 1, nt - 1, nt, nt + 1, c - 1, c, c + 1, 2 * c + 3]


def make_keys(oracle, shape, seed, n):
    stride = SHAPES[shape][0]
    if stride == 16:
        return oracle.gen_keys16(seed, 0, n), 16
    return np.random.default_rng(seed).integers(0, 256, (n, 24), dtype=np.uint8), 24


def build_and_compare(oracle, amq, torch, shape, counts, bpk, seed):
    """Builds the batch, compares every leaf with the oracle, returns the batch's route."""
    keys, stride = make_keys(oracle, shape, seed, sum(counts))
    plan, out = gpu_build(amq, torch, 0, torch.from_numpy(keys).cuda(), counts, bpk)
    r, _ = amq.filters.build_route(plan, stride, False)
    assert_same(plan, out, oracle_per_segment(oracle, 0, keys, counts, bpk, stride=stride))
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]])
    assert any(int(s) & 1 and c for s, c in zip(starts, counts)), "no leaf starts at an odd key index"
    return r


@pytest.mark.parametrize("bpk", [6, 10, 12])
@pytest.mark.parametrize("shape", ["k16", "k24"])
def test_lds_256_threads(oracle, amq, torch, shape, bpk):
    nt, c = 256, 256 * SHAPES[shape][1]
    rng = np.random.default_rng(bpk)
    counts = edge_sizes(nt, c) + [int(x) for x in rng.integers(0, 40, 2048 - 9)]
    r = build_and_compare(oracle, amq, torch, shape, counts, bpk, 71)
    assert r.route == amq.abi.ROUTE_LDS and r.threads == 256


@pytest.mark.parametrize("bpk", [6, 10, 12])
@pytest.mark.parametrize("shape", ["k16", "k24"])
def test_lds_1024_threads(oracle, amq, torch, shape, bpk):
    nt, c = 1024, 1024 * SHAPES[shape][1]
    rng = np.random.default_rng(bpk)
    counts = edge_sizes(nt, c) + [int(x) for x in rng.integers(0, 40, 256 - 9)]
    r = build_and_compare(oracle, amq, torch, shape, counts, bpk, 72)
    assert r.route == amq.abi.ROUTE_LDS and r.threads == 1024


def split_part_sizes(n, parts):
    """bloom_build_split's key ranges of a leaf of n keys"""
    chunk = -(-n // parts)
    kb = [min(n, p * chunk) for p in range(parts)]
    return kb, [min(n, b + chunk) - b for b in kb]


@pytest.mark.parametrize("bpk", [6, 10, 12])
@pytest.mark.parametrize("shape", ["k16", "k24"])
def test_split_parts(oracle, amq, torch, shape, bpk):
    """Four parts per leaf (the batch averages 4,096 to 5,119 keys a leaf).  A leaf of n keys is
    cut into parts of ceil(n / 4) keys and a shorter last one: 2,048 -> 4 x 512, 2,050 -> 3 x 513
    and 511, 4C - 1 -> 3 x C and C - 1, 4C + 4 -> 4 x (C + 1), 8C + 12 -> 4 x (2C + 3)."""
    nt, c = 512, 512 * SHAPES[shape][1]
    counts = [2049, 2048, 2050, 2052, 4 * c - 1, 4 * c, 4 * c + 4, 8 * c + 12]
    counts += [x for x in (c, c + 1, 2 * c + 3) if x >= 2048 and x not in counts]
    # fill with leaves of 2,051 and 6,001 keys up to an average of four parts' worth
    while not 4096 <= (sum(counts) + 2051) // (len(counts) + 1) < 5120:
        counts.append(6001 if sum(counts) // len(counts) < 4608 else 2051)
    counts.append(2051)
    seen, off_row = set(), False
    for n in counts:
        kb, sizes = split_part_sizes(n, 4)
        seen.update(sizes)
        off_row |= any(b % nt for b in kb)
    assert set(edge_sizes(nt, c)[2:]) <= seen and off_row
    r = build_and_compare(oracle, amq, torch, shape, counts, bpk, 73)
    assert r.route == amq.abi.ROUTE_SPLIT and r.parts == 4 and r.threads == 512


@pytest.mark.parametrize("bpk", [6, 10, 12])
@pytest.mark.parametrize("shape", ["k16", "k24"])
def test_window_single_window_leaves(oracle, amq, torch, shape, bpk):
    """One leaf of two windows makes the batch take the window route; the leaves beside it fit
    one window each and run the leaf loop (1,024 threads).  Enough tiny leaves bring the average
    under 4,096 keys a leaf, so every leaf is one part and the loop sees whole leaves."""
    nt, c = 1024, 1024 * SHAPES[shape][1]
    big = 1_400_000 // bpk   # 2,735 blocks: two windows of 1,368
    rng = np.random.default_rng(bpk)
    counts = [3, 1] + edge_sizes(nt, c) + [big] + [int(x) for x in rng.integers(0, 40, 80)]
    assert sum(counts) // len(counts) < 4096
    r = build_and_compare(oracle, amq, torch, shape, counts, bpk, 74)
    assert r.route == amq.abi.ROUTE_WINDOW and r.windows == 2 and r.parts == 1
