"""The Bloom leaf, split and window builds keep their LDS image strided (word w of local block b at
byte (b >> 3) * 512 + w * 32 + (b & 7) * 4: turtle_kv_amd/csrc/tkv_amq_lds_stride.h) and write it
out in canonical order.  Every leaf of every batch here is byte-compared with the CPU oracle, and
every batch asserts its route.

Leaves sit round the edges of the layout's 8-block regions: 1, 7, 8, 9, 15, 16, 17 and 41 blocks
(a last region that is full, one block short, one block long), a leaf of no keys, and leaves under
one chunk of the loops beside leaves of several, at 6 bits per key (the looped hash count), 10
(k = 7) and 12 (k = 8).  Key shapes: 16-byte and 24-byte keys (the unguarded loops), a 20-byte
stride (the generic loop) and variable-length keys of 8..31 bytes (the length-sorted build, whose
image lies behind the sort's scratch in LDS).

  route                                   batch
  bloom_build_lds, 256 threads            2,048 leaves
  bloom_build_lds, 1,024 threads          256 leaves
  bloom_build_split + bloom_split_merge   8 leaves of 2,048+ keys, block counts off the multiples of 8
  bloom_build_window, two windows         one leaf of 2,561 blocks (a block past 160 KB: windows
                                          of 1,281 blocks, so the second starts at block 1,281,
                                          off a region's edge) among small ones; one part a leaf
                                          (straight into the filters) and several (merged)
  page images                             a 2,048-leaf batch planned as whole filter pages"""
import numpy as np
import pytest

from test_gpu_parity import assert_same, gpu_build, oracle_per_segment

pytestmark = pytest.mark.gpu

EDGE_BLOCKS = [1, 7, 8, 9, 15, 16, 17, 41]
SHAPES = ["k16", "k24", "k20", "var"]


@pytest.fixture(scope="module")
def torch():
    import torch as t
    assert t.cuda.is_available(), "GPU tests need a visible MI355X"
    return t


def keys_for(blocks, bpk):
    """the most keys whose filter has `blocks` blocks: ceil(n * bpk / 512) == blocks"""
    return blocks * 512 // bpk


def make_keys(oracle, shape, seed, n):
    """(key bytes, stride, offsets or None) of n keys"""
    rng = np.random.default_rng(seed)
    if shape == "k16":
        return oracle.gen_keys16(seed, 0, n), 16, None
    if shape in ("k24", "k20"):
        stride = int(shape[1:])
        return rng.integers(0, 256, (n, stride), dtype=np.uint8), stride, None
    lens = rng.integers(8, 32, n)
    offs = np.zeros(n + 1, np.int64)
    offs[1:] = np.cumsum(lens)
    return rng.integers(0, 256, max(int(lens.sum()), 1), dtype=np.uint8), 0, offs


def build_and_compare(oracle, amq, torch, shape, counts, bpk, seed, want_blocks=()):
    """Builds the batch, compares every leaf with the oracle, returns (route, plan)."""
    keys, stride, offs = make_keys(oracle, shape, seed, sum(counts))
    plan, out = gpu_build(amq, torch, 0, torch.from_numpy(keys).cuda(), counts, bpk,
                          offsets_t=None if offs is None else torch.from_numpy(offs).cuda())
    have = {int(b) for b in plan.segs["n_blocks"]}
    assert set(want_blocks) <= have, (sorted(set(want_blocks) - have), bpk)
    r, _ = amq.filters.build_route(plan, stride, offs is not None)
    ref = oracle_per_segment(oracle, 0, keys, counts, bpk, stride=stride,
                             offsets=None if offs is None else offs.astype(np.uint64))
    assert_same(plan, out, ref)
    return r, plan


def edge_counts(bpk):
    """a leaf of no keys, the region-edge leaves (the larger ones span chunks of the loops, the
    smaller ones are all tail), and the same one key short (odd key indices behind them)"""
    counts = [0] + [keys_for(b, bpk) for b in EDGE_BLOCKS]
    return counts + [keys_for(b, bpk) - 1 for b in (8, 9, 16)] + [1, 3]


@pytest.mark.parametrize("bpk", [6, 10, 12])
@pytest.mark.parametrize("shape", SHAPES)
def test_lds_256_threads(oracle, amq, torch, shape, bpk):
    rng = np.random.default_rng(bpk)
    counts = edge_counts(bpk)
    counts += [int(x) for x in rng.integers(0, 40, 2048 - len(counts))]
    r, _ = build_and_compare(oracle, amq, torch, shape, counts, bpk, 81, EDGE_BLOCKS)
    assert r.route == amq.abi.ROUTE_LDS and r.threads == 256


@pytest.mark.parametrize("bpk", [6, 10, 12])
@pytest.mark.parametrize("shape", SHAPES)
def test_lds_1024_threads(oracle, amq, torch, shape, bpk):
    rng = np.random.default_rng(bpk)
    counts = edge_counts(bpk)
    counts += [int(x) for x in rng.integers(0, 40, 256 - len(counts))]
    r, _ = build_and_compare(oracle, amq, torch, shape, counts, bpk, 82, EDGE_BLOCKS)
    assert r.route == amq.abi.ROUTE_LDS and r.threads == 1024


SPLIT_BLOCKS = [49, 55, 56, 57, 63, 64, 65, 97]   # 2,048+ keys each at 12 bits per key and under


@pytest.mark.parametrize("bpk", [6, 10, 12])
@pytest.mark.parametrize("shape", SHAPES)
def test_split_and_merge(oracle, amq, torch, shape, bpk):
    counts = [keys_for(b, bpk) for b in SPLIT_BLOCKS]
    assert min(counts) >= 2048
    r, plan = build_and_compare(oracle, amq, torch, shape, counts, bpk, 83, SPLIT_BLOCKS)
    assert r.route == amq.abi.ROUTE_SPLIT and r.parts >= 2 and r.threads == 512
    assert int(plan.max_seg_blocks) % 8 != 0


BIG_BLOCKS = 2561   # one block past 160 KB of image


@pytest.mark.parametrize("bpk", [6, 10, 12])
@pytest.mark.parametrize("shape", SHAPES)
def test_two_windows_one_part(oracle, amq, torch, shape, bpk):
    """Enough small leaves beside the big one keep the batch at one part a leaf: each window is
    written straight into its filter, the small leaves are one window each (the leaf loops)."""
    rng = np.random.default_rng(bpk)
    counts = edge_counts(bpk) + [keys_for(BIG_BLOCKS, bpk)] + [int(x) for x in rng.integers(0, 40, 80)]
    assert sum(counts) // len(counts) < 4096
    r, plan = build_and_compare(oracle, amq, torch, shape, counts, bpk, 84, EDGE_BLOCKS + [BIG_BLOCKS])
    assert r.route == amq.abi.ROUTE_WINDOW and r.windows == 2 and r.parts == 1
    assert -(-BIG_BLOCKS // r.windows) % 8 != 0   # the second window starts inside a region


@pytest.mark.parametrize("shape", ["k16", "k24"])
def test_two_windows_merged_parts(oracle, amq, torch, shape):
    """Few leaves: several parts a leaf, each writing its windows into a partial image in the
    workspace (canonical, like the filters), ORed by bloom_split_merge."""
    counts = [keys_for(BIG_BLOCKS, 10), keys_for(41, 10), keys_for(1281, 10)]
    r, _ = build_and_compare(oracle, amq, torch, shape, counts, 10, 85, [BIG_BLOCKS, 41, 1281])
    assert r.route == amq.abi.ROUTE_WINDOW and r.windows == 2 and r.parts > 1


def test_page_images(oracle, amq, torch):
    """Whole filter pages: the page header's pieces are written by the lanes beside the ones that
    start the un-permuted payload."""
    bpk, log2 = 10, 12   # 4 KiB pages: 64 + 64 + 41 * 64 bytes fit
    rng = np.random.default_rng(5)
    counts = edge_counts(bpk)
    counts += [int(x) for x in rng.integers(0, 40, 2048 - len(counts))]
    keys = oracle.gen_keys16(86, 0, sum(counts))
    plan = amq.plan_filter_pages(0, counts, bpk, log2)
    assert (plan.segs["page_flags"] & amq.abi.PAGE_IMAGE).all()
    assert set(EDGE_BLOCKS) <= {int(b) for b in plan.segs["n_blocks"]}
    r, _ = amq.filters.build_route(plan, 16, False)
    assert r.route == amq.abi.ROUTE_LDS and r.threads == 256
    out = amq.build_all_filters(plan, amq.KeyBatch.fixed(torch.from_numpy(keys).cuda()))
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    assert_same(plan, o, oracle_per_segment(oracle, 0, keys, counts, bpk))
    for s in range(len(counts)):
        page = o[s << log2:(s << log2) + 64]
        assert bytes(page[16:24]) == b"bloomflt", s
        assert int(page[28:32].view(np.uint32)[0]) == 64 + int(plan.segs[s]["payload_bytes"]), s
        assert int(page[32:36].view(np.uint32)[0]) == 1 << log2, s
        assert int(page[60:64].view(np.uint32)[0]) == 1 << log2, s
        assert not page[:16].any() and not page[24:28].any() and not page[36:60].any(), s
