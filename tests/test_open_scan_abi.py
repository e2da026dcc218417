"""tkv_amq_open_filters / tkv_amq_scan_filters as far as they go without a device: the symbols
bind, the workspace size, every InvalidArgument case, the answer without a GPU -- and a numpy
restatement of the open validation and of the scan's block rules (include/tkv_amq.h), checked
here against oracle-built payloads.  tests/test_gpu_open_scan.py holds the device code to the
same restatement."""
import ctypes

import numpy as np
import pytest

from turtle_kv_amd import abi

BLOOM, VQF = 0, 1
BLOOM_MAGIC = 0xCA6F49A0F3F8A4B0
VQF_MAGIC = 0x16015305E0F43A7D
VQF_SEED = 0x9D0924DC03E79A75
LAYOUT_ID = {BLOOM: b"bloomflt", VQF: b"vqf_filt"}
U64 = (1 << 64) - 1

# (kind, bits/key, payload capacity): the settings of both test files
SETTINGS = [(BLOOM, 10, 0), (BLOOM, 12, 0), (BLOOM, 16, 0), (VQF, 12, 32704), (VQF, 22, 65472)]
LEAF_COUNTS = [16384, 8448, 0, 5, 1, 9000]
BLOOM_BIG = 110_000   # at 10 bits/key: 2,149 blocks, several scan chunks and a ragged tail
VQF_BIG = 40_000      # in 32,704 bytes: every block of the page, hash_val_shift 1


# ---------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------
def ref_open_payload(kind, buf, begin, bound):
    """include/tkv_amq.h, tkv_amq_open_filters, steps 1-5 for the payload at [begin, bound) of
    `buf`: (code, fields).  Reads nothing at or past `bound`."""
    if begin > bound:
        return abi.OPEN_OUT_OF_BOUNDS, None
    if begin % 16:
        return abi.OPEN_MISALIGNED, None
    room = bound - begin
    if room < (64 if kind == BLOOM else 80):
        return abi.OPEN_OUT_OF_BOUNDS, None
    q = np.frombuffer(bytes(buf[begin:begin + (64 if kind == BLOOM else 80)]), dtype="<u8")
    magic = int(q[0])
    if magic == (VQF_MAGIC if kind == BLOOM else BLOOM_MAGIC):
        return abi.OPEN_WRONG_KIND, None
    if magic != (BLOOM_MAGIC if kind == BLOOM else VQF_MAGIC):
        return abi.OPEN_BAD_MAGIC, None
    f = dict(out_offset=begin, hash_count=0, tag_bits=0, hash_val_shift=0, mod_magic=0)
    if kind == BLOOM:
        bit_count, src, word_count, item_count = int(q[1]), int(q[2]), int(q[4]), int(q[6])
        block_count = int(q[5]) & 0xFFFFFFFF
        hash_count = (int(q[5]) >> 32) & 0xFFFF
        layout = (int(q[5]) >> 48) & 0xFF
        if layout != 2 or not 1 <= hash_count <= 32 or block_count < 1:
            return abi.OPEN_BAD_GEOMETRY, None
        size = 64 + 64 * block_count
        if size > room or size > 0xFFFFFFFF:
            return abi.OPEN_OUT_OF_BOUNDS, None
        if bit_count != 512 * block_count or word_count != 8 * block_count:
            return abi.OPEN_BAD_GEOMETRY, None
        f.update(n_blocks=block_count, hash_count=hash_count, src_page_id=src,
                 n_keys=min(item_count, 0xFFFFFFFF), payload_bytes=size)
        return abi.OPEN_OK, f
    src, seed, mask = int(q[1]), int(q[2]), int(q[3])
    total_size, t, rng, nblocks, nelts, nslots = (int(x) for x in q[4:10])
    shifts = [sh for sh in range(64) if mask == (U64 << sh) & U64]
    if seed != VQF_SEED or not shifts or t not in (8, 16) or not 1 <= nblocks <= 1 << 24:
        return abi.OPEN_BAD_GEOMETRY, None
    size = 32 + 48 + 64 * nblocks
    if size > room or size > 0xFFFFFFFF:
        return abi.OPEN_OUT_OF_BOUNDS, None
    buckets, slots = (80, 48) if t == 8 else (36, 28)
    if total_size != 64 * nblocks or rng != (nblocks * buckets) << t or nslots != nblocks * slots \
            or nelts > nslots:
        return abi.OPEN_BAD_GEOMETRY, None
    f.update(n_blocks=nblocks, tag_bits=t, hash_val_shift=shifts[0], mod_magic=U64 // (nblocks * buckets),
             src_page_id=src, n_keys=min(nelts, 0xFFFFFFFF), payload_bytes=size)
    return abi.OPEN_OK, f


def ref_open(kind, buf, s, offsets=None, stride=0, page_size_log2=0):
    """Filter s of the buffer in one of the three location forms: (code, fields)."""
    total = len(buf)
    if page_size_log2:
        page, size = s << page_size_log2, 1 << page_size_log2
        begin, bound = page + 64, min(page + size, total)
    elif offsets is not None:
        begin, bound = int(offsets[s]), total
    else:
        begin, bound = s * stride, min((s + 1) * stride, total)
    code, f = ref_open_payload(kind, buf, begin, bound)
    if code == abi.OPEN_OK:
        f["page_flags"] = 0
        if page_size_log2:
            h = np.frombuffer(bytes(buf[page:page + 64]), dtype="<u4")
            if bytes(buf[page + 16:page + 24]) != LAYOUT_ID[kind] or int(h[7]) != 64 + f["payload_bytes"] \
                    or int(h[8]) != size or int(h[15]) != size:
                return abi.OPEN_BAD_PAGE, None
            f["page_flags"] = abi.PAGE_IMAGE | (page_size_log2 << 8)
    return code, f


def ref_scan_bloom(payload):
    """tkv_amq_filter_stats of one Bloom payload, with np.unpackbits per block."""
    q = np.frombuffer(bytes(payload[:64]), dtype="<u8")
    nb = int(q[5]) & 0xFFFFFFFF
    per = np.unpackbits(np.asarray(payload[64:64 + 64 * nb], dtype=np.uint8).reshape(nb, 64),
                        axis=1).sum(axis=1, dtype=np.int64)
    return dict(occupied=int(per.sum()), header_items=int(q[6]), full_blocks=int((per == 512).sum()),
                empty_blocks=int((per == 0).sum()), max_block=int(per.max()), bad_blocks=0)


def ref_vqf_blocks(payload):
    """Per block of one VQF payload: (occ, bad).  occ is -1 where the metadata gives none."""
    q = np.frombuffer(bytes(payload[:80]), dtype="<u8")
    t, nb = int(q[5]), int(q[7])
    W, B, S = (128, 80, 48) if t == 8 else (64, 36, 28)
    blocks = np.asarray(payload[80:80 + 64 * nb], dtype=np.uint8).reshape(nb, 64)
    md = np.unpackbits(blocks[:, :W // 8], axis=1, bitorder="little").astype(np.int64)
    pop = md.sum(axis=1)
    csum = np.cumsum(md, axis=1)
    sel = np.argmax(csum >= B, axis=1)                    # position of the B-th set bit
    occ = np.where(pop >= B, sel - (B - 1), -1)
    occ = np.where(occ > S, -1, occ)
    want = np.where(occ == 0, W - 1, W - occ)
    tags = blocks[:, 16:] if t == 8 else np.ascontiguousarray(blocks[:, 8:]).view("<u2")
    assert tags.shape == (nb, S)
    stray = ((tags != 0) & (np.arange(S)[None, :] >= occ[:, None])).any(axis=1)
    bad = (occ < 0) | (pop != want) | stray
    return occ, bad, S


def ref_scan_vqf(payload):
    q = np.frombuffer(bytes(payload[:80]), dtype="<u8")
    occ, bad, S = ref_vqf_blocks(payload)
    ok = occ[occ >= 0]
    return dict(occupied=int(ok.sum()), header_items=int(q[8]), full_blocks=int((ok == S).sum()),
                empty_blocks=int((ok == 0).sum()), max_block=int(ok.max()) if len(ok) else 0,
                bad_blocks=int(bad.sum()))


def ref_scan(kind, payload):
    return ref_scan_bloom(payload) if kind == BLOOM else ref_scan_vqf(payload)


def oracle_payload(O, kind, bpk, cap, keys, n, src_page_id=0):
    """One oracle-built payload (its used bytes) and, for VQF, the oracle's plan."""
    if kind == BLOOM:
        st, out = O.bloom_build(keys, n, bpk, src_page_id=src_page_id)
        assert st == 0
        return out, None
    st, out, pl = O.vqf_build(keys, n, bpk, cap, src_page_id=src_page_id)
    assert st == 0
    return out[:pl.payload_used], pl


# ---------------------------------------------------------------------------------------
# the ABI without a device
# ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    return abi.lib()


def test_symbols_exist_and_bind(L):
    for name in ("tkv_amq_open_filters", "tkv_amq_scan_filters_ws_bytes", "tkv_amq_scan_filters"):
        assert name in abi.EXPORTS
        assert hasattr(L, name)
    assert L.tkv_amq_open_filters.restype is ctypes.c_int and len(L.tkv_amq_open_filters.argtypes) == 11
    assert len(L.tkv_amq_scan_filters.argtypes) == 8
    assert abi.FILTER_STATS_DTYPE.itemsize == 32
    import turtle_kv_amd as amq
    for name in ("open_filters", "scan_filters", "filter_fill", "OpenedFilters"):
        assert hasattr(amq, name)
    assert hasattr(amq.FilterPage, "from_payload")


def test_scan_ws_bytes(L):
    f = L.tkv_amq_scan_filters_ws_bytes
    ns = (0, 1, 2, 255, 256, 6104, 6105, 1 << 20, 0xFFFFFFFF)
    v = [f(n) for n in ns]
    assert all(x >= 16 and x % 16 == 0 for x in v)
    assert v == sorted(v) and v[-1] > v[0]


# (a bad call is InvalidArgument with or without a device: the arguments are judged first)
def test_open_invalid_arguments(L):
    f = L.tkv_amq_open_filters
    buf = (ctypes.c_uint8 * 256)()
    p = ctypes.addressof(buf)
    p = p + (-p % 16)
    some = ctypes.c_void_p(p)
    # unknown kind
    assert f(2, some, 64, None, 64, 0, 0, None, None, None, None) == abi.INVALID_ARGUMENT
    assert f(-1, some, 64, None, 64, 0, 1, some, some, None, None) == abi.INVALID_ARGUMENT
    # contradictory location forms: two at once, all three, none with filters to open
    assert f(0, some, 64, some, 64, 0, 1, some, some, None, None) == abi.INVALID_ARGUMENT
    assert f(0, some, 64, some, 0, 12, 1, some, some, None, None) == abi.INVALID_ARGUMENT
    assert f(0, some, 64, None, 64, 12, 1, some, some, None, None) == abi.INVALID_ARGUMENT
    assert f(0, some, 64, some, 64, 12, 0, some, some, None, None) == abi.INVALID_ARGUMENT
    assert f(0, some, 64, None, 0, 0, 1, some, some, None, None) == abi.INVALID_ARGUMENT
    # a page size outside 7..31
    assert f(0, some, 64, None, 0, 6, 1, some, some, None, None) == abi.INVALID_ARGUMENT
    assert f(0, some, 64, None, 0, 32, 1, some, some, None, None) == abi.INVALID_ARGUMENT
    # null required buffers, a misaligned filter array
    assert f(0, some, 64, None, 64, 0, 1, None, some, None, None) == abi.INVALID_ARGUMENT
    assert f(0, some, 64, None, 64, 0, 1, some, None, None, None) == abi.INVALID_ARGUMENT
    assert f(0, None, 64, None, 64, 0, 1, some, some, None, None) == abi.INVALID_ARGUMENT
    assert f(0, ctypes.c_void_p(p + 8), 64, None, 64, 0, 1, some, some, None, None) == abi.INVALID_ARGUMENT


def test_scan_invalid_arguments(L):
    f = L.tkv_amq_scan_filters
    buf = (ctypes.c_uint8 * 256)()
    p = ctypes.addressof(buf)
    p = p + (-p % 16)
    some = ctypes.c_void_p(p)
    need = L.tkv_amq_scan_filters_ws_bytes(1)
    assert f(2, some, some, 0, some, some, need, None) == abi.INVALID_ARGUMENT
    assert f(0, None, some, 1, some, some, need, None) == abi.INVALID_ARGUMENT
    assert f(0, some, None, 1, some, some, need, None) == abi.INVALID_ARGUMENT
    assert f(1, some, some, 1, None, some, need, None) == abi.INVALID_ARGUMENT
    assert f(1, some, some, 1, some, None, need, None) == abi.INVALID_ARGUMENT
    assert f(0, some, some, 1, some, some, need - 1, None) == abi.INVALID_ARGUMENT      # short
    assert f(0, some, some, 1, some, ctypes.c_void_p(p + 8), need + 8, None) == abi.INVALID_ARGUMENT


def test_unavailable_without_a_device(L):
    if L.tkv_amq_device_count() != 0:
        # a device is visible: an empty batch is simply OK (tests/test_gpu_open_scan.py runs the rest)
        assert L.tkv_amq_open_filters(0, None, 0, None, 64, 0, 0, None, None, None, None) == abi.OK
        assert L.tkv_amq_scan_filters(0, None, None, 0, None, None, 0, None) == abi.OK
        return
    assert L.tkv_amq_open_filters(0, None, 0, None, 64, 0, 0, None, None, None, None) == abi.UNAVAILABLE
    assert L.tkv_amq_scan_filters(1, None, None, 0, None, None, 0, None) == abi.UNAVAILABLE
    import turtle_kv_amd as amq
    with pytest.raises(amq.TkvAmqError) as e:
        amq.scan_filters(amq.plan_filters(amq.BLOOM, [100], 10), None)
    assert e.value.status == abi.UNAVAILABLE


# ---------------------------------------------------------------------------------------
# the restatement against the oracle
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,bpk,cap", SETTINGS)
def test_restatement_agrees_with_oracle_payloads(oracle, kind, bpk, cap):
    import turtle_kv_amd as amq
    counts = LEAF_COUNTS + ([BLOOM_BIG] if (kind, bpk) == (BLOOM, 10) else []) + \
        ([VQF_BIG] if (kind, bpk) == (VQF, 12) else [])
    keys = oracle.gen_keys16(7, 0, sum(counts))
    plan = amq.plan_filters(kind, counts, bpk, payload_capacity=cap, src_page_ids=range(50, 50 + len(counts)))
    b = 0
    for s, n in enumerate(counts):
        payload, pl = oracle_payload(oracle, kind, bpk, cap, keys[b:b + n] if n else keys[:1], n, 50 + s)
        b += n
        seg = plan.segs[s]
        # the open restatement: exactly the plan's segment, from the bytes alone
        room = np.concatenate([np.zeros(32, np.uint8), payload, np.zeros(48, np.uint8)])
        code, f = ref_open_payload(kind, room, 32, 32 + len(payload))
        assert code == abi.OPEN_OK
        for name in ("n_blocks", "hash_count", "tag_bits", "hash_val_shift", "mod_magic",
                     "src_page_id", "payload_bytes"):
            assert f[name] == int(seg[name]), (name, s)
        assert ref_open_payload(kind, room, 32, 32 + len(payload) - 1)[0] == abi.OPEN_OUT_OF_BOUNDS
        assert ref_open_payload(kind, room, 24, len(room))[0] == abi.OPEN_MISALIGNED
        assert ref_open_payload(1 - kind, room, 32, len(room))[0] == abi.OPEN_WRONG_KIND
        # the scan restatement
        st = ref_scan(kind, payload)
        assert st["bad_blocks"] == 0
        if kind == BLOOM:
            assert st["header_items"] == n == f["n_keys"]
            k = int(seg["hash_count"])
            assert st["occupied"] <= n * k and (n == 0) == (st["occupied"] == 0)
            assert st["max_block"] <= 512
        else:
            occ, bad, S = ref_vqf_blocks(payload)
            assert st["occupied"] == st["header_items"] == f["n_keys"]       # sum(occ) == nelts
            assert (pl.hash_val_shift == 0) == (st["header_items"] == n) or n == 0
            assert pl.hash_val_shift == (1 if n == VQF_BIG else 0)
            assert pl.tag_bits == (16 if bpk == 22 else 8)
            assert int(occ.max()) <= S


def test_restatement_sees_a_broken_vqf_block(oracle):
    keys = oracle.gen_keys16(9, 0, 9000)
    payload, _ = oracle_payload(oracle, VQF, 12, 32704, keys, 9000)
    base = ref_scan_vqf(payload)
    occ, _, S = ref_vqf_blocks(payload)
    blk = int(np.argmax((occ > 0) & (occ < S)))
    p = payload.copy()
    # the top metadata bit: with 0 < occ < S it is a one above the B-th set bit, so clearing it
    # leaves occ alone and breaks popcount(md) == W - occ
    p[80 + 64 * blk + 15] ^= 0x80
    got = ref_scan_vqf(p)
    assert got["bad_blocks"] == 1 and got["occupied"] == base["occupied"]
    p = payload.copy()
    p[80 + 64 * blk + 16 + S - 1] = 0x5A            # a spare tag byte (the last slot is free)
    got = ref_scan_vqf(p)
    assert got["bad_blocks"] == 1 and got["occupied"] == base["occupied"]
