"""Host-side mirror of TurtleKV's filter build/probe API over libtkv_amq (HIP, gfx950).

Reference interface (mathworks/turtle_kv, src/turtle_kv/...) and the function here that
replaces it:

  TreeOptions::filter_bits_per_key        tree/tree_options.hpp:155-164  -> filter_bits_per_key
  TreeOptions filter page sizing          tree/tree_options.hpp:166-258  -> TreeOptions
  vqf_hash_val                            vqf_filter_page_view.hpp:32-35 -> vqf_hash_val
  vqf_filter_load_factor<T>               vqf_filter_page_view.hpp:39-59 -> vqf_filter_load_factor
  build_bloom_filter_for_leaf             tree/filter_builder.hpp:109-152 -> build_bloom_filter_for_leaf
  build_quotient_filter_for_leaf          tree/filter_builder.hpp:221-301 -> build_quotient_filter_for_leaf
  build_filter_for_leaf_in_job            tree/filter_builder.hpp:307-331 -> build_filter_for_leaf_in_job
  TreeSerializeContext::build_all_pages   tree/tree_serialize_context.cpp:62-115 (the filter
                                          half of it)                     -> build_all_filters
  PackedVqfFilter::is_present             vqf_filter_page_view.hpp:113-125 -> PackedVqfFilter.is_present
  KeyQuery::reject_page                   tree/key_query.hpp:149-247      -> KeyQuery.reject_page
  KeyQuery::Metrics                       tree/key_query.hpp:36-60        -> KeyQueryMetrics
  FilterPageAlloc page + header fields    tree/filter_builder.hpp:58-105,231-237,293-296
                                                                          -> plan_filter_pages
  reject_page's read of a loaded page     tree/key_query.hpp:149-247, vqf_filter_page_view.hpp:96-100
                                                                          -> open_filters,
                                                                             FilterPage.from_payload

Device memory, streams and multi-GPU plumbing come from PyTorch-ROCm; every filter
computation runs in the HIP kernels of libtkv_amq.so.  There is no CPU fallback: with no
GPU visible the device entry points raise TkvAmqError(Unavailable).
"""
from __future__ import annotations

import ctypes
import enum
import logging
import threading
import time
from dataclasses import dataclass, field

import numpy as np

from . import abi
from .abi import BLOOM, VQF, TkvAmqError

log = logging.getLogger("turtle_kv_amd")

# config.hpp:20-24 -- the reference compiles VQF in by default
TURTLE_KV_USE_BLOOM_FILTER = 0
TURTLE_KV_USE_QUOTIENT_FILTER = 1
DEFAULT_FILTER_KIND = VQF if TURTLE_KV_USE_QUOTIENT_FILTER else BLOOM

K_VQF_HASH_SEED = 0x9D0924DC03E79A75          # vqf_filter_page_view.hpp:26
K_MIN_QUOTIENT_FILTER_BITS_PER_KEY = 12       # vqf_filter_page_view.hpp:27
K_MAX_QUOTIENT_FILTER_LOAD_FACTOR = 0.85      # vqf_filter_page_view.hpp:28
K_DEFAULT_FILTER_BITS_PER_KEY = 12            # tree/tree_options.hpp:57
PACKED_PAGE_HEADER_BYTES = 64                 # llfs::PackedPageHeader (page payload offset)
VQF_MAGIC = 0x16015305E0F43A7D
BLOOM_MAGIC = 0xCA6F49A0F3F8A4B0


class BoolStatus(enum.Enum):
    """turtle_kv/import/bool_status.hpp: reject_page's tri-state result."""
    kFalse = 0
    kTrue = 1
    kUnknown = 2


def _torch():
    import torch
    return torch


def _stream_handle(stream=None):
    torch = _torch()
    s = stream if stream is not None else torch.cuda.current_stream()
    return ctypes.c_void_p(s.cuda_stream)


def _hold(stream, *tensors):
    """Temporaries handed to a kernel launched on `stream` (a torch.cuda.Stream other than the
    current one): record that stream on them, so the caching allocator does not give their
    memory to other work before the kernel has read it."""
    torch = _torch()
    if stream is None or stream == torch.cuda.current_stream():
        return
    for t in tensors:
        if t is not None and getattr(t, "is_cuda", False):
            t.record_stream(stream)


def _ptr(t) -> ctypes.c_void_p | None:
    if t is None:
        return None
    if isinstance(t, np.ndarray):
        return ctypes.c_void_p(t.ctypes.data)
    return ctypes.c_void_p(t.data_ptr())


def _require_device():
    if abi.lib().tkv_amq_device_count() == 0:
        raise TkvAmqError(abi.UNAVAILABLE, "no HIP device visible")


# ---------------------------------------------------------------------------------------
# sizing
# ---------------------------------------------------------------------------------------
def filter_bits_per_key(requested: int | None, kind: int = DEFAULT_FILTER_KIND) -> int:
    """TreeOptions::filter_bits_per_key(): default 12; VQF clamps nonzero values to >= 12."""
    bpk = K_DEFAULT_FILTER_BITS_PER_KEY if requested is None else int(requested)
    return int(abi.lib().tkv_amq_filter_bits_per_key(kind, bpk))


def vqf_filter_load_factor(tag_bits: int, bits_per_key: int) -> float:
    if bits_per_key != 0 and bits_per_key < K_MIN_QUOTIENT_FILTER_BITS_PER_KEY:
        raise TkvAmqError(abi.INVALID_ARGUMENT, "vqf_filter_load_factor: bits_per_key < 12")
    if tag_bits not in (8, 16):
        raise TkvAmqError(abi.INVALID_ARGUMENT, "TAG_BITS must be 8 or 16")
    return float(abi.lib().tkv_amq_vqf_load_factor(tag_bits, bits_per_key))


def _log2_ceil(x: int) -> int:
    return max(0, (int(x) - 1).bit_length())


class TreeOptions:
    """The filter part of TreeOptions (tree/tree_options.hpp:43-395, tree_options.cpp:17-60):
    bits per key with the VQF clamp, and the filter page size derived from the leaf size and
    the key/value size hints.  `kind` stands for the compile-time filter switch (config.hpp:20-24)."""

    kDefaultFilterBitsPerKey = 12   # :57
    kDefaultKeySizeHint = 24        # :58
    kDefaultValueSizeHint = 100     # :59

    def __init__(self, kind: int = DEFAULT_FILTER_KIND):
        self.kind = kind
        self.leaf_size_log2_ = 21                  # 2 MiB (:384, with_default_values)
        self.filter_bits_per_key_ = None
        self.filter_page_size_log2_ = None
        self.key_size_hint_ = self.kDefaultKeySizeHint
        self.value_size_hint_ = self.kDefaultValueSizeHint

    @classmethod
    def with_default_values(cls, kind: int = DEFAULT_FILTER_KIND) -> "TreeOptions":
        return cls(kind)

    # leaf size
    def leaf_size(self) -> int:
        return 1 << self.leaf_size_log2_

    def set_leaf_size(self, size: int) -> "TreeOptions":
        self.leaf_size_log2_ = _log2_ceil(size)
        if self.leaf_size() != size:
            raise TkvAmqError(abi.INVALID_ARGUMENT, "leaf_size must be a power of 2")  # :106
        return self

    def set_leaf_size_log2(self, size_log2: int) -> "TreeOptions":
        self.leaf_size_log2_ = int(size_log2)
        return self

    def leaf_data_size(self) -> int:
        """leaf_max_space_from_size (tree/packed_leaf_page.hpp:307-311)."""
        return int(abi.lib().tkv_amq_leaf_data_size(self.leaf_size()))

    # bits per key
    def set_filter_bits_per_key(self, bits_per_key: int | None) -> "TreeOptions":
        self.filter_bits_per_key_ = bits_per_key
        return self

    def filter_bits_per_key(self) -> int:
        return filter_bits_per_key(self.filter_bits_per_key_, self.kind)

    # item size hints
    def key_size_hint(self) -> int:
        return self.key_size_hint_

    def set_key_size_hint(self, n_bytes: int) -> "TreeOptions":
        self.key_size_hint_ = int(n_bytes)
        return self

    def value_size_hint(self) -> int:
        return self.value_size_hint_

    def set_value_size_hint(self, n_bytes: int) -> "TreeOptions":
        self.value_size_hint_ = int(n_bytes)
        return self

    def expected_item_size(self) -> int:
        """PackedSizeOfEdit (core/packed_sizeof_edit.hpp:13-15) of a hint-sized edit."""
        return 4 + self.key_size_hint_ + 4 + 1 + self.value_size_hint_

    def expected_items_per_leaf(self) -> int:
        return int(abi.lib().tkv_amq_expected_items_per_leaf(self.leaf_size(), self.key_size_hint_,
                                                             self.value_size_hint_))

    # filter page size
    def set_filter_page_size_log2(self, size_log2: int) -> "TreeOptions":
        self.filter_page_size_log2_ = int(size_log2)
        return self

    def set_filter_page_size(self, size: int) -> "TreeOptions":
        return self.set_filter_page_size_log2(_log2_ceil(size))

    def filter_page_size_log2(self) -> int:
        if self.filter_page_size_log2_ is not None:
            return self.filter_page_size_log2_
        return int(abi.lib().tkv_amq_filter_page_size_log2(
            self.kind, self.leaf_size(), self.key_size_hint_, self.value_size_hint_,
            K_DEFAULT_FILTER_BITS_PER_KEY if self.filter_bits_per_key_ is None
            else int(self.filter_bits_per_key_)))

    def filter_page_size(self) -> int:
        return 1 << self.filter_page_size_log2()

    def filter_page_payload_size(self) -> int:
        """The payload buffer the filter builders size against: page size minus the llfs
        PackedPageHeader (filter_builder.hpp:231-244)."""
        return self.filter_page_size() - PACKED_PAGE_HEADER_BYTES


def vqf_required_size(tag_bits: int, nslots: int) -> int:
    return int(abi.lib().tkv_amq_vqf_required_size(tag_bits, nslots))


def vqf_nslots_for_size(tag_bits: int, nbytes: int) -> int:
    return int(abi.lib().tkv_amq_vqf_nslots_for_size(tag_bits, nbytes))


@dataclass
class FilterPlan:
    """Host plan of one batch of leaf filters (one build_all_pages queue)."""
    kind: int
    bits_per_key: int
    segs: np.ndarray                     # SEGMENT_DTYPE[n_segs]
    total_out_bytes: int
    workspace_bytes: int
    max_seg_blocks: int
    n_keys: int
    _device: dict = field(default_factory=dict, repr=False)
    _stats: dict | None = field(default=None, repr=False)

    @property
    def n_segs(self) -> int:
        return len(self.segs)

    def device_segs(self, device=None):
        """The plan uploaded to the device (cached per device)."""
        torch = _torch()
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        key = str(dev)
        if key not in self._device:
            host = torch.from_numpy(self.segs.view(np.uint8).reshape(-1).copy())
            self._device[key] = host.to(dev, non_blocking=False)
        return self._device[key]


def plan_filters(kind: int, seg_key_counts, bits_per_key: int, payload_capacity: int = 0,
                 out_stride: int = 0, src_page_ids=None) -> FilterPlan:
    """Restated build_{bloom,quotient}_filter_for_leaf sizing for every leaf of a batch."""
    counts = np.ascontiguousarray(np.asarray(seg_key_counts, dtype=np.uint64))
    n = len(counts)
    segs = np.zeros(n, dtype=abi.SEGMENT_DTYPE)
    src = None if src_page_ids is None else np.ascontiguousarray(np.asarray(src_page_ids, dtype=np.uint64))
    tot, ws, mb = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint32(0)
    st = abi.lib().tkv_amq_plan(kind, _ptr(counts), _ptr(src), n, int(bits_per_key),
                                int(payload_capacity), int(out_stride), _ptr(segs),
                                ctypes.byref(tot), ctypes.byref(ws), ctypes.byref(mb))
    abi.check(st, "tkv_amq_plan")
    return FilterPlan(kind, int(bits_per_key), segs, int(tot.value), int(ws.value), int(mb.value),
                      int(counts.sum()) if n else 0)


def plan_filter_pages(kind: int, seg_key_counts, bits_per_key: int, page_size_log2: int,
                      src_page_ids=None) -> FilterPlan:
    """One whole filter page per leaf (tkv_amq_plan_pages): leaf s's page is bytes
    [s << log2, (s+1) << log2) of the output, a 64-byte page header then the payload, the
    buffer FilterPageAlloc hands the builder (filter_builder.hpp:70-88).  The build writes the
    header fields the builders set (layout_id, unused_begin, unused_end) and the page size."""
    counts = np.ascontiguousarray(np.asarray(seg_key_counts, dtype=np.uint64))
    n = len(counts)
    segs = np.zeros(n, dtype=abi.SEGMENT_DTYPE)
    src = None if src_page_ids is None else np.ascontiguousarray(np.asarray(src_page_ids, dtype=np.uint64))
    tot, ws, mb = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint32(0)
    st = abi.lib().tkv_amq_plan_pages(kind, _ptr(counts), _ptr(src), n, int(bits_per_key),
                                      int(page_size_log2), _ptr(segs), ctypes.byref(tot),
                                      ctypes.byref(ws), ctypes.byref(mb))
    abi.check(st, "tkv_amq_plan_pages")
    return FilterPlan(kind, int(bits_per_key), segs, int(tot.value), int(ws.value), int(mb.value),
                      int(counts.sum()) if n else 0)


def page_header_fields(page: np.ndarray) -> dict:
    """The PackedPageHeader fields of one filter page image (offsets as in tkv_amq_plan_pages,
    llfs 0.42's layout: UNPINNED)."""
    b = np.asarray(page, dtype=np.uint8)
    u32 = b[:64].view("<u4")
    return {"layout_id": bytes(b[16:24]).rstrip(b"\0").decode("ascii", "replace"),
            "unused_begin": int(u32[7]), "unused_end": int(u32[8]), "size": int(u32[15])}


# ---------------------------------------------------------------------------------------
# keys
# ---------------------------------------------------------------------------------------
@dataclass
class KeyBatch:
    """Device-resident keys: fixed-length rows (`data` [n, L]) or variable-length bytes
    (`data` [total] + `offsets` int64 [n+1]), the flattened EditView key range the reference
    passes as `items` (core/merge_compactor.hpp:108-139)."""
    data: object
    n: int
    stride: int = 16
    offsets: object = None

    @staticmethod
    def fixed(t) -> "KeyBatch":
        assert t.dim() == 2 and t.dtype == _torch().uint8 and t.is_cuda and t.is_contiguous()
        return KeyBatch(t, t.shape[0], t.shape[1], None)

    @staticmethod
    def variable(data, offsets) -> "KeyBatch":
        torch = _torch()
        assert data.dtype == torch.uint8 and offsets.dtype == torch.int64
        return KeyBatch(data, offsets.numel() - 1, 0, offsets)

    @staticmethod
    def from_host(keys, device=None) -> "KeyBatch":
        """bytes-like list or [n, L] uint8 array -> device KeyBatch (H2D copy)."""
        torch = _torch()
        dev = device or "cuda"
        if isinstance(keys, np.ndarray) and keys.ndim == 2:
            return KeyBatch.fixed(torch.from_numpy(np.ascontiguousarray(keys)).to(dev))
        ks = [bytes(k) for k in keys]
        lens = {len(k) for k in ks}
        if len(lens) == 1 and ks:
            arr = np.frombuffer(b"".join(ks), dtype=np.uint8).reshape(len(ks), -1)
            return KeyBatch.fixed(torch.from_numpy(arr.copy()).to(dev))
        offs = np.zeros(len(ks) + 1, dtype=np.int64)
        np.cumsum([len(k) for k in ks], out=offs[1:])
        blob = np.frombuffer(b"".join(ks), dtype=np.uint8) if ks else np.zeros(0, np.uint8)
        data = torch.from_numpy(blob.copy() if len(blob) else np.zeros(1, np.uint8)).to(dev)
        return KeyBatch.variable(data, torch.from_numpy(offs).to(dev))


def key_views(buf: np.ndarray, offsets, lengths) -> np.ndarray:
    """tkv_amq_key_view records (KeyView = std::string_view {size, data}) for keys stored at
    byte `offsets[i]` (length `lengths[i]`) of host buffer `buf` -- the shape of the EditView
    key range the reference iterates (core/merge_compactor.hpp:107-139)."""
    offsets = np.asarray(offsets, dtype=np.uint64)
    v = np.empty(len(offsets), dtype=abi.KEY_VIEW_DTYPE)
    v["size"] = np.broadcast_to(np.asarray(lengths, dtype=np.uint64), offsets.shape)
    v["data"] = np.uint64(buf.ctypes.data) + offsets
    return v


def stage_keys(views, n: int | None = None, fixed_len: int = 16, out=None, view_stride: int = 16,
               n_threads: int = 0):
    """Gather viewed keys into one contiguous host buffer (tkv_amq_stage_keys, host threads).
    `views`: KEY_VIEW_DTYPE array or the address of the first view (then `n` and
    `view_stride` say how many and how far apart).  fixed_len > 0: returns `out` ([n,
    fixed_len] uint8, numpy or pinned torch); fixed_len == 0: returns (bytes, offsets[n+1])."""
    if isinstance(views, np.ndarray):
        assert views.dtype == abi.KEY_VIEW_DTYPE and views.flags.c_contiguous
        addr, n, view_stride = views.ctypes.data, len(views), abi.KEY_VIEW_DTYPE.itemsize
    else:
        addr = int(views)
    if fixed_len:
        if out is None:
            out = np.empty((n, fixed_len), dtype=np.uint8)
        cap = out.nbytes if isinstance(out, np.ndarray) else out.numel()
        st = abi.lib().tkv_amq_stage_keys(ctypes.c_void_p(addr), view_stride, n, fixed_len,
                                          _ptr(out), cap, None, n_threads)
        abi.check(st, "tkv_amq_stage_keys")
        return out
    sizes = np.ctypeslib.as_array((ctypes.c_uint64 * (2 * n)).from_address(addr)) if n and \
        view_stride == 16 else None
    total = int(sizes[0::2].sum()) if sizes is not None else (0 if n == 0 else None)
    if out is None:
        if total is None:
            raise TkvAmqError(abi.INVALID_ARGUMENT, "pass `out` for strided variable-length views")
        out = np.empty(max(total, 1), dtype=np.uint8)
    offs = np.empty(n + 1, dtype=np.uint64)
    cap = out.nbytes if isinstance(out, np.ndarray) else out.numel()
    st = abi.lib().tkv_amq_stage_keys(ctypes.c_void_p(addr), view_stride, n, 0, _ptr(out), cap,
                                      _ptr(offs), n_threads)
    abi.check(st, "tkv_amq_stage_keys")
    return out, offs


def gen_keys16(seed: int, first: int, n: int, device=None, stream=None):
    """Synthetic bench keys on the device (splitmix64 stream)."""
    torch = _torch()
    _require_device()
    out = torch.empty((n, 16), dtype=torch.uint8, device=device or "cuda")
    abi.check(abi.lib().tkv_amq_gen_keys16(seed, first, n, _ptr(out), _stream_handle(stream)),
              "tkv_amq_gen_keys16")
    return out


# ---------------------------------------------------------------------------------------
# build
# ---------------------------------------------------------------------------------------
# ---------------------------------------------------------------------------------------
# build metrics (BloomFilterMetrics, tree/filter_builder.hpp:39-56,136-147;
# QuotientFilterMetrics, :156-172,198-202)
# ---------------------------------------------------------------------------------------
class StatsMetric:
    """batt StatsMetric<u64>: count, total, min, max of the values it was updated with."""

    def __init__(self):
        self._lock = threading.Lock()
        self.count, self.total, self.min, self.max = 0, 0, None, None

    def merge(self, count: int, total: int, lo: int, hi: int) -> None:
        if count == 0:
            return
        with self._lock:
            self.count += count
            self.total += total
            self.min = lo if self.min is None else min(self.min, lo)
            self.max = hi if self.max is None else max(self.max, hi)

    def update(self, v: int) -> None:
        self.merge(1, int(v), int(v), int(v))

    @property
    def mean(self) -> float:
        return self.total / self.count if self.count else 0.0

    def __repr__(self):
        return f"StatsMetric(count={self.count}, total={self.total}, min={self.min}, max={self.max})"


class LatencyMetric:
    """LatencyMetric: count and total microseconds (per leaf filter, amortised over a batch)."""

    def __init__(self):
        self._lock = threading.Lock()
        self.count, self.total_usec = 0, 0

    def add(self, count: int, usec: float) -> None:
        with self._lock:
            self.count += count
            self.total_usec += int(usec)


class BloomFilterMetrics:
    """tree/filter_builder.hpp:39-56 (one process-wide instance, like Self::instance())."""
    _inst = None

    def __init__(self):
        self.word_count_stats = StatsMetric()
        self.byte_size_stats = StatsMetric()
        self.bit_size_stats = StatsMetric()
        self.bit_count_stats = StatsMetric()
        self.item_count_stats = StatsMetric()
        self.build_page_latency = LatencyMetric()

    @classmethod
    def instance(cls) -> "BloomFilterMetrics":
        if cls._inst is None:
            cls._inst = cls()
        return cls._inst


class QuotientFilterMetrics:
    """tree/filter_builder.hpp:156-172."""
    _inst = None

    def __init__(self):
        self.byte_size_stats = StatsMetric()
        self.bit_size_stats = StatsMetric()
        self.item_count_stats = StatsMetric()
        self.bits_per_key_stats = StatsMetric()
        self.build_page_latency = LatencyMetric()

    @classmethod
    def instance(cls) -> "QuotientFilterMetrics":
        if cls._inst is None:
            cls._inst = cls()
        return cls._inst


def _agg(v: np.ndarray):
    return (len(v), int(v.sum()), int(v.min()), int(v.max())) if len(v) else (0, 0, 0, 0)


def plan_filter_stats(plan: FilterPlan) -> dict:
    """The per-leaf values the reference records for every filter of a plan, aggregated
    (count, total, min, max), keyed by metric name.  Leaves without a filter (bits_per_key 0)
    record nothing; an empty VQF leaf skips bits_per_key (the reference would divide by
    zero, :202)."""
    if plan._stats is not None:
        return plan._stats
    segs = plan.segs
    n = segs["n_keys"].astype(np.int64)
    if plan.kind == BLOOM:
        has = segs["hash_count"] != 0
        words = 8 * segs["n_blocks"][has].astype(np.int64)        # PackedBloomFilter::word_count()
        st = {"word_count_stats": _agg(words), "byte_size_stats": _agg(8 * words),
              "bit_size_stats": _agg(64 * words),
              "bit_count_stats": _agg(512 * segs["n_blocks"][has].astype(np.int64)),  # header bit_count
              "item_count_stats": _agg(n[has])}
    else:
        has = segs["tag_bits"] != 0
        size = segs["payload_bytes"][has].astype(np.int64) - 32   # vqf_filter_size (:194)
        nz = n[has] > 0
        st = {"byte_size_stats": _agg(size), "bit_size_stats": _agg(8 * size),
              "item_count_stats": _agg(n[has]),
              "bits_per_key_stats": _agg((size[nz] * 8 + 4) // n[has][nz])}
    plan._stats = st
    return st


def record_filter_metrics(plan: FilterPlan, latency_usec: float | None = None) -> None:
    """Fold one built batch into BloomFilterMetrics / QuotientFilterMetrics, as the reference
    does per built leaf filter (filter_builder.hpp:139-147, :198-202)."""
    m = BloomFilterMetrics.instance() if plan.kind == BLOOM else QuotientFilterMetrics.instance()
    st = plan_filter_stats(plan)
    for name, agg in st.items():
        getattr(m, name).merge(*agg)
    if latency_usec is not None:
        leaves = st["item_count_stats"][0]
        if leaves:
            m.build_page_latency.add(leaves, latency_usec)


def build_all_filters(plan: FilterPlan, keys: KeyBatch, out=None, workspace=None, stream=None,
                      check: bool = True):
    """Build every planned filter into one device array (the filter half of
    TreeSerializeContext::build_all_pages).  Returns the output uint8 tensor."""
    torch = _torch()
    _require_device()
    if keys.n != plan.n_keys:
        raise TkvAmqError(abi.INVALID_ARGUMENT, f"plan covers {plan.n_keys} keys, got {keys.n}")
    dev = keys.data.device
    if out is None:
        out = torch.empty(max(plan.total_out_bytes, 1), dtype=torch.uint8, device=dev)
    elif out.numel() < plan.total_out_bytes:
        raise TkvAmqError(abi.INVALID_ARGUMENT,
                          f"output holds {out.numel()} bytes, the plan needs {plan.total_out_bytes}")
    if plan.workspace_bytes and workspace is None:
        workspace = torch.empty(plan.workspace_bytes, dtype=torch.uint8, device=dev)
    ws_bytes = 0 if workspace is None else workspace.numel() * workspace.element_size()
    if ws_bytes < plan.workspace_bytes:
        raise TkvAmqError(abi.INVALID_ARGUMENT,
                          f"workspace holds {ws_bytes} bytes, the plan needs {plan.workspace_bytes}")
    sh = _stream_handle(stream)
    t0 = time.perf_counter()
    # (_ex with the host plan: in a Bloom batch, leaves of 16- or 24-byte keys past 5 LDS windows
    # -- other key shapes past 16 -- take the tiled build, up to 40 such leaves per launch, and
    # the rest the batch kernels)
    L = abi.lib()
    if hasattr(L, "tkv_amq_build_ex"):
        st = L.tkv_amq_build_ex(plan.kind, _ptr(keys.data), _ptr(keys.offsets), keys.stride,
                                keys.n, _ptr(plan.device_segs(dev)), _ptr(plan.segs), plan.n_segs,
                                plan.max_seg_blocks, _ptr(out), _ptr(workspace), ws_bytes, sh)
        abi.check(st, "tkv_amq_build_ex")
    else:  # (an older library loaded through TKV_AMQ_LIB: the batch entry without the host plan)
        st = L.tkv_amq_build(plan.kind, _ptr(keys.data), _ptr(keys.offsets), keys.stride, keys.n,
                             _ptr(plan.device_segs(dev)), plan.n_segs, plan.max_seg_blocks,
                             _ptr(out), _ptr(workspace), ws_bytes, sh)
        abi.check(st, "tkv_amq_build")
    if check:
        # synchronous: the batch is known good, record its metrics with the build latency
        abi.check(abi.lib().tkv_amq_build_check(plan.kind, _ptr(workspace), ws_bytes, sh),
                  "vqf_insert (filter_builder.hpp:211)")
        record_filter_metrics(plan, (time.perf_counter() - t0) * 1e6)
    return out


def build_route(plan: FilterPlan, key_stride: int = 16, has_offsets: bool = False,
                aligned8: bool = True, workspace_bytes: int | None = None, ex: bool = True):
    """The route build_all_filters (ex: tkv_amq_build_ex with the host plan; else tkv_amq_build)
    takes for `plan` and such keys, without a device: (abi.BuildRoute, per-leaf abi.LEAF_*).
    workspace_bytes None: the plan's workspace (none when the plan needs none)."""
    ws = plan.workspace_bytes if workspace_bytes is None else int(workspace_bytes)
    out = abi.BuildRoute()
    leaves = np.zeros(plan.n_segs, dtype=np.uint8)
    st = abi.lib().tkv_amq_build_route(plan.kind, 0 if has_offsets else int(key_stride),
                                       int(bool(has_offsets)), int(bool(aligned8)), plan.n_segs,
                                       plan.n_keys, plan.max_seg_blocks,
                                       _ptr(plan.segs) if ex else None, int(ws > 0), ws,
                                       ctypes.byref(out), _ptr(leaves))
    abi.check(st, "tkv_amq_build_route")
    return out, leaves


class ProbeMetrics:
    """Device-side KeyQuery::Metrics counters (tkv_amq_probe_metrics) that probe launches add
    to; `collect()` reads them, `fold_into()` adds them to a host KeyQueryMetrics."""

    def __init__(self, device=None):
        torch = _torch()
        self.counts = torch.zeros(len(abi.PROBE_METRICS_FIELDS), dtype=torch.int64,
                                  device=device or "cuda")

    def reset(self) -> None:
        self.counts.zero_()

    def collect(self) -> dict:
        return dict(zip(abi.PROBE_METRICS_FIELDS, (int(v) for v in self.counts.cpu().tolist())))

    def fold_into(self, m: "KeyQueryMetrics", reset: bool = True) -> None:
        for k, v in self.collect().items():
            getattr(m, k).add(v)
        if reset:
            self.reset()


def _probe_opts(query_page_ids, truth, metrics):
    torch = _torch()
    keep = []
    pid = None
    if query_page_ids is not None:
        pid = query_page_ids.to(dtype=torch.int64).contiguous()
        keep.append(pid)
    tr = None
    if truth is not None:
        tr = truth.to(dtype=torch.uint8).contiguous()
        keep.append(tr)
    o = abi.ProbeOpts(None if pid is None else pid.data_ptr(), None if tr is None else tr.data_ptr(),
                      None if metrics is None else metrics.counts.data_ptr())
    return o, keep


def probe_filters(plan: FilterPlan, filters, queries: KeyBatch, query_seg, out=None, stream=None,
                  query_page_ids=None, truth=None, metrics: ProbeMetrics | None = None):
    """Batched KeyQuery filter test: result[i] = 0 iff the filter of segment query_seg[i]
    rejects queries[i] (reject_page == kTrue).  Optional, per query: the leaf page id asked
    about (a filter built for another page answers 1, kUnknown), the ground truth (1 = key is
    in the leaf) for the false-positive count, and device KeyQuery::Metrics counters."""
    torch = _torch()
    _require_device()
    dev = filters.device
    if out is None:
        out = torch.empty(queries.n, dtype=torch.uint8, device=dev)
    qs = query_seg.to(dtype=torch.int32)
    sh = _stream_handle(stream)
    if query_page_ids is None and truth is None and metrics is None:
        st = abi.lib().tkv_amq_probe(plan.kind, _ptr(filters), _ptr(plan.device_segs(dev)),
                                     plan.n_segs, _ptr(queries.data), _ptr(queries.offsets),
                                     queries.stride, queries.n, _ptr(qs), _ptr(out), sh)
    else:
        o, _keep = _probe_opts(query_page_ids, truth, metrics)
        st = abi.lib().tkv_amq_probe_ex(plan.kind, _ptr(filters), _ptr(plan.device_segs(dev)),
                                        plan.n_segs, _ptr(queries.data), _ptr(queries.offsets),
                                        queries.stride, queries.n, _ptr(qs), _ptr(out),
                                        ctypes.byref(o), sh)
        _hold(stream, *_keep)
    _hold(stream, qs)
    abi.check(st, "tkv_amq_probe")
    return out


def vqf_hash_val(keys: KeyBatch, stream=None):
    """vqf_hash_val for every key -> int64 tensor holding the u64 XXH64 bit patterns."""
    torch = _torch()
    _require_device()
    out = torch.empty(keys.n, dtype=torch.int64, device=keys.data.device)
    abi.check(abi.lib().tkv_amq_vqf_hash(_ptr(keys.data), _ptr(keys.offsets), keys.stride, keys.n,
                                         _ptr(out), _stream_handle(stream)), "tkv_amq_vqf_hash")
    return out


def vqf_probe_hashed(plan: FilterPlan, filters, hash_vals, query_seg, out=None, stream=None,
                     pair_query=None, query_page_ids=None, truth=None,
                     metrics: ProbeMetrics | None = None):
    """PackedVqfFilter::is_present for pre-hashed queries; pair i tests leaf query_seg[i]
    with hash_vals[pair_query[i]] (identity when pair_query is None).  The optional inputs
    are per pair, as in probe_filters."""
    torch = _torch()
    _require_device()
    dev = filters.device
    n = query_seg.numel()
    if out is None:
        out = torch.empty(n, dtype=torch.uint8, device=dev)
    qs = query_seg.to(dtype=torch.int32)
    pq = None if pair_query is None else pair_query.to(dtype=torch.int32)
    o, _keep = _probe_opts(query_page_ids, truth, metrics)
    abi.check(abi.lib().tkv_amq_vqf_probe_hashed_ex(_ptr(filters), _ptr(plan.device_segs(dev)),
                                                    plan.n_segs, _ptr(hash_vals), _ptr(pq), n,
                                                    _ptr(qs), _ptr(out), ctypes.byref(o),
                                                    _stream_handle(stream)),
              "tkv_amq_vqf_probe_hashed")
    _hold(stream, qs, pq, *_keep)
    return out


def bloom_query_hashes(keys: KeyBatch, k_max: int, stream=None):
    """BloomFilterQuery<KeyView> cache for a batch of queries (tree/key_query.hpp:78,97):
    one record per query (h0 + k_max-1 bit indices), computed once."""
    torch = _torch()
    _require_device()
    stride = int(abi.lib().tkv_amq_bloom_query_stride(k_max))
    out = torch.empty(max(keys.n, 1) * stride, dtype=torch.uint8, device=keys.data.device)
    abi.check(abi.lib().tkv_amq_bloom_hash(_ptr(keys.data), _ptr(keys.offsets), keys.stride, keys.n,
                                           k_max, _ptr(out), _stream_handle(stream)),
              "tkv_amq_bloom_hash")
    return out


def bloom_probe_hashed(plan: FilterPlan, filters, query_hashes, k_max: int, query_seg, out=None,
                       stream=None, pair_query=None, query_page_ids=None, truth=None,
                       metrics: ProbeMetrics | None = None):
    """PackedBloomFilter::query(BloomFilterQuery) for (query, leaf) pairs."""
    torch = _torch()
    _require_device()
    dev = filters.device
    n = query_seg.numel()
    if out is None:
        out = torch.empty(n, dtype=torch.uint8, device=dev)
    qs = query_seg.to(dtype=torch.int32)
    pq = None if pair_query is None else pair_query.to(dtype=torch.int32)
    o, _keep = _probe_opts(query_page_ids, truth, metrics)
    abi.check(abi.lib().tkv_amq_bloom_probe_hashed_ex(_ptr(filters), _ptr(plan.device_segs(dev)),
                                                      plan.n_segs, _ptr(query_hashes), k_max,
                                                      _ptr(pq), n, _ptr(qs), _ptr(out),
                                                      ctypes.byref(o), _stream_handle(stream)),
              "tkv_amq_bloom_probe_hashed")
    _hold(stream, qs, pq, *_keep)
    return out


def path_probe_workspace_bytes(n_queries: int, n_entries: int) -> int:
    """Device workspace tkv_amq_path_probe needs (host only; 0 for counts it refuses)."""
    return int(abi.lib().tkv_amq_path_probe_ws_bytes(int(n_queries), int(n_entries)))


@dataclass
class PathProbeResult:
    """What probe_paths leaves on the device: query i's candidates -- the leaves of its path
    the filters could not reject, in path order -- are cand_leaf[cand_begin[i]:cand_begin[i+1]]
    (and their entry indices cand_entry[...], if asked for).  Only the first
    cand_begin[n_queries] elements of cand_leaf / cand_entry are written."""
    cand_begin: object                   # int32 [n_queries + 1]
    cand_leaf: object                    # int32 [n_entries] capacity
    cand_entry: object = None            # int32 [n_entries] capacity, or None
    entry_result: object = None          # uint8 [n_entries], or None
    workspace: object = field(default=None, repr=False)

    def total(self) -> int:
        """Number of candidates (the one call here that synchronises)."""
        return int(self.cand_begin[-1].item())


def probe_paths(plan: FilterPlan, filters, queries: KeyBatch, path_begin, path_leaf, *,
                entry_result=None, want_entries: bool = False, query_page_ids=None, truth=None,
                metrics: ProbeMetrics | None = None, workspace=None, stream=None) -> PathProbeResult:
    """A batched multi-get's filter walk (tkv_amq_path_probe): query i would visit the leaves
    path_leaf[path_begin[i]:path_begin[i+1]] (segment indices of `plan`, in lookup order); each
    key is hashed once and every filter on its path is asked reject_page.  Returns the leaves
    still to search per query, compacted on the device.  entry_result (uint8 [n_entries], or
    True to allocate it) receives every entry's answer, exactly what the pair probes answer;
    query_page_ids, truth and metrics are per ENTRY, as they are per pair there.  `workspace`:
    a caller-owned uint8 tensor of path_probe_workspace_bytes() bytes (e.g. for graph capture)."""
    torch = _torch()
    _require_device()
    dev = filters.device
    n_entries = int(path_leaf.numel())
    pb = path_begin.to(dtype=torch.int32).contiguous()
    pl = path_leaf.to(dtype=torch.int32).contiguous()
    if pb.numel() != queries.n + 1:
        raise ValueError("path_begin must have one element per query plus one")
    if entry_result is True:
        entry_result = torch.empty(n_entries, dtype=torch.uint8, device=dev)
    cand_begin = torch.empty(queries.n + 1, dtype=torch.int32, device=dev)
    cand_leaf = torch.empty(n_entries, dtype=torch.int32, device=dev)
    cand_entry = torch.empty(n_entries, dtype=torch.int32, device=dev) if want_entries else None
    need = path_probe_workspace_bytes(queries.n, n_entries)
    if need == 0:
        raise TkvAmqError(abi.INVALID_ARGUMENT, "tkv_amq_path_probe: too many queries or entries")
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    o, _keep = _probe_opts(query_page_ids, truth, metrics)
    used = query_page_ids is not None or truth is not None or metrics is not None
    st = abi.lib().tkv_amq_path_probe(plan.kind, _ptr(filters), _ptr(plan.device_segs(dev)),
                                      plan.n_segs, _ptr(queries.data), _ptr(queries.offsets),
                                      queries.stride, queries.n, _ptr(pb), _ptr(pl), n_entries,
                                      _ptr(entry_result), _ptr(cand_begin), _ptr(cand_leaf),
                                      _ptr(cand_entry), ctypes.byref(o) if used else None,
                                      _ptr(workspace), int(workspace.numel()), _stream_handle(stream))
    _hold(stream, pb, pl, workspace, *_keep)
    abi.check(st, "tkv_amq_path_probe")
    return PathProbeResult(cand_begin, cand_leaf, cand_entry, entry_result, workspace)


# ---------------------------------------------------------------------------------------
# open built filters without a plan / scan their fill
# ---------------------------------------------------------------------------------------
@dataclass
class OpenedFilters:
    """What open_filters read from a buffer of built filters: a FilterPlan made of the segments
    the device reconstructed (it serves probe_filters, the hashed probes, probe_paths and
    scan_filters; building into it is not supported), the per-filter abi.OPEN_* code and the
    count of each code.  A filter that failed is a "no filter" segment of the plan: every probe
    answers 1 (kUnknown) for it."""
    plan: FilterPlan
    status: np.ndarray                   # uint32 [n_filters]
    summary: np.ndarray                  # uint32 [7]

    @property
    def all_ok(self) -> bool:
        return int(self.summary[abi.OPEN_OK]) == len(self.status)


def open_filters_device(kind: int, filters, n_filters: int, d_segs, d_status, d_summary=None,
                        offsets=None, stride: int = 0, page_size_log2: int = 0, stream=None) -> None:
    """The launch alone (tkv_amq_open_filters): device buffers in, nothing copied back, so it can
    be captured.  d_segs: uint8 [64 * n_filters]; d_status: int32 [n_filters]; d_summary: int32
    [7] or None; offsets: int64 [n_filters] on the device, or None."""
    _require_device()
    total = int(filters.numel()) if filters is not None else 0
    st = abi.lib().tkv_amq_open_filters(kind, _ptr(filters), total, _ptr(offsets), int(stride),
                                        int(page_size_log2), int(n_filters), _ptr(d_segs),
                                        _ptr(d_status), _ptr(d_summary), _stream_handle(stream))
    abi.check(st, "tkv_amq_open_filters")


def open_filters(kind: int, filters, offsets=None, stride: int = 0, page_size_log2: int = 0,
                 n_filters: int | None = None, stream=None) -> OpenedFilters:
    """Reconstruct and validate the segments of built filters from their bytes (a store
    restarting on a checkpoint, filter pages received from elsewhere).  `filters`: device uint8
    tensor.  Filter s lives at offsets[s] (payloads), at s * stride (payload slots) or in the
    page s << page_size_log2 (page images, as plan_filter_pages lays them out); n_filters
    defaults to len(offsets) or the number of whole slots in the buffer."""
    torch = _torch()
    _require_device()
    dev = filters.device
    d_off = None
    if offsets is not None:
        d_off = (offsets if hasattr(offsets, "data_ptr") else torch.from_numpy(
            np.ascontiguousarray(np.asarray(offsets, dtype=np.uint64)).view(np.int64))).to(
                device=dev, dtype=torch.int64).contiguous()
        n = int(d_off.numel()) if n_filters is None else int(n_filters)
    elif n_filters is not None:
        n = int(n_filters)
    elif stride:
        n = -(-int(filters.numel()) // int(stride))
    elif page_size_log2:
        n = -(-int(filters.numel()) >> int(page_size_log2))
    else:
        raise TkvAmqError(abi.INVALID_ARGUMENT, "open_filters: offsets, stride or page_size_log2")
    d_segs = torch.empty(max(n, 1) * 64, dtype=torch.uint8, device=dev)
    d_status = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    d_summary = torch.empty(7, dtype=torch.int32, device=dev)
    open_filters_device(kind, filters, n, d_segs, d_status, d_summary, d_off, stride,
                        page_size_log2, stream)
    _hold(stream, d_off, d_segs, d_status, d_summary)
    if stream is not None:
        stream.synchronize()
    segs = d_segs[:64 * n].cpu().numpy().view(abi.SEGMENT_DTYPE).copy()
    status = d_status[:n].cpu().numpy().view(np.uint32).copy()
    summary = d_summary.cpu().numpy().view(np.uint32).copy()
    plan = FilterPlan(kind, 0, segs, int(filters.numel()), 0,
                      int(segs["n_blocks"].max()) if n else 0, int(segs["n_keys"].sum()) if n else 0)
    plan._device[str(d_segs.device)] = d_segs[:64 * n] if n else d_segs[:0]
    return OpenedFilters(plan, status, summary)


def scan_filters_workspace_bytes(n_segs: int) -> int:
    """Device workspace tkv_amq_scan_filters needs (host only)."""
    return int(abi.lib().tkv_amq_scan_filters_ws_bytes(int(n_segs)))


def scan_filters_device(kind: int, filters, d_segs, n_segs: int, d_stats, workspace, stream=None) -> None:
    """The launches alone (tkv_amq_scan_filters), capturable.  d_stats: uint8 [32 * n_segs]."""
    _require_device()
    st = abi.lib().tkv_amq_scan_filters(kind, _ptr(filters), _ptr(d_segs), int(n_segs), _ptr(d_stats),
                                        _ptr(workspace), int(workspace.numel()) if workspace is not None else 0,
                                        _stream_handle(stream))
    abi.check(st, "tkv_amq_scan_filters")


def scan_filters(plan: FilterPlan, filters, stream=None) -> np.ndarray:
    """One read-only pass over the blocks of every filter of `plan` (built or opened): a
    FILTER_STATS_DTYPE record per filter -- set bits (Bloom) or occupied tag slots (VQF), the
    item count the payload header stores, full / empty blocks, the fullest block, and the VQF
    blocks that break a block invariant."""
    torch = _torch()
    _require_device()
    dev = filters.device
    n = plan.n_segs
    d_stats = torch.empty(max(n, 1) * 32, dtype=torch.uint8, device=dev)
    ws = torch.empty(scan_filters_workspace_bytes(n), dtype=torch.uint8, device=dev)
    scan_filters_device(plan.kind, filters, plan.device_segs(dev), n, d_stats, ws, stream)
    _hold(stream, d_stats, ws)
    if stream is not None:
        stream.synchronize()
    return d_stats[:32 * n].cpu().numpy().view(abi.FILTER_STATS_DTYPE).copy()


def filter_fill(plan: FilterPlan, stats: np.ndarray) -> np.ndarray:
    """Per filter: the fraction of its bits that are set (Bloom: occupied / (512 * n_blocks)) or
    of its tag slots that are taken (VQF: occupied / (n_blocks * slots)); 0 without a filter."""
    nb = plan.segs["n_blocks"].astype(np.float64)
    if plan.kind == BLOOM:
        cap = 512.0 * nb * (plan.segs["hash_count"] != 0)
    else:
        t = plan.segs["tag_bits"]
        cap = nb * np.where(t == 8, 48.0, np.where(t == 16, 28.0, 0.0))
    occ = stats["occupied"].astype(np.float64)
    return np.divide(occ, cap, out=np.zeros_like(occ), where=cap > 0)


# ---------------------------------------------------------------------------------------
# verify built filters against their keys (no false negatives, per leaf)
# ---------------------------------------------------------------------------------------
def verify_members_workspace_bytes(n_segs: int) -> int:
    """Device workspace tkv_amq_verify_members needs (host only)."""
    return int(abi.lib().tkv_amq_verify_members_ws_bytes(int(n_segs)))


def verify_members_device(kind: int, filters, d_segs, n_segs: int, max_seg_blocks: int, keys, key_offsets,
                          key_stride: int, n_keys: int, d_key_begin, d_result, d_total, workspace,
                          stream=None) -> None:
    """The launches alone (tkv_amq_verify_members), capturable: raw device tensors in, nothing
    copied back.  d_result: uint8 [16 * n_segs] (MEMBER_CHECK_DTYPE records); d_total: int64 [1]
    or None; d_key_begin: int64 [n_segs + 1] or None; key_offsets: int64 [n_keys + 1] or None."""
    _require_device()
    st = abi.lib().tkv_amq_verify_members(
        kind, _ptr(filters), _ptr(d_segs), int(n_segs), int(max_seg_blocks), _ptr(keys), _ptr(key_offsets),
        int(key_stride), int(n_keys), _ptr(d_key_begin), _ptr(d_result), _ptr(d_total), _ptr(workspace),
        int(workspace.numel()) if workspace is not None else 0, _stream_handle(stream))
    abi.check(st, "tkv_amq_verify_members")


def verify_members(plan_or_opened, filters, keys: KeyBatch, key_begin=None, stream=None,
                   max_seg_blocks: int | None = None) -> np.ndarray:
    """Does every key of every leaf pass its own filter?  One leaf-major device pass over the
    filters of a FilterPlan (or of an OpenedFilters) and the keys they hold: a
    MEMBER_CHECK_DTYPE record per leaf -- `missing`, the keys the filter rejects (false
    negatives: what tkv_amq_probe would answer 0 for), `first_missing`, the smallest such key
    index (abi.NONE_MISSING if none), and `flags` (abi.VERIFY_NO_FILTER: nothing to check;
    abi.VERIFY_ID_MISMATCH: the payload was built for another page; its keys are checked all the
    same).  Leaf s holds keys [key_begin[s], key_begin[s+1]) -- n_segs + 1 entries, host or
    device: the form for opened filters, whose segments do not record their key ranges -- or,
    without key_begin, the plan's own range.  max_seg_blocks: the LDS sizing hint (the plan's by
    default); the result never depends on it."""
    torch = _torch()
    _require_device()
    plan = plan_or_opened.plan if isinstance(plan_or_opened, OpenedFilters) else plan_or_opened
    dev = filters.device
    n = plan.n_segs
    d_kb = None
    if key_begin is not None:
        d_kb = (key_begin if hasattr(key_begin, "data_ptr") else torch.from_numpy(
            np.ascontiguousarray(np.asarray(key_begin, dtype=np.uint64)).view(np.int64))).to(
                device=dev, dtype=torch.int64).contiguous()
        if int(d_kb.numel()) != n + 1:
            raise TkvAmqError(abi.INVALID_ARGUMENT, "verify_members: key_begin needs n_segs + 1 entries")
    d_result = torch.empty(max(n, 1) * 16, dtype=torch.uint8, device=dev)
    d_total = torch.empty(1, dtype=torch.int64, device=dev)
    ws = torch.empty(verify_members_workspace_bytes(n), dtype=torch.uint8, device=dev)
    verify_members_device(plan.kind, filters, plan.device_segs(dev), n,
                          plan.max_seg_blocks if max_seg_blocks is None else max_seg_blocks, keys.data,
                          keys.offsets, keys.stride, keys.n, d_kb, d_result, d_total, ws, stream)
    _hold(stream, d_kb, d_result, d_total, ws)
    if stream is not None:
        stream.synchronize()
    return d_result[:16 * n].cpu().numpy().view(abi.MEMBER_CHECK_DTYPE).copy()


# ---------------------------------------------------------------------------------------
# leaf search: resolve a path probe's candidates to found keys
# ---------------------------------------------------------------------------------------
class FindCounts:
    """Device-side tkv_amq_find_counts that find_keys launches add to; `collect()` reads them."""

    def __init__(self, device=None):
        torch = _torch()
        self.counts = torch.zeros(len(abi.FIND_COUNTS_FIELDS), dtype=torch.int64, device=device or "cuda")

    def reset(self) -> None:
        self.counts.zero_()

    def collect(self) -> dict:
        return dict(zip(abi.FIND_COUNTS_FIELDS, (int(v) for v in self.counts.cpu().tolist())))


@dataclass
class FindResult:
    """What find_keys leaves on the device, per query: the global index (into the leaf keys) of
    the found key (-1, i.e. abi.NOT_FOUND as int64, if none), the leaf that holds it and the
    position of that candidate in cand_leaf (-1 if none); `state`: one abi.CAND_* byte per
    candidate position, if asked for.  `raw` is the tkv_amq_find_result array itself (uint8
    [16 * n_queries], abi.FIND_RESULT_DTYPE records); the three fields are views into it."""
    key_index: object                    # int64 [n_queries]
    leaf: object                         # int32 [n_queries]
    cand: object                         # int32 [n_queries]
    state: object = None                 # uint8 [n_cand], or None
    raw: object = field(default=None, repr=False)


def find_keys_device(kind: int, filters, d_segs, n_segs: int, queries, query_offsets, query_stride: int,
                     n_queries: int, cand_begin, cand_leaf, cand_entry, n_cand: int, leaf_keys,
                     leaf_key_offsets, leaf_key_stride: int, n_leaf_keys: int, d_key_begin, d_result,
                     d_state=None, flags: int = 0, d_query_page_ids=None, d_metrics=None, d_counts=None,
                     stream=None) -> None:
    """The launch alone (tkv_amq_find_keys), capturable behind probe_paths: raw device tensors in,
    nothing copied back.  cand_begin: int32 [n_queries + 1]; cand_leaf / cand_entry: int32
    [>= n_cand] (cand_entry may be None); d_result: uint8 [16 * n_queries]
    (abi.FIND_RESULT_DTYPE records); d_state: uint8 [n_cand] or None; d_key_begin: int64
    [n_segs + 1] or None; d_query_page_ids: int64 per path ENTRY or None; d_metrics: int64 [6]
    (ProbeMetrics.counts) or None; d_counts: int64 [4] (FindCounts.counts) or None."""
    _require_device()
    o = abi.ProbeOpts(None if d_query_page_ids is None else d_query_page_ids.data_ptr(), None,
                      None if d_metrics is None else d_metrics.data_ptr())
    used = d_query_page_ids is not None or d_metrics is not None
    st = abi.lib().tkv_amq_find_keys(
        kind, _ptr(filters), _ptr(d_segs), int(n_segs), _ptr(queries), _ptr(query_offsets), int(query_stride),
        int(n_queries), _ptr(cand_begin), _ptr(cand_leaf), _ptr(cand_entry), int(n_cand), _ptr(leaf_keys),
        _ptr(leaf_key_offsets), int(leaf_key_stride), int(n_leaf_keys), _ptr(d_key_begin), int(flags),
        _ptr(d_result), _ptr(d_state), ctypes.byref(o) if used else None, _ptr(d_counts),
        _stream_handle(stream))
    abi.check(st, "tkv_amq_find_keys")


def find_keys(plan_or_opened, filters, queries: KeyBatch, cands, leaf_keys: KeyBatch, *, key_begin=None,
              find_all: bool = False, want_state: bool = False, query_page_ids=None,
              metrics: ProbeMetrics | None = None, counts: FindCounts | None = None,
              stream=None) -> FindResult:
    """The leaf search behind the filters (tkv_amq_find_keys): query i's candidates -- a
    PathProbeResult of probe_paths, or a hand-made (cand_begin, cand_leaf[, cand_entry]) CSR list
    of segment indices of `plan` -- are searched in path order for queries[i]: a lower bound over
    the leaf's sorted keys, then an equality test.  The walk ends at the first leaf that holds
    the key (find_all=True searches every candidate; the result is still the first hit).  Leaf s
    holds leaf_keys [key_begin[s], key_begin[s+1]) -- n_segs + 1 entries, host or device: the form
    for opened filters -- or, without key_begin, the plan's own range; each leaf's keys must be in
    ascending byte order.  With `metrics`, every searched candidate without the key that a filter
    had let through adds 1 to filter_false_positive_count (query_page_ids: per path ENTRY, as
    given to probe_paths; needs the candidates' entry indices): together with probe_paths'
    counts, KeyQuery::Metrics without host truth.  `filters` is read for the page-id check only
    and may be None otherwise.  Nothing is copied back: the result stays on the device."""
    torch = _torch()
    _require_device()
    plan = plan_or_opened.plan if isinstance(plan_or_opened, OpenedFilters) else plan_or_opened
    dev = queries.data.device
    if isinstance(cands, PathProbeResult):
        cb, cl, ce = cands.cand_begin, cands.cand_leaf, cands.cand_entry
    else:
        cb, cl = cands[0], cands[1]
        ce = cands[2] if len(cands) > 2 else None
    cb = cb.to(dtype=torch.int32).contiguous()
    cl = cl.to(dtype=torch.int32).contiguous()
    ce = None if ce is None else ce.to(dtype=torch.int32).contiguous()
    if cb.numel() != queries.n + 1:
        raise ValueError("cand_begin must have one element per query plus one")
    n_cand = int(cl.numel())
    n = plan.n_segs
    d_kb = None
    if key_begin is not None:
        d_kb = (key_begin if hasattr(key_begin, "data_ptr") else torch.from_numpy(
            np.ascontiguousarray(np.asarray(key_begin, dtype=np.uint64)).view(np.int64))).to(
                device=dev, dtype=torch.int64).contiguous()
        if int(d_kb.numel()) != n + 1:
            raise TkvAmqError(abi.INVALID_ARGUMENT, "find_keys: key_begin needs n_segs + 1 entries")
    pid = None if query_page_ids is None else query_page_ids.to(dtype=torch.int64).contiguous()
    raw = torch.empty(max(queries.n, 1) * 16, dtype=torch.uint8, device=dev)
    state = torch.empty(n_cand, dtype=torch.uint8, device=dev) if want_state else None
    find_keys_device(plan.kind, filters, plan.device_segs(dev) if n else None, n, queries.data,
                     queries.offsets, queries.stride, queries.n, cb, cl, ce, n_cand, leaf_keys.data,
                     leaf_keys.offsets, leaf_keys.stride, leaf_keys.n, d_kb, raw, state,
                     abi.FIND_ALL if find_all else 0, pid, None if metrics is None else metrics.counts,
                     None if counts is None else counts.counts, stream)
    _hold(stream, cb, cl, ce, d_kb, pid, raw, state)
    rec = raw[:16 * queries.n].view(torch.int64).view(queries.n, 2)
    lc = raw[:16 * queries.n].view(torch.int32).view(queries.n, 4)
    return FindResult(rec[:, 0], lc[:, 2], lc[:, 3], state, raw)


# ---------------------------------------------------------------------------------------
# tree walk: resolve each lookup to the path the probe and the search start from
# ---------------------------------------------------------------------------------------
class TreeIndex:
    """The flat tree tkv_amq_walk_paths descends, built on the host from a nested description and
    uploaded once.

    A node is a dict: "pivot_keys": its pivot_count + 1 keys k0..kp (bytes; k0 and kp bound the
    node and are never compared), "children": one per pivot -- all nodes, or all leaves
    {"leaf": plan segment index, "page_id": int} --, "levels": the update buffer, newest first,
    each a list of segments {"leaf": int, "page_id": int, "active": bit set of pivots,
    "flushed": {pivot: flushed item upper bound}}, and "page_id" (the root's is not stored).
    The limits are PackedNodePage's (tree/packed_node_page.hpp:42-223): at most 64 pivots and 63
    segments per node; levels: the 7 the flat record holds (the reference's page holds 6).  Node 0
    is the root; nodes are numbered breadth first."""

    def __init__(self, nodes, segments, children, flushed_bounds, pivot_keys):
        self.nodes = np.ascontiguousarray(nodes, dtype=abi.TREE_NODE_DTYPE)
        self.segments = np.ascontiguousarray(segments, dtype=abi.TREE_SEGMENT_DTYPE)
        self.children = np.ascontiguousarray(children, dtype=abi.TREE_CHILD_DTYPE)
        self.flushed_bounds = np.ascontiguousarray(flushed_bounds, dtype=np.uint32)
        self.pivot_keys = [bytes(k) for k in pivot_keys]
        self._device = {}

    @staticmethod
    def _check_node(node, height_of):
        keys, kids, levels = node["pivot_keys"], node["children"], node.get("levels", [])
        n = len(kids)
        if not 1 <= n <= abi.TREE_MAX_PIVOTS:
            raise ValueError(f"a node has 1..{abi.TREE_MAX_PIVOTS} pivots, not {n}")
        if len(keys) != n + 1:
            raise ValueError(f"a node of {n} pivots owns {n + 1} pivot keys, not {len(keys)}")
        if len(levels) > abi.TREE_MAX_LEVELS:
            raise ValueError(f"a node has at most {abi.TREE_MAX_LEVELS} levels, not {len(levels)}")
        n_seg = sum(len(lv) for lv in levels)
        if n_seg > abi.TREE_MAX_SEGMENTS:
            raise ValueError(f"a node has at most {abi.TREE_MAX_SEGMENTS} segments, not {n_seg}")
        kinds = {"pivot_keys" in c for c in kids}
        if len(kinds) != 1:
            raise ValueError("a node's children are all nodes or all leaves")
        heights = {height_of(c) for c in kids}
        if len(heights) != 1:
            raise ValueError("a node's children have one height")
        for lv in levels:
            for s in lv:
                if int(s.get("active", 0)) >> n or any(not 0 <= int(p) < n for p in s.get("flushed", {})):
                    raise ValueError("a segment names a pivot the node does not have")
        return heights.pop() + 1

    @classmethod
    def from_description(cls, root) -> "TreeIndex":
        heights = {}

        def height_of(d):
            if "pivot_keys" not in d:
                return 0
            if id(d) not in heights:
                heights[id(d)] = cls._check_node(d, height_of)
            return heights[id(d)]

        if height_of(root) > abi.WALK_MAX_DEPTH:
            raise ValueError(f"a tree has at most {abi.WALK_MAX_DEPTH} levels of nodes")
        order, at = [root], 0
        while at < len(order):  # breadth first: a node's children get consecutive numbers
            order.extend(c for c in order[at]["children"] if "pivot_keys" in c)
            at += 1
        number = {id(d): i for i, d in enumerate(order)}
        nodes = np.zeros(len(order), dtype=abi.TREE_NODE_DTYPE)
        segs, kids, bounds, keys = [], [], [], []
        for i, d in enumerate(order):
            levels = d.get("levels", [])
            nd = nodes[i]
            nd["pivot_key_begin"], nd["seg_begin"], nd["child_begin"] = len(keys), len(segs), len(kids)
            nd["pivot_count"], nd["height"], nd["level_count"] = len(d["children"]), heights[id(d)], len(levels)
            start = np.cumsum([0] + [len(lv) for lv in levels])
            nd["level_start"][:len(start)] = start
            nd["level_start"][len(start):] = start[-1]
            keys.extend(bytes(k) for k in d["pivot_keys"])
            for c in d["children"]:
                kids.append((int(c.get("page_id", 0)), number[id(c)] if "pivot_keys" in c else int(c["leaf"]), 0))
            for lv in levels:
                for s in lv:
                    fl = {int(p): int(b) for p, b in s.get("flushed", {}).items()}
                    segs.append((int(s.get("page_id", 0)), int(s.get("active", 0)),
                                 sum(1 << p for p in fl), int(s["leaf"]), len(bounds)))
                    bounds.extend(fl[p] for p in sorted(fl))
        return cls(nodes, np.array(segs, dtype=abi.TREE_SEGMENT_DTYPE),
                   np.array(kids, dtype=abi.TREE_CHILD_DTYPE), np.array(bounds, dtype=np.uint32), keys)

    def describe(self, node: int = 0, page_id: int = 0) -> dict:
        """The nested description of the subtree under `node` (from_description's inverse)."""
        nd = self.nodes[node]
        n, kb, sb, cb = int(nd["pivot_count"]), int(nd["pivot_key_begin"]), int(nd["seg_begin"]), \
            int(nd["child_begin"])
        levels = []
        for lv in range(int(nd["level_count"])):
            level = []
            for s in self.segments[sb + int(nd["level_start"][lv]):sb + int(nd["level_start"][lv + 1])]:
                fp, fb = int(s["flushed_pivots"]), int(s["flushed_begin"])
                pivots = [p for p in range(64) if fp >> p & 1]
                level.append({"leaf": int(s["leaf"]), "page_id": int(s["leaf_page_id"]),
                              "active": int(s["active_pivots"]),
                              "flushed": {p: int(self.flushed_bounds[fb + r]) for r, p in enumerate(pivots)}})
            levels.append(level)
        kids = []
        for c in self.children[cb:cb + n]:
            if int(nd["height"]) > 1:
                kids.append(self.describe(int(c["index"]), int(c["page_id"])))
            else:
                kids.append({"leaf": int(c["index"]), "page_id": int(c["page_id"])})
        return {"pivot_keys": self.pivot_keys[kb:kb + n + 1], "children": kids, "levels": levels,
                "page_id": page_id}

    def pivot_key_batch(self, device=None) -> KeyBatch:
        return KeyBatch.from_host(self.pivot_keys, device)

    def device(self, device=None):
        """(nodes, segments, children, flushed_bounds, pivot keys) on the device: uint8 views of the
        records, int32 bounds and a KeyBatch; uploaded once per device."""
        torch = _torch()
        dev = torch.device(device or "cuda")
        if dev not in self._device:
            def up(a):
                raw = np.frombuffer(a.tobytes(), dtype=np.uint8)
                return torch.from_numpy(raw.copy() if len(raw) else np.zeros(16, np.uint8)).to(dev)
            b = self.flushed_bounds.view(np.int32)
            self._device[dev] = (up(self.nodes), up(self.segments), up(self.children),
                                 torch.from_numpy(b.copy() if len(b) else np.zeros(1, np.int32)).to(dev),
                                 self.pivot_key_batch(dev))
        return self._device[dev]


def walk_paths_workspace_bytes(n_queries: int) -> int:
    """Device workspace tkv_amq_walk_paths needs (host only; 0 for counts it refuses)."""
    return int(abi.lib().tkv_amq_walk_paths_ws_bytes(int(n_queries)))


@dataclass
class WalkResult:
    """What walk_paths leaves on the device: query i's path is entries
    [path_begin[i], path_begin[i+1]) of path_leaf (plan segment indices, in lookup order) and of
    each optional array; only entries below min(needed, capacity) are written."""
    path_begin: object                   # int32 [n_queries + 1]
    path_leaf: object                    # int32 [capacity]
    path_page_id: object = None          # int64 [capacity], or None
    path_flushed: object = None          # int32 [capacity], or None
    path_where: object = None            # int16 [capacity] (depth << 8 | level), or None
    needed: object = None                # int64 [1]: the unclamped total
    capacity: int = 0
    workspace: object = field(default=None, repr=False)

    def total(self) -> int:
        """Number of entries written (synchronises)."""
        return int(self.path_begin[-1].item())


def walk_paths_device(d_nodes, n_nodes: int, d_segments, n_segments: int, d_children, n_children: int,
                      d_flushed_bounds, n_flushed_bounds: int, pivot_keys, pivot_key_offsets,
                      pivot_key_stride: int, n_pivot_keys: int, queries, query_offsets, query_stride: int,
                      n_queries: int, d_path_begin, d_path_leaf, path_capacity: int, workspace,
                      d_path_page_id=None, d_path_flushed=None, d_path_where=None, d_needed=None,
                      stream=None) -> None:
    """The launch alone (tkv_amq_walk_paths), capturable in front of probe_paths: raw device tensors
    in, nothing allocated, nothing copied back."""
    _require_device()
    st = abi.lib().tkv_amq_walk_paths(
        _ptr(d_nodes), int(n_nodes), _ptr(d_segments), int(n_segments), _ptr(d_children), int(n_children),
        _ptr(d_flushed_bounds), int(n_flushed_bounds), _ptr(pivot_keys), _ptr(pivot_key_offsets),
        int(pivot_key_stride), int(n_pivot_keys), _ptr(queries), _ptr(query_offsets), int(query_stride),
        int(n_queries), _ptr(d_path_begin), _ptr(d_path_leaf), _ptr(d_path_page_id), _ptr(d_path_flushed),
        _ptr(d_path_where), int(path_capacity), _ptr(d_needed), _ptr(workspace),
        0 if workspace is None else int(workspace.numel()), _stream_handle(stream))
    abi.check(st, "tkv_amq_walk_paths")


def walk_paths(tree: TreeIndex, queries: KeyBatch, capacity: int | None = None, want_page_ids: bool = False,
               want_flushed: bool = False, want_where: bool = False, workspace=None,
               stream=None) -> WalkResult:
    """Each query's ordered list of leaves (tkv_amq_walk_paths): the CSR list probe_paths and
    find_keys start from.  With a `capacity` the call is asynchronous; entries past it are counted
    in `needed` and not written.  capacity=None is the one synchronising convenience: the walk runs
    once with capacity 0, `needed` is read back, and it runs again with exactly that capacity."""
    torch = _torch()
    _require_device()
    dev = queries.data.device
    d_nodes, d_segs, d_kids, d_bounds, pk = tree.device(dev)
    need = walk_paths_workspace_bytes(queries.n)
    if need == 0:
        raise TkvAmqError(abi.INVALID_ARGUMENT, "tkv_amq_walk_paths: too many queries")
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    begin = torch.empty(queries.n + 1, dtype=torch.int32, device=dev)
    needed = torch.empty(1, dtype=torch.int64, device=dev)

    def run(cap, leaf, page, flushed, where):
        walk_paths_device(d_nodes, len(tree.nodes), d_segs, len(tree.segments), d_kids, len(tree.children),
                          d_bounds, len(tree.flushed_bounds), pk.data, pk.offsets, pk.stride, pk.n,
                          queries.data, queries.offsets, queries.stride, queries.n, begin, leaf, cap,
                          workspace, page, flushed, where, needed, stream)

    if capacity is None:
        run(0, None, None, None, None)
        if stream is not None:
            stream.synchronize()
        capacity = int(needed.item())
    capacity = int(capacity)
    leaf = torch.empty(max(capacity, 1), dtype=torch.int32, device=dev)
    page = torch.empty(max(capacity, 1), dtype=torch.int64, device=dev) if want_page_ids else None
    flushed = torch.empty(max(capacity, 1), dtype=torch.int32, device=dev) if want_flushed else None
    where = torch.empty(max(capacity, 1), dtype=torch.int16, device=dev) if want_where else None
    run(capacity, leaf, page, flushed, where)
    _hold(stream, workspace, begin, needed, leaf, page, flushed, where)
    return WalkResult(begin, leaf[:capacity], None if page is None else page[:capacity],
                      None if flushed is None else flushed[:capacity],
                      None if where is None else where[:capacity], needed, capacity, workspace)

# ---------------------------------------------------------------------------------------
# fused point lookup: root to found key in one launch
# ---------------------------------------------------------------------------------------
class GetCounts:
    """Device-side tkv_amq_get_counts that get_keys launches add to; `collect()` reads them."""

    def __init__(self, device=None):
        torch = _torch()
        self.counts = torch.zeros(len(abi.GET_COUNTS_FIELDS), dtype=torch.int64, device=device or "cuda")

    def reset(self) -> None:
        self.counts.zero_()

    def collect(self) -> dict:
        return dict(zip(abi.GET_COUNTS_FIELDS, (int(v) for v in self.counts.cpu().tolist())))


@dataclass
class GetResult:
    """What get_keys leaves on the device, per query: the global index (into the leaf keys) of the
    found key (-1, i.e. abi.NOT_FOUND as int64, if none), the leaf that holds it (-1 if none) and
    `where`, depth << 8 | level of the entry that held it (level abi.WALK_LEAF_LEVEL: the child
    leaf; -1 if none); `visits`: the number of entries the lookup visited, if asked for.  `raw` is
    the tkv_amq_get_result array itself (uint8 [16 * n_queries], abi.GET_RESULT_DTYPE records);
    the three fields are views into it."""
    key_index: object                    # int64 [n_queries]
    leaf: object                         # int32 [n_queries]
    where: object                        # int32 [n_queries]
    visits: object = None                # int32 [n_queries], or None
    raw: object = field(default=None, repr=False)


def get_keys_device(kind: int, filters, d_segs, n_segs: int, d_nodes, n_nodes: int, d_segments,
                    n_segments: int, d_children, n_children: int, d_flushed_bounds, n_flushed_bounds: int,
                    pivot_keys, pivot_key_offsets, pivot_key_stride: int, n_pivot_keys: int, queries,
                    query_offsets, query_stride: int, n_queries: int, leaf_keys, leaf_key_offsets,
                    leaf_key_stride: int, n_leaf_keys: int, d_key_begin, d_result, d_query_visits=None,
                    flags: int = 0, d_metrics=None, d_counts=None, stream=None) -> None:
    """The launch alone (tkv_amq_get_keys), capturable: raw device tensors in, nothing allocated,
    nothing copied back.  The tree as walk_paths_device takes it, the leaf keys as find_keys_device
    takes them; d_result: uint8 [16 * n_queries] (abi.GET_RESULT_DTYPE records); d_query_visits:
    int32 [n_queries] or None; d_metrics: int64 [6] (ProbeMetrics.counts) or None; d_counts: int64
    [6] (GetCounts.counts) or None."""
    _require_device()
    st = abi.lib().tkv_amq_get_keys(
        kind, _ptr(filters), _ptr(d_segs), int(n_segs), _ptr(d_nodes), int(n_nodes), _ptr(d_segments),
        int(n_segments), _ptr(d_children), int(n_children), _ptr(d_flushed_bounds), int(n_flushed_bounds),
        _ptr(pivot_keys), _ptr(pivot_key_offsets), int(pivot_key_stride), int(n_pivot_keys), _ptr(queries),
        _ptr(query_offsets), int(query_stride), int(n_queries), _ptr(leaf_keys), _ptr(leaf_key_offsets),
        int(leaf_key_stride), int(n_leaf_keys), _ptr(d_key_begin), int(flags), _ptr(d_result),
        _ptr(d_query_visits), _ptr(d_metrics), _ptr(d_counts), _stream_handle(stream))
    abi.check(st, "tkv_amq_get_keys")


def get_keys(plan_or_opened, filters, tree: TreeIndex, queries: KeyBatch, leaf_keys: KeyBatch, *,
             key_begin=None, check_page_ids: bool = False, want_visits: bool = False,
             metrics: ProbeMetrics | None = None, counts: GetCounts | None = None,
             stream=None) -> GetResult:
    """A batch of point lookups in one launch (tkv_amq_get_keys): each query descends `tree`, asks
    the filter of every entry on its way (hashed once), searches the leaves whose filters say
    maybe, and ends at the first leaf that holds its key -- skipping the rest of a level when the
    key is found below the segment's flushed item upper bound, as the reference does.  What
    walk_paths -> probe_paths -> find_keys compute for a tree without flushed bounds, without a
    path in memory and without a visit below the hit.  Leaf s holds leaf_keys [key_begin[s],
    key_begin[s+1]) or, without key_begin, the plan's own range, in ascending byte order.
    check_page_ids: a filter whose stored page id differs from the tree's id of the leaf cannot
    reject.  `metrics` takes KeyQuery::Metrics (the false positives included), `counts` the
    lookup's own tallies.  Nothing is copied back: the result stays on the device."""
    torch = _torch()
    _require_device()
    plan = plan_or_opened.plan if isinstance(plan_or_opened, OpenedFilters) else plan_or_opened
    dev = queries.data.device
    n = plan.n_segs
    d_kb = None
    if key_begin is not None:
        d_kb = (key_begin if hasattr(key_begin, "data_ptr") else torch.from_numpy(
            np.ascontiguousarray(np.asarray(key_begin, dtype=np.uint64)).view(np.int64))).to(
                device=dev, dtype=torch.int64).contiguous()
        if int(d_kb.numel()) != n + 1:
            raise TkvAmqError(abi.INVALID_ARGUMENT, "get_keys: key_begin needs n_segs + 1 entries")
    d_nodes, d_segments, d_kids, d_bounds, pk = tree.device(dev)
    raw = torch.empty(max(queries.n, 1) * 16, dtype=torch.uint8, device=dev)
    visits = torch.empty(max(queries.n, 1), dtype=torch.int32, device=dev) if want_visits else None
    get_keys_device(plan.kind, filters if n else None, plan.device_segs(dev) if n else None, n, d_nodes,
                    len(tree.nodes), d_segments, len(tree.segments), d_kids, len(tree.children), d_bounds,
                    len(tree.flushed_bounds), pk.data, pk.offsets, pk.stride, pk.n, queries.data,
                    queries.offsets, queries.stride, queries.n, leaf_keys.data, leaf_keys.offsets,
                    leaf_keys.stride, leaf_keys.n, d_kb, raw, visits,
                    abi.GET_CHECK_PAGE_ID if check_page_ids else 0,
                    None if metrics is None else metrics.counts, None if counts is None else counts.counts,
                    stream)
    _hold(stream, d_kb, raw, visits)
    rec = raw[:16 * queries.n].view(torch.int64).view(queries.n, 2)
    lc = raw[:16 * queries.n].view(torch.int32).view(queries.n, 4)
    return GetResult(rec[:, 0], lc[:, 2], lc[:, 3], None if visits is None else visits[:queries.n], raw)


# ---------------------------------------------------------------------------------------
# point lookup with values: the same descent, the found items folded as combine_in_place folds them
# ---------------------------------------------------------------------------------------
class ValueCounts:
    """Device-side tkv_amq_value_counts that get_values launches add to; `collect()` reads them."""

    def __init__(self, device=None):
        torch = _torch()
        self.counts = torch.zeros(len(abi.VALUE_COUNTS_FIELDS), dtype=torch.int64, device=device or "cuda")

    def reset(self) -> None:
        self.counts.zero_()

    def collect(self) -> dict:
        return dict(zip(abi.VALUE_COUNTS_FIELDS, (int(v) for v in self.counts.cpu().tolist())))


@dataclass
class ValueResult:
    """What get_values leaves on the device: `raw`, the tkv_amq_value_result array (uint8 [32 *
    n_queries], abi.VALUE_RESULT_DTYPE records), views of its key_index, leaf and where (as
    GetResult's), `visits` if asked for and, with gather=out_stride, `slots` (uint8 [n_queries,
    out_stride]; bytes past a value's length are not written) and `lengths` (int32 [n_queries], the
    full data length of each value)."""
    key_index: object                    # int64 [n_queries]
    leaf: object                         # int32 [n_queries]
    where: object                        # int32 [n_queries]
    visits: object = None                # int32 [n_queries], or None
    raw: object = field(default=None, repr=False)
    slots: object = None
    lengths: object = None

    def records(self) -> np.ndarray:
        """The records on the host (a copy; synchronises)."""
        n = int(self.key_index.numel())
        return self.raw[:32 * n].cpu().numpy().view(abi.VALUE_RESULT_DTYPE)


def get_values_device(kind: int, filters, d_segs, n_segs: int, d_nodes, n_nodes: int, d_segments,
                      n_segments: int, d_children, n_children: int, d_flushed_bounds, n_flushed_bounds: int,
                      pivot_keys, pivot_key_offsets, pivot_key_stride: int, n_pivot_keys: int, queries,
                      query_offsets, query_stride: int, n_queries: int, leaf_keys, leaf_key_offsets,
                      leaf_key_stride: int, n_leaf_keys: int, d_key_begin, leaf_values, leaf_value_offsets,
                      leaf_value_stride: int, leaf_values_bytes: int, d_result, d_query_visits=None,
                      flags: int = 0, d_metrics=None, d_counts=None, stream=None) -> None:
    """The launch alone (tkv_amq_get_values), capturable: get_keys_device's arguments and the
    leaves' values (bytes, offsets or a fixed stride, the buffer's size); d_result: uint8 [32 *
    n_queries] (abi.VALUE_RESULT_DTYPE records); d_counts: int64 [8] (ValueCounts.counts) or None."""
    _require_device()
    st = abi.lib().tkv_amq_get_values(
        kind, _ptr(filters), _ptr(d_segs), int(n_segs), _ptr(d_nodes), int(n_nodes), _ptr(d_segments),
        int(n_segments), _ptr(d_children), int(n_children), _ptr(d_flushed_bounds), int(n_flushed_bounds),
        _ptr(pivot_keys), _ptr(pivot_key_offsets), int(pivot_key_stride), int(n_pivot_keys), _ptr(queries),
        _ptr(query_offsets), int(query_stride), int(n_queries), _ptr(leaf_keys), _ptr(leaf_key_offsets),
        int(leaf_key_stride), int(n_leaf_keys), _ptr(d_key_begin), _ptr(leaf_values), _ptr(leaf_value_offsets),
        int(leaf_value_stride), int(leaf_values_bytes), int(flags), _ptr(d_result), _ptr(d_query_visits),
        _ptr(d_metrics), _ptr(d_counts), _stream_handle(stream))
    abi.check(st, "tkv_amq_get_values")


def gather_values_device(d_result, n_queries: int, leaf_values, leaf_value_offsets, leaf_value_stride: int,
                         leaf_values_bytes: int, n_leaf_keys: int, d_out, out_stride: int, d_value_len,
                         stream=None) -> None:
    """The launch alone (tkv_amq_gather_values), capturable behind get_values_device: d_out: uint8
    [n_queries * out_stride]; d_value_len: int32 [n_queries]."""
    _require_device()
    st = abi.lib().tkv_amq_gather_values(
        _ptr(d_result), int(n_queries), _ptr(leaf_values), _ptr(leaf_value_offsets), int(leaf_value_stride),
        int(leaf_values_bytes), int(n_leaf_keys), _ptr(d_out), int(out_stride), _ptr(d_value_len),
        _stream_handle(stream))
    abi.check(st, "tkv_amq_gather_values")


def get_values(plan_or_opened, filters, tree: TreeIndex, queries: KeyBatch, leaf_keys: KeyBatch,
               leaf_values: KeyBatch, *, key_begin=None, check_page_ids: bool = False,
               want_visits: bool = False, metrics: ProbeMetrics | None = None,
               counts: ValueCounts | None = None, gather: int | None = None, stream=None) -> ValueResult:
    """A batch of point lookups from keys to resolved values (tkv_amq_get_values): get_keys'
    descent, with every found item's packed value (an op byte, then the data; value i belongs to
    leaf key i, `leaf_values` in either KeyBatch form) folded as the reference's combine_in_place
    folds it -- ADD_I32 deltas are summed through the older levels and the child until a WRITE or a
    DELETE resolves them.  gather=out_stride also runs tkv_amq_gather_values behind it: each
    value's bytes in a slot of out_stride bytes, and its full length.  Nothing is copied back."""
    torch = _torch()
    _require_device()
    plan = plan_or_opened.plan if isinstance(plan_or_opened, OpenedFilters) else plan_or_opened
    dev = queries.data.device
    n = plan.n_segs
    d_kb = None
    if key_begin is not None:
        d_kb = (key_begin if hasattr(key_begin, "data_ptr") else torch.from_numpy(
            np.ascontiguousarray(np.asarray(key_begin, dtype=np.uint64)).view(np.int64))).to(
                device=dev, dtype=torch.int64).contiguous()
        if int(d_kb.numel()) != n + 1:
            raise TkvAmqError(abi.INVALID_ARGUMENT, "get_values: key_begin needs n_segs + 1 entries")
    if leaf_values.n != leaf_keys.n:
        raise TkvAmqError(abi.INVALID_ARGUMENT, "get_values: one value per leaf key")
    d_nodes, d_segments, d_kids, d_bounds, pk = tree.device(dev)
    nq = queries.n
    raw = torch.empty(max(nq, 1) * 32, dtype=torch.uint8, device=dev)
    visits = torch.empty(max(nq, 1), dtype=torch.int32, device=dev) if want_visits else None
    v_bytes = int(leaf_values.data.numel())
    get_values_device(plan.kind, filters if n else None, plan.device_segs(dev) if n else None, n, d_nodes,
                      len(tree.nodes), d_segments, len(tree.segments), d_kids, len(tree.children), d_bounds,
                      len(tree.flushed_bounds), pk.data, pk.offsets, pk.stride, pk.n, queries.data,
                      queries.offsets, queries.stride, nq, leaf_keys.data, leaf_keys.offsets,
                      leaf_keys.stride, leaf_keys.n, d_kb, leaf_values.data, leaf_values.offsets,
                      leaf_values.stride, v_bytes, raw, visits,
                      abi.GET_CHECK_PAGE_ID if check_page_ids else 0,
                      None if metrics is None else metrics.counts, None if counts is None else counts.counts,
                      stream)
    slots = lengths = None
    if gather is not None:
        slots = torch.empty((max(nq, 1), int(gather)), dtype=torch.uint8, device=dev)
        lengths = torch.empty(max(nq, 1), dtype=torch.int32, device=dev)
        gather_values_device(raw, nq, leaf_values.data, leaf_values.offsets, leaf_values.stride, v_bytes,
                             leaf_values.n, slots, int(gather), lengths, stream)
        slots, lengths = slots[:nq], lengths[:nq]
    _hold(stream, d_kb, raw, visits, slots, lengths)
    rec = raw[:32 * nq].view(torch.int64).view(nq, 4)
    lc = raw[:32 * nq].view(torch.int32).view(nq, 8)
    return ValueResult(rec[:, 0], lc[:, 4], lc[:, 5], None if visits is None else visits[:nq], raw, slots, lengths)


# ---------------------------------------------------------------------------------------
# leaf update: a batch of two-run merges (the update's edits over the leaves' items) on the device
# ---------------------------------------------------------------------------------------
class MergeCounts:
    """Device-side tkv_amq_merge_counts that merge_leaves launches add to; `collect()` reads them."""

    def __init__(self, device=None):
        torch = _torch()
        self.counts = torch.zeros(len(abi.MERGE_COUNTS_FIELDS), dtype=torch.int64, device=device or "cuda")

    def reset(self) -> None:
        self.counts.zero_()

    def collect(self) -> dict:
        return dict(zip(abi.MERGE_COUNTS_FIELDS, (int(v) for v in self.counts.cpu().tolist())))


def merge_run(keys: KeyBatch, values: KeyBatch, d_begin=None) -> abi.MergeRun:
    """tkv_amq_merge_run of one side: its keys and its packed values (value i belongs to key i, either
    in either KeyBatch form) and, for the merge, d_begin (int64 [n_jobs + 1] on the device).  The
    struct holds addresses only: the caller keeps the tensors alive."""
    if values.n != keys.n:
        raise TkvAmqError(abi.INVALID_ARGUMENT, "merge_run: one value per key")

    def addr(t):
        return None if t is None or int(t.numel()) == 0 else t.data_ptr()

    return abi.MergeRun(addr(keys.data), addr(keys.offsets), addr(values.data), addr(values.offsets),
                        addr(d_begin), keys.n, int(values.data.numel()), int(keys.stride), int(values.stride))


def merge_leaves_workspace_bytes(n_jobs: int, n_newer: int, n_older: int) -> int:
    """tkv_amq_merge_leaves_ws_bytes (0: counts the call refuses)."""
    return int(abi.lib().tkv_amq_merge_leaves_ws_bytes(int(n_jobs), int(n_newer), int(n_older)))


def gather_merged_workspace_bytes(out_capacity: int) -> int:
    """tkv_amq_gather_merged_ws_bytes."""
    return int(abi.lib().tkv_amq_gather_merged_ws_bytes(int(out_capacity)))


def merge_values_bound(newer_bytes: int, older_bytes: int, n_newer: int) -> int:
    """tkv_amq_merge_values_bound: the merged values' bytes at most."""
    return int(abi.lib().tkv_amq_merge_values_bound(int(newer_bytes), int(older_bytes), int(n_newer)))


def merge_leaves_device(newer: abi.MergeRun, older: abi.MergeRun, n_jobs: int, d_out_begin, d_items,
                        out_capacity: int, workspace, d_needed=None, flags: int = 0, d_counts=None,
                        stream=None) -> None:
    """The launches alone (tkv_amq_merge_leaves), capturable: the two runs (merge_run), d_out_begin:
    int64 [n_jobs + 1]; d_items: uint8 [16 * out_capacity] (abi.MERGE_ITEM_DTYPE records); workspace:
    uint8 [merge_leaves_workspace_bytes]; d_needed: int64 [1] or None; d_counts: int64 [7]
    (MergeCounts.counts) or None."""
    _require_device()
    st = abi.lib().tkv_amq_merge_leaves(
        ctypes.byref(newer), ctypes.byref(older), int(n_jobs), int(flags), _ptr(d_out_begin), _ptr(d_items),
        int(out_capacity), _ptr(d_needed), _ptr(d_counts), _ptr(workspace),
        0 if workspace is None else int(workspace.numel()), _stream_handle(stream))
    abi.check(st, "tkv_amq_merge_leaves")


def gather_merged_device(d_items, d_out_begin, n_jobs: int, out_capacity: int, newer: abi.MergeRun,
                         older: abi.MergeRun, d_out_keys, out_key_stride: int, d_out_key_offsets,
                         out_keys_capacity: int, d_out_values, d_out_value_offsets, out_values_capacity: int,
                         workspace, d_needed_bytes=None, stream=None) -> None:
    """The launches alone (tkv_amq_gather_merged), capturable behind merge_leaves_device: the records'
    keys (fixed slots of out_key_stride bytes, or with out_key_stride 0 bytes and d_out_key_offsets:
    int64 [out_capacity + 1]) and values (bytes and d_out_value_offsets); capacities in bytes;
    d_needed_bytes: int64 [2] or None."""
    _require_device()
    st = abi.lib().tkv_amq_gather_merged(
        _ptr(d_items), _ptr(d_out_begin), int(n_jobs), int(out_capacity), ctypes.byref(newer),
        ctypes.byref(older), _ptr(d_out_keys), int(out_key_stride), _ptr(d_out_key_offsets),
        int(out_keys_capacity), _ptr(d_out_values), _ptr(d_out_value_offsets), int(out_values_capacity),
        _ptr(d_needed_bytes), _ptr(workspace), 0 if workspace is None else int(workspace.numel()),
        _stream_handle(stream))
    abi.check(st, "tkv_amq_gather_merged")


@dataclass
class MergeResult:
    """What merge_leaves leaves on the device: the merged items' `keys` and packed `values` (KeyBatch
    each: the keys fixed when both inputs were fixed with one stride, else variable; the values
    variable), `out_begin` (int64 [n_jobs + 1]: job j's items are [out_begin[j], out_begin[j + 1]),
    the d_key_begin of a plan, a build or a lookup over them), `items` (uint8 [16 * n_out],
    abi.MERGE_ITEM_DTYPE records) and `counts`, this call's tkv_amq_merge_counts as a dict."""
    keys: KeyBatch
    values: KeyBatch
    out_begin: object
    items: object = field(default=None, repr=False)
    counts: dict = field(default_factory=dict)

    def records(self) -> np.ndarray:
        """The records on the host (a copy; synchronises)."""
        return self.items.cpu().numpy().view(abi.MERGE_ITEM_DTYPE)


def _begin_tensor(begin, dev, what: str):
    torch = _torch()
    t = (begin if hasattr(begin, "data_ptr") else torch.from_numpy(
        np.ascontiguousarray(np.asarray(begin, dtype=np.uint64)).view(np.int64)))
    t = t.to(device=dev, dtype=torch.int64).contiguous()
    if int(t.numel()) < 1:
        raise TkvAmqError(abi.INVALID_ARGUMENT, f"merge_leaves: {what} needs n_jobs + 1 entries")
    return t


def merge_leaves(newer: KeyBatch, newer_values: KeyBatch, newer_begin, older: KeyBatch, older_values: KeyBatch,
                 older_begin, *, decay: bool = False, stream=None) -> MergeResult:
    """The leaf update of a batch of leaves (tkv_amq_merge_leaves, then tkv_amq_gather_merged): job j
    merges the update's items [newer_begin[j], newer_begin[j + 1]) over the leaf's items
    [older_begin[j], older_begin[j + 1]) -- each run strictly ascending -- as the reference's
    merge_compact_edits does: the newer item of a key stands, an ADD_I32 is folded with the older
    item, and with decay=True tombstones and no-ops are dropped (a leaf keeps them).  The outputs are
    sized from the inputs (every item kept), so nothing is truncated; the record count and `counts`
    are read back, which synchronises."""
    torch = _torch()
    _require_device()
    dev = older.data.device
    d_nb = _begin_tensor(newer_begin, dev, "newer_begin")
    d_ob = _begin_tensor(older_begin, dev, "older_begin")
    if d_nb.numel() != d_ob.numel():
        raise TkvAmqError(abi.INVALID_ARGUMENT, "merge_leaves: the begin arrays differ in length")
    n_jobs = int(d_nb.numel()) - 1
    rn, ro = merge_run(newer, newer_values, d_nb), merge_run(older, older_values, d_ob)
    cap = newer.n + older.n
    ws_bytes = max(merge_leaves_workspace_bytes(n_jobs, newer.n, older.n), gather_merged_workspace_bytes(cap))
    if ws_bytes == 0:
        raise TkvAmqError(abi.INVALID_ARGUMENT, "merge_leaves: too many jobs or items")
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    out_begin = torch.empty(n_jobs + 1, dtype=torch.int64, device=dev)
    items = torch.empty(max(cap, 1) * 16, dtype=torch.uint8, device=dev)
    counts = MergeCounts(dev)
    merge_leaves_device(rn, ro, n_jobs, out_begin, items, cap, ws, None,
                        abi.MERGE_DECAY_TO_ITEMS if decay else 0, counts.counts, stream)
    fixed = newer.offsets is None and older.offsets is None and newer.stride == older.stride
    k_cap = cap * newer.stride if fixed else \
        (newer.n * newer.stride if newer.offsets is None else int(newer.data.numel())) + \
        (older.n * older.stride if older.offsets is None else int(older.data.numel()))
    v_cap = merge_values_bound(int(newer_values.data.numel()), int(older_values.data.numel()), newer.n)
    out_keys = torch.empty(max(k_cap, 1), dtype=torch.uint8, device=dev)
    out_vals = torch.empty(max(v_cap, 1), dtype=torch.uint8, device=dev)
    k_offs = None if fixed else torch.empty(cap + 1, dtype=torch.int64, device=dev)
    v_offs = torch.empty(cap + 1, dtype=torch.int64, device=dev)
    gather_merged_device(items, out_begin, n_jobs, cap, rn, ro, out_keys, newer.stride if fixed else 0, k_offs,
                         k_cap, out_vals, v_offs, v_cap, ws, None, stream)
    _hold(stream, d_nb, d_ob, ws, out_begin, items, out_keys, out_vals, k_offs, v_offs, counts.counts)
    (stream if stream is not None else torch.cuda.current_stream()).synchronize()
    n_out = int(out_begin[n_jobs].item())
    if fixed:
        keys = KeyBatch.fixed(out_keys[:n_out * newer.stride].view(n_out, newer.stride))
    else:
        keys = KeyBatch.variable(out_keys, k_offs[:n_out + 1])
    return MergeResult(keys, KeyBatch.variable(out_vals, v_offs[:n_out + 1]), out_begin, items[:16 * n_out],
                       counts.collect())


# ---------------------------------------------------------------------------------------
# node merge: a batch of K-way merges (the incoming batch over the update-buffer levels) on the device
# ---------------------------------------------------------------------------------------
def merge_levels_workspace_bytes(n_jobs: int, n_runs: int, n_items_total: int) -> int:
    """tkv_amq_merge_levels_ws_bytes (0: counts the call refuses)."""
    return int(abi.lib().tkv_amq_merge_levels_ws_bytes(int(n_jobs), int(n_runs), int(n_items_total)))


def gather_levels_workspace_bytes(out_capacity: int) -> int:
    """tkv_amq_gather_levels_ws_bytes."""
    return int(abi.lib().tkv_amq_gather_levels_ws_bytes(int(out_capacity)))


def merge_levels_values_bound(values_bytes_total: int, n_items_not_in_oldest_run: int) -> int:
    """tkv_amq_merge_levels_values_bound: the merged values' bytes at most."""
    return int(abi.lib().tkv_amq_merge_levels_values_bound(int(values_bytes_total), int(n_items_not_in_oldest_run)))


def _run_table(runs):
    """A list of abi.MergeRun (the newest first) as the contiguous host array the library takes."""
    return (abi.MergeRun * max(len(runs), 1))(*runs)


def merge_levels_device(runs, n_jobs: int, d_out_begin, d_items, out_capacity: int, workspace, d_needed=None,
                        flags: int = 0, d_counts=None, stream=None) -> None:
    """The launches alone (tkv_amq_merge_levels), capturable: `runs` a list of 1..8 merge_run structs,
    the newest first; the other arguments as merge_leaves_device has them, with a workspace of
    merge_levels_workspace_bytes.  A record's src holds its run in bits 56..63."""
    _require_device()
    st = abi.lib().tkv_amq_merge_levels(
        _run_table(runs), len(runs), int(n_jobs), int(flags), _ptr(d_out_begin), _ptr(d_items), int(out_capacity),
        _ptr(d_needed), _ptr(d_counts), _ptr(workspace), 0 if workspace is None else int(workspace.numel()),
        _stream_handle(stream))
    abi.check(st, "tkv_amq_merge_levels")


def gather_levels_device(d_items, d_out_begin, n_jobs: int, out_capacity: int, runs, d_out_keys,
                         out_key_stride: int, d_out_key_offsets, out_keys_capacity: int, d_out_values,
                         d_out_value_offsets, out_values_capacity: int, workspace, d_needed_bytes=None,
                         stream=None) -> None:
    """The launches alone (tkv_amq_gather_levels), capturable behind merge_levels_device: as
    gather_merged_device, over the merge's list of runs."""
    _require_device()
    st = abi.lib().tkv_amq_gather_levels(
        _ptr(d_items), _ptr(d_out_begin), int(n_jobs), int(out_capacity), _run_table(runs), len(runs),
        _ptr(d_out_keys), int(out_key_stride), _ptr(d_out_key_offsets), int(out_keys_capacity), _ptr(d_out_values),
        _ptr(d_out_value_offsets), int(out_values_capacity), _ptr(d_needed_bytes), _ptr(workspace),
        0 if workspace is None else int(workspace.numel()), _stream_handle(stream))
    abi.check(st, "tkv_amq_gather_levels")


def merge_levels(runs, *, decay: bool = False, stream=None) -> MergeResult:
    """The merge of K levels for a batch of key ranges (tkv_amq_merge_levels, then tkv_amq_gather_levels):
    `runs` is a list of 1..8 (keys: KeyBatch, values: KeyBatch, begin) triples, the newest level first;
    job j merges items [begin[j], begin[j + 1]) of every run -- each strictly ascending -- as the
    reference's merge_compact_edits does over the levels InMemoryNode::push_levels_to_merge pushes: the
    newest item of a key stands, an ADD_I32 is folded through the older items of its key, and with
    decay=True tombstones and no-ops are dropped.  The counterpart of merge_leaves: the outputs are sized
    from the inputs, and the record count and `counts` are read back, which synchronises."""
    torch = _torch()
    _require_device()
    if not 1 <= len(runs) <= abi.MERGE_MAX_RUNS:
        raise TkvAmqError(abi.INVALID_ARGUMENT, "merge_levels: 1 to 8 runs")
    dev = runs[-1][0].data.device
    begins = [_begin_tensor(b, dev, f"begin of run {r}") for r, (_, _, b) in enumerate(runs)]
    if any(b.numel() != begins[0].numel() for b in begins):
        raise TkvAmqError(abi.INVALID_ARGUMENT, "merge_levels: the begin arrays differ in length")
    n_jobs = int(begins[0].numel()) - 1
    table = [merge_run(k, v, b) for (k, v, _), b in zip(runs, begins)]
    keys, values = [k for k, _, _ in runs], [v for _, v, _ in runs]
    cap = sum(k.n for k in keys)
    ws_bytes = max(merge_levels_workspace_bytes(n_jobs, len(runs), cap), gather_levels_workspace_bytes(cap))
    if merge_levels_workspace_bytes(n_jobs, len(runs), cap) == 0:
        raise TkvAmqError(abi.INVALID_ARGUMENT, "merge_levels: too many jobs or items")
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    out_begin = torch.empty(n_jobs + 1, dtype=torch.int64, device=dev)
    items = torch.empty(max(cap, 1) * 16, dtype=torch.uint8, device=dev)
    counts = MergeCounts(dev)
    merge_levels_device(table, n_jobs, out_begin, items, cap, ws, None, abi.MERGE_DECAY_TO_ITEMS if decay else 0,
                        counts.counts, stream)
    stride = keys[0].stride
    fixed = all(k.offsets is None and k.stride == stride for k in keys)
    k_cap = cap * stride if fixed else sum(k.n * k.stride if k.offsets is None else int(k.data.numel()) for k in keys)
    v_cap = merge_levels_values_bound(sum(int(v.data.numel()) for v in values), cap - keys[-1].n)
    out_keys = torch.empty(max(k_cap, 1), dtype=torch.uint8, device=dev)
    out_vals = torch.empty(max(v_cap, 1), dtype=torch.uint8, device=dev)
    k_offs = None if fixed else torch.empty(cap + 1, dtype=torch.int64, device=dev)
    v_offs = torch.empty(cap + 1, dtype=torch.int64, device=dev)
    gather_levels_device(items, out_begin, n_jobs, cap, table, out_keys, stride if fixed else 0, k_offs, k_cap,
                         out_vals, v_offs, v_cap, ws, None, stream)
    _hold(stream, *begins, ws, out_begin, items, out_keys, out_vals, k_offs, v_offs, counts.counts)
    (stream if stream is not None else torch.cuda.current_stream()).synchronize()
    n_out = int(out_begin[n_jobs].item())
    if fixed:
        out = KeyBatch.fixed(out_keys[:n_out * stride].view(n_out, stride))
    else:
        out = KeyBatch.variable(out_keys, k_offs[:n_out + 1])
    return MergeResult(out, KeyBatch.variable(out_vals, v_offs[:n_out + 1]), out_begin, items[:16 * n_out],
                       counts.collect())


# ---------------------------------------------------------------------------------------
# single-leaf API (the reference's per-leaf entry points)
# ---------------------------------------------------------------------------------------
@dataclass
class FilterPage:
    """A built filter page payload on the device plus its one-segment plan."""
    kind: int
    payload: object          # device uint8 tensor (page payload bytes)
    plan: FilterPlan
    leaf_page_id: int
    load_status: int = 0     # abi.OPEN_* of from_payload (0: a planned page, or opened fine)

    @classmethod
    def from_payload(cls, kind: int, payload) -> "FilterPage":
        """A filter page from its bare payload bytes (device uint8 tensor, or host bytes that are
        uploaded), with no plan: the one-segment plan comes from the payload itself
        (open_filters), as reject_page reads a loaded page (tree/key_query.hpp:149-247).  A
        payload that does not open keeps its code in load_status: reject_page then answers
        kUnknown for every key and counts filter_page_load_failed_count."""
        torch = _torch()
        if not hasattr(payload, "data_ptr"):
            host = np.frombuffer(bytes(payload), dtype=np.uint8) if not isinstance(payload, np.ndarray) \
                else np.ascontiguousarray(payload, dtype=np.uint8)
            payload = torch.from_numpy(host.copy() if len(host) else np.zeros(1, np.uint8)).cuda()[:len(host)]
        if not payload.is_contiguous() or payload.data_ptr() % 16:
            payload = payload.clone()
        opened = open_filters(kind, payload, offsets=[0])
        return cls(kind, payload, opened.plan, int(opened.plan.segs[0]["src_page_id"]),
                   int(opened.status[0]))

    @property
    def filter_size(self) -> int:
        return int(self.plan.segs[0]["payload_bytes"])

    def unused_begin(self) -> int:
        """filter_page_header->unused_begin (filter_builder.hpp:293-294)."""
        return PACKED_PAGE_HEADER_BYTES + self.filter_size


def _build_one(kind: int, bpk: int, leaf_page_id: int, keys: KeyBatch,
               page_payload_bytes: int) -> FilterPage | None:
    if bpk == 0:
        return None  # filter_builder.hpp:115-117 / :227-229
    plan = plan_filters(kind, [keys.n], bpk, payload_capacity=page_payload_bytes,
                        src_page_ids=[leaf_page_id])
    out = build_all_filters(plan, keys)
    return FilterPage(kind, out, plan, leaf_page_id)


def build_bloom_filter_for_leaf(filter_bits_per_key: int, leaf_page_id: int, keys: KeyBatch,
                                page_payload_bytes: int = 0) -> FilterPage | None:
    return _build_one(BLOOM, filter_bits_per_key, leaf_page_id, keys, page_payload_bytes)


def build_quotient_filter_for_leaf(filter_bits_per_key: int, leaf_page_id: int, keys: KeyBatch,
                                   page_payload_bytes: int) -> FilterPage | None:
    return _build_one(VQF, filter_bits_per_key, leaf_page_id, keys, page_payload_bytes)


def build_filter_for_leaf_in_job(filter_bits_per_key: int, leaf_page_id: int, keys: KeyBatch,
                                 page_payload_bytes: int | None = None,
                                 kind: int = DEFAULT_FILTER_KIND) -> FilterPage | None:
    """Like the reference: a failed build is logged and the leaf gets no filter
    (filter_builder.hpp:323-325).  The payload capacity defaults to the filter page of the
    default TreeOptions for this bits/key (TreeOptions.filter_page_payload_size)."""
    if page_payload_bytes is None:
        page_payload_bytes = (TreeOptions(kind).set_filter_bits_per_key(filter_bits_per_key)
                              .filter_page_payload_size())
    try:
        if kind == BLOOM:
            return build_bloom_filter_for_leaf(filter_bits_per_key, leaf_page_id, keys,
                                               page_payload_bytes)
        return build_quotient_filter_for_leaf(filter_bits_per_key, leaf_page_id, keys,
                                              page_payload_bytes)
    except TkvAmqError as e:
        if e.status == abi.UNAVAILABLE:
            raise
        log.warning("Failed to build filter: %s", e)
        return None


class PackedVqfFilter:
    """View of a VQF filter page payload in device memory (vqf_filter_page_view.hpp:63-126)."""

    def __init__(self, page: FilterPage):
        if page.kind != VQF:
            raise TkvAmqError(abi.INVALID_ARGUMENT, "not a VQF filter page")
        self.page = page
        hdr = page.payload[:80].cpu().numpy().view("<u8")
        self.magic, self.src_page_id, self.hash_seed, self.hash_mask = (int(x) for x in hdr[:4])
        self.key_remainder_bits = int(hdr[5])

    def check_magic(self) -> None:
        if self.magic != VQF_MAGIC:
            raise TkvAmqError(abi.INTERNAL, "PackedVqfFilter magic mismatch")

    def is_present(self, hash_vals):
        """Batched is_present(hash_val): uint8 tensor, 1 = maybe present."""
        torch = _torch()
        hv = hash_vals if hasattr(hash_vals, "data_ptr") else torch.tensor(
            np.asarray(hash_vals, dtype=np.uint64).view(np.int64), device=self.page.payload.device)
        qs = torch.zeros(hv.numel(), dtype=torch.int32, device=hv.device)
        return vqf_probe_hashed(self.page.plan, self.page.payload, hv, qs)


class _Count:
    """FastCountMetric<u64>."""

    def __init__(self):
        self._lock = threading.Lock()
        self.value = 0

    def add(self, n: int) -> None:
        with self._lock:
            self.value += int(n)

    def get(self) -> int:
        return self.value

    def __repr__(self):
        return str(self.value)


class KeyQueryMetrics:
    """KeyQuery::Metrics, the filter counters (tree/key_query.hpp:36-60).  reject_page updates
    total / no-filter / load-failed / page-id-mismatch / reject (:154,157,183,210,231,243);
    the caller's leaf search updates positive / false positive (key_query.cpp:41,77): the
    batched device probes count those when given a ProbeMetrics (and ground truth)."""

    def __init__(self):
        self.total_filter_query_count = _Count()
        self.no_filter_page_count = _Count()
        self.filter_page_load_failed_count = _Count()
        self.page_id_mismatch_count = _Count()
        self.filter_reject_count = _Count()
        self.filter_positive_count = _Count()
        self.filter_false_positive_count = _Count()

    def filter_false_positive_rate(self) -> float:
        positives = self.filter_positive_count.get()
        if positives == 0:
            return -1.0
        return self.filter_false_positive_count.get() / positives

    def as_dict(self) -> dict:
        return {k: v.get() for k, v in vars(self).items() if isinstance(v, _Count)}


class KeyQuery:
    """KeyQuery (tree/key_query.hpp:33-253) for a batch of point-query keys.  The hashes are
    computed once per query and reused for every filter probed: the VQF hash_val
    (key_query.hpp:82) and the Bloom BloomFilterQuery cache (:78,97)."""

    BLOOM_K_MAX = 32
    _metrics = KeyQueryMetrics()

    @classmethod
    def metrics(cls) -> KeyQueryMetrics:
        """The process-wide counters (KeyQuery::metrics(), :64-68)."""
        return cls._metrics

    def __init__(self, keys: KeyBatch):
        self.keys = keys
        self.hash_val = vqf_hash_val(keys)
        self.bloom_query = bloom_query_hashes(keys, self.BLOOM_K_MAX)

    def reject_page(self, page_id_to_reject: int, filter_page: FilterPage | None,
                    truth=None) -> list:
        """Per key: kTrue = filter says definitely absent; kFalse = maybe present;
        kUnknown = no filter page, or it belongs to another leaf (key_query.hpp:156-159,207-232).
        `truth` (optional, 1 = key is in the leaf): counts the positives that are false, as the
        caller's leaf search does (key_query.cpp:41,77)."""
        torch = _torch()
        m = self.metrics()
        n = self.keys.n
        m.total_filter_query_count.add(n)
        if filter_page is None:
            m.no_filter_page_count.add(n)
            return [BoolStatus.kUnknown] * n
        if filter_page.load_status != abi.OPEN_OK:  # the page could not be loaded (:183)
            m.filter_page_load_failed_count.add(n)
            return [BoolStatus.kUnknown] * n
        hdr = filter_page.payload[:32].cpu().numpy().view("<u8")
        magic = int(hdr[0])
        want = VQF_MAGIC if filter_page.kind == VQF else BLOOM_MAGIC
        if magic != want:  # check_magic (:194, vqf_filter_page_view.hpp:97-100)
            raise TkvAmqError(abi.INTERNAL, "filter page magic mismatch")
        src = int(hdr[2]) if filter_page.kind == BLOOM else int(hdr[1])
        if src != page_id_to_reject:
            m.page_id_mismatch_count.add(n)
            return [BoolStatus.kUnknown] * n
        dev = filter_page.payload.device
        qs = torch.zeros(n, dtype=torch.int32, device=dev)
        pm = ProbeMetrics(dev)
        tr = None if truth is None else torch.as_tensor(np.asarray(truth, dtype=np.uint8), device=dev)
        if filter_page.kind == VQF:
            present = vqf_probe_hashed(filter_page.plan, filter_page.payload, self.hash_val, qs,
                                       truth=tr, metrics=pm)
        else:
            present = bloom_probe_hashed(filter_page.plan, filter_page.payload, self.bloom_query,
                                         self.BLOOM_K_MAX, qs, truth=tr, metrics=pm)
        c = pm.collect()
        m.filter_reject_count.add(c["filter_reject_count"])
        m.filter_positive_count.add(c["filter_positive_count"])
        if truth is not None:
            m.filter_false_positive_count.add(c["filter_false_positive_count"])
        return [BoolStatus.kFalse if p else BoolStatus.kTrue for p in present.cpu().tolist()]


# ---------------------------------------------------------------------------------------
# host-resident keys -> host filter pages (keys come from host
# checkpoint buffers and the filters return to host page memory)
# ---------------------------------------------------------------------------------------
class HostFilterPipeline:
    """Host-resident keys -> host filter pages for one batch shape (a checkpoint's leaves).

    Chunks of whole leaves flow H2D -> build -> D2H on three streams (copy-in, build,
    copy-out), double-buffered, so PCIe transfers in both directions overlap the kernels.
    Plans, device buffers and per-chunk plan uploads are prepared once in the constructor;
    run() only enqueues copies and builds.  Output: the batch's filter pages at a fixed
    per-leaf stride (leaf s at byte s * out_stride)."""

    def __init__(self, kind: int, leaf_key_counts, bits_per_key: int, payload_capacity: int = 0,
                 out_stride: int = 0, chunk_keys: int = 8 << 20, src_page_ids=None,
                 key_bytes: int = 16, device=None):
        torch = _torch()
        _require_device()
        self.kind, self.dev = kind, torch.device(device or "cuda")
        self.key_bytes = key_bytes
        counts = np.asarray(leaf_key_counts, dtype=np.int64)
        if out_stride == 0:
            biggest = int(counts.max()) if len(counts) else 0
            p1 = plan_filters(kind, [biggest], bits_per_key, payload_capacity=payload_capacity)
            out_stride = (int(p1.segs[0]["payload_bytes"]) + 63) // 64 * 64 or 64
        self.out_stride = out_stride
        self.plan = plan_filters(kind, counts, bits_per_key, payload_capacity=payload_capacity,
                                 out_stride=out_stride, src_page_ids=src_page_ids)
        bounds, acc = [0], 0
        for i, c in enumerate(counts):
            acc += int(c)
            if acc >= chunk_keys:
                bounds.append(i + 1)
                acc = 0
        if bounds[-1] != len(counts):
            bounds.append(len(counts))
        self.key_begin = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        self.chunks = list(zip(bounds, bounds[1:]))
        self.plans = [plan_filters(kind, counts[b0:b1], bits_per_key,
                                   payload_capacity=payload_capacity, out_stride=out_stride,
                                   src_page_ids=self.plan.segs["src_page_id"][b0:b1])
                      for b0, b1 in self.chunks]
        max_keys = max((int(self.key_begin[b1] - self.key_begin[b0]) for b0, b1 in self.chunks), default=1)
        max_leaves = max((b1 - b0 for b0, b1 in self.chunks), default=1)
        ws_bytes = max((p.workspace_bytes for p in self.plans), default=0)
        self.d_keys = [torch.empty((max(max_keys, 1), key_bytes), dtype=torch.uint8, device=self.dev)
                       for _ in range(2)]
        self.d_out = [torch.empty(max(max_leaves * out_stride, 1), dtype=torch.uint8, device=self.dev)
                      for _ in range(2)]
        self.d_ws = [torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=self.dev) for _ in range(2)]
        for p in self.plans:
            p.device_segs(self.dev)
        self.s_in, self.s_run, self.s_out = (torch.cuda.Stream(self.dev) for _ in range(3))
        # failed leaves by cause: [0] inserts that overflowed a block (TKV_AMQ_VQF_FLAG_OVERFLOW,
        # bit 31), [1] a workspace smaller than the plan (TKV_AMQ_VQF_FLAG_WORKSPACE, bit 30)
        self.fail = torch.zeros(2, dtype=torch.int32, device=self.dev)
        torch.cuda.synchronize(self.dev)

    def new_host_output(self):
        return _torch().empty(self.plan.total_out_bytes, dtype=_torch().uint8, pin_memory=True)

    def _fold_flags(self, slot: int, chunk) -> None:
        """Add the chunk's failed-leaf counts (the flag bits of each leaf's nelts word in the VQF
        workspace, tkv_amq_build_check's source) to self.fail, on the device: bit 31 (an insert
        overflowed its block) and bit 30 (the workspace was short) counted apart, so each is
        reported as tkv_amq_build_check reports it."""
        torch = _torch()
        b0, b1 = chunk
        w = self.d_ws[slot][64:64 + 4 * (b1 - b0)].view(torch.int32)
        self.fail[0].add_((w < 0).sum(dtype=torch.int32))                  # bit 31
        self.fail[1].add_((((w >> 30) & 1) != 0).sum(dtype=torch.int32))  # bit 30

    def run_views(self, views, host_out=None, view_stride: int = 16, n_threads: int = 16,
                  check: bool = True):
        """Keys given as tkv_amq_key_view records (the EditView key range; KEY_VIEW_DTYPE
        array or the address of the first view).  Each chunk's keys are gathered into a
        pinned staging buffer by host threads just before its H2D copy is enqueued, so the
        gather of chunk c+1 overlaps the copies and build of chunk c.  The threads are a
        persistent pool, each running tkv_amq_stage_keys on a slice (ctypes releases the GIL),
        so no threads are created per chunk."""
        import concurrent.futures
        torch = _torch()
        if isinstance(views, np.ndarray):
            assert views.dtype == abi.KEY_VIEW_DTYPE and views.flags.c_contiguous
            addr, view_stride = views.ctypes.data, abi.KEY_VIEW_DTYPE.itemsize
        else:
            addr = int(views)
        n_keys = int(self.key_begin[-1])
        if getattr(self, "_h_stage", None) is None or self._h_stage.shape[0] < n_keys:
            self._h_stage = torch.empty((max(n_keys, 1), self.key_bytes), dtype=torch.uint8,
                                        pin_memory=True)
        h = self._h_stage
        if getattr(self, "_pool", None) is None or self._pool_threads != n_threads:
            self._pool = concurrent.futures.ThreadPoolExecutor(max(1, n_threads))
            self._pool_threads = n_threads

        def one(a, b):
            stage_keys(addr + a * view_stride, b - a, self.key_bytes, out=h[a:b],
                       view_stride=view_stride, n_threads=1)

        def stage(k0, k1):
            if k1 <= k0:
                return
            parts = max(1, min(n_threads, (k1 - k0) // 16384))
            cuts = [k0 + (k1 - k0) * i // parts for i in range(parts + 1)]
            for f in [self._pool.submit(one, a, b) for a, b in zip(cuts, cuts[1:])]:
                f.result()

        return self.run(h, host_out, check, stage=stage)

    def run(self, host_keys, host_out=None, check: bool = True, stage=None):
        """`stage(k0, k1)`, if given, fills host_keys[k0:k1] before that chunk's H2D copy is
        enqueued (run_views)."""
        torch = _torch()
        t_run = time.perf_counter()
        if host_out is None:
            host_out = self.new_host_output()
        n = len(self.chunks)
        ev_in = [torch.cuda.Event() for _ in range(n)]
        ev_run = [torch.cuda.Event() for _ in range(n)]
        ev_out = [torch.cuda.Event() for _ in range(n)]
        st = self.out_stride
        self.s_run.wait_stream(torch.cuda.current_stream(self.dev))
        with torch.cuda.stream(self.s_run):
            self.fail.zero_()
        for c, (b0, b1) in enumerate(self.chunks):
            slot = c & 1
            k0, k1 = int(self.key_begin[b0]), int(self.key_begin[b1])
            if stage is not None:
                stage(k0, k1)
            with torch.cuda.stream(self.s_in):
                if c >= 2:
                    self.s_in.wait_event(ev_run[c - 2])       # slot's keys no longer read
                self.d_keys[slot][:k1 - k0].copy_(host_keys[k0:k1], non_blocking=True)
                ev_in[c].record(self.s_in)
            with torch.cuda.stream(self.s_run):
                self.s_run.wait_event(ev_in[c])
                if c >= 2:
                    self.s_run.wait_event(ev_out[c - 2])      # slot's output copied out
                    if self.kind == VQF:                      # fold chunk c-2's failure flags
                        self._fold_flags(slot, self.chunks[c - 2])
                build_all_filters(self.plans[c], KeyBatch.fixed(self.d_keys[slot][:k1 - k0]),
                                  out=self.d_out[slot], workspace=self.d_ws[slot],
                                  stream=self.s_run, check=False)
                ev_run[c].record(self.s_run)
            with torch.cuda.stream(self.s_out):
                self.s_out.wait_event(ev_run[c])
                nbytes = (b1 - b0) * st
                host_out[b0 * st:b0 * st + nbytes].copy_(self.d_out[slot][:nbytes], non_blocking=True)
                ev_out[c].record(self.s_out)
        if self.kind == VQF:
            with torch.cuda.stream(self.s_run):
                for c in range(max(0, n - 2), n):
                    self._fold_flags(c & 1, self.chunks[c])
        self.s_out.synchronize()
        if check and self.kind == VQF:
            self.s_run.synchronize()
            overflow, short_ws = (int(x) for x in self.fail.tolist())
            if short_ws:  # as tkv_amq_build_check: the plan's workspace was not given
                raise TkvAmqError(abi.INVALID_ARGUMENT, f"vqf build: workspace smaller than the plan "
                                                        f"({short_ws} leaves)")
            if overflow:
                raise TkvAmqError(abi.INTERNAL, "vqf_insert (filter_builder.hpp:211)")
        if check or self.kind == BLOOM:
            record_filter_metrics(self.plan, (time.perf_counter() - t_run) * 1e6)
        return host_out


def build_filters_from_host(kind: int, leaf_key_counts, bits_per_key: int, host_keys,
                            payload_capacity: int = 0, out_stride: int = 0, host_out=None,
                            chunk_keys: int = 8 << 20, src_page_ids=None, device=None):
    """One-shot HostFilterPipeline: returns (host_out, plan of the whole batch)."""
    torch = _torch()
    if not isinstance(host_keys, torch.Tensor):
        host_keys = torch.from_numpy(np.ascontiguousarray(host_keys))
    pipe = HostFilterPipeline(kind, leaf_key_counts, bits_per_key, payload_capacity, out_stride,
                              chunk_keys, src_page_ids, host_keys.shape[1], device)
    return pipe.run(host_keys, host_out), pipe.plan
