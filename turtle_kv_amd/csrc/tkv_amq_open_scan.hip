// tkv_amq_open_scan.hip -- open built filter pages without a plan, and scan their fill.
//
//   open_filters_kernel  one lane per filter: bounds-checks and reads the payload header (and
//                        the page header of a page image), validates it against the tkv-amq v1
//                        spec and writes the segment the probes address
//                        with -- what KeyQuery::reject_page reads from a loaded filter page
//                        (tree/key_query.hpp:149-247, vqf_filter_page_view.hpp:96-100).
//   scan_init / prefix_inclusive_u64 (tkv_amq_scan.h) / scan_blocks / scan_fold
//                        a read-only pass over every filter's blocks: the
//                        blocks are cut into chunks of kScanChunkBlocks, a device-side prefix
//                        over the segments' chunk counts lives in the workspace, and every
//                        workgroup takes a contiguous run of chunks whatever leaf they belong
//                        to.  Four neighbouring lanes read one 64-byte block with a 16-byte load
//                        each, so a wave's load covers 1 KiB of whole lines; counts are kept in
//                        registers while the segment stays the same, reduced over the wave with
//                        shuffles, over the workgroup through 80 bytes of LDS, and added to the
//                        segment's stats with integer atomics -- but for the segment still open
//                        at the end of a workgroup's run, whose counts go to a slot that
//                        scan_fold combines, so one filter spread over the whole grid does not
//                        queue thousands of atomics on one word.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "tkv_amq.h"
#include "tkv_amq_device.h"
#include "tkv_amq_scan.h"

namespace tkv {
namespace {

constexpr uint64_t kLayoutVqfId = 0x746c69665f667176ull;    // "vqf_filt"
constexpr uint64_t kLayoutBloomId = 0x746c666d6f6f6c62ull;  // "bloomflt"
constexpr uint64_t kVqfBlocksMax = 1ull << 24;              // kVqfMaxBlocks of the builds

constexpr uint32_t kScanThreads = 256;
constexpr uint32_t kScanRows = 4;                                // 16-byte loads per lane per chunk
constexpr uint32_t kScanChunkBlocks = kScanRows * kScanThreads / 4;  // 256 blocks = 16 KiB
constexpr uint32_t kScanMaxGrid = 4096;  // scan_blocks' workgroups at most: one 32-byte slot each
constexpr uint32_t kFoldThreads = 256;
constexpr uint64_t kScanWsHeader = 16;

__host__ __device__ inline uint32_t vqf_slots_of(uint32_t t) { return t == 8 ? 48u : 28u; }
__host__ __device__ inline uint32_t vqf_buckets_of(uint32_t t) { return t == 8 ? 80u : 36u; }

struct OpenArgs {
  int kind;
  const uint8_t* filters;
  uint64_t total_bytes;
  const uint64_t* offsets;
  uint64_t stride;
  uint32_t page_log2;
  uint32_t n;
  tkv_amq_segment* segs;
  uint32_t* status;
  uint32_t* summary;
};

__device__ inline ulonglong2 ld128(const uint8_t* p)
{
  return *reinterpret_cast<const ulonglong2*>(p);
}

// Validates the payload at [begin, bound) and fills `g` (zeroed by the caller).  Every read is
// preceded by the check that it lies below `bound`.
__device__ inline uint32_t open_payload(int kind, const uint8_t* filters, uint64_t begin, uint64_t bound,
                                        tkv_amq_segment& g)
{
  if (begin > bound) return TKV_AMQ_OPEN_OUT_OF_BOUNDS;
  if (begin & 15) return TKV_AMQ_OPEN_MISALIGNED;
  const uint64_t room = bound - begin;
  // the magic is the first word of either header; the smaller header (Bloom's 64 bytes, the
  // VQF's 80) must fit before anything is read
  const uint64_t hdr = kind == TKV_AMQ_BLOOM ? kBloomHeader : kVqfHeader + kVqfMetadata;
  if (room < hdr) return TKV_AMQ_OPEN_OUT_OF_BOUNDS;
  const uint8_t* p = filters + begin;
  const ulonglong2 w0 = ld128(p);
  const uint64_t magic = w0.x;
  const uint64_t mine = kind == TKV_AMQ_BLOOM ? kBloomMagic : kVqfMagic;
  const uint64_t other = kind == TKV_AMQ_BLOOM ? kVqfMagic : kBloomMagic;
  if (magic == other) return TKV_AMQ_OPEN_WRONG_KIND;
  if (magic != mine) return TKV_AMQ_OPEN_BAD_MAGIC;
  if (kind == TKV_AMQ_BLOOM) {
    // 0 magic | 8 bit_count | 16 src_page_id | 24 xxh3_checksum | 32 word_count |
    // 40 block_count u32 | 44 hash_count u16 | 46 layout u8 | 48 item_count
    const ulonglong2 w1 = ld128(p + 16), w2 = ld128(p + 32), w3 = ld128(p + 48);
    const uint64_t bit_count = w0.y, word_count = w2.x;
    const uint32_t block_count = (uint32_t)w2.y;
    const uint32_t hash_count = (uint32_t)(w2.y >> 32) & 0xffffu;
    const uint32_t layout = (uint32_t)(w2.y >> 48) & 0xffu;
    if (layout != 2 || hash_count < 1 || hash_count > kMaxBloomHashes || block_count < 1)
      return TKV_AMQ_OPEN_BAD_GEOMETRY;
    const uint64_t bytes = kBloomHeader + 64ull * block_count;
    if (bytes > room || bytes > 0xffffffffull) return TKV_AMQ_OPEN_OUT_OF_BOUNDS;
    if (bit_count != 512ull * block_count || word_count != 8ull * block_count)
      return TKV_AMQ_OPEN_BAD_GEOMETRY;
    g.n_blocks = block_count;
    g.hash_count = (uint16_t)hash_count;
    g.src_page_id = w1.x;
    g.n_keys = w3.x > 0xffffffffull ? 0xffffffffu : (uint32_t)w3.x;
    g.payload_bytes = (uint32_t)bytes;
    return TKV_AMQ_OPEN_OK;
  }
  // PackedVqfFilter: 0 magic | 8 src_page_id | 16 hash_seed | 24 hash_mask | vqf_metadata @32:
  // total_size_in_bytes, key_remainder_bits, range, nblocks, nelts, nslots
  const ulonglong2 w1 = ld128(p + 16), w2 = ld128(p + 32), w3 = ld128(p + 48), w4 = ld128(p + 64);
  const uint64_t seed = w1.x, mask = w1.y, total_size = w2.x, t = w2.y, range = w3.x, nblocks = w3.y,
                 nelts = w4.x, nslots = w4.y;
  if (seed != kVqfHashSeed || mask == 0) return TKV_AMQ_OPEN_BAD_GEOMETRY;
  const uint32_t shift = (uint32_t)__ffsll((unsigned long long)mask) - 1u;
  if (mask != (~0ull << shift)) return TKV_AMQ_OPEN_BAD_GEOMETRY;
  if ((t != 8 && t != 16) || nblocks < 1 || nblocks > kVqfBlocksMax) return TKV_AMQ_OPEN_BAD_GEOMETRY;
  const uint64_t bytes = kVqfHeader + kVqfMetadata + 64ull * nblocks;
  if (bytes > room || bytes > 0xffffffffull) return TKV_AMQ_OPEN_OUT_OF_BOUNDS;
  const uint64_t buckets = vqf_buckets_of((uint32_t)t), slots = vqf_slots_of((uint32_t)t);
  if (total_size != 64ull * nblocks || range != (nblocks * buckets) << t || nslots != nblocks * slots ||
      nelts > nslots)
    return TKV_AMQ_OPEN_BAD_GEOMETRY;
  g.n_blocks = (uint32_t)nblocks;
  g.tag_bits = (uint8_t)t;
  g.hash_val_shift = (uint8_t)shift;
  g.mod_magic = ~0ull / (nblocks * buckets);
  g.src_page_id = w0.y;
  g.n_keys = nelts > 0xffffffffull ? 0xffffffffu : (uint32_t)nelts;
  g.payload_bytes = (uint32_t)bytes;
  return TKV_AMQ_OPEN_OK;
}

__global__ __launch_bounds__(256) void open_filters_kernel(OpenArgs a)
{
  const uint32_t s = blockIdx.x * 256 + threadIdx.x;
  uint32_t st = 0xffffffffu;  // (a lane past the last filter)
  if (s < a.n) {
    tkv_amq_segment g = {};
    uint64_t begin, bound;
    bool page_ok = true;
    if (a.page_log2) {
      const uint64_t size = 1ull << a.page_log2;
      const uint64_t page = (uint64_t)s << a.page_log2;
      begin = page + kPackedPageHeaderBytes;
      // (begin > bound below when the page header itself does not fit)
      bound = page + size < a.total_bytes ? page + size : a.total_bytes;
    } else if (a.offsets) {
      begin = a.offsets[s];
      bound = a.total_bytes;
    } else {
      const uint64_t hi = __umul64hi((uint64_t)s, a.stride);
      begin = hi ? ~0ull : (uint64_t)s * a.stride;
      const uint64_t end = begin + a.stride;
      bound = (hi || end < begin || end > a.total_bytes) ? a.total_bytes : end;
    }
    st = open_payload(a.kind, a.filters, begin, bound, g);
    if (st == TKV_AMQ_OPEN_OK && a.page_log2) {
      // the PackedPageHeader fields the builders set: layout_id @16,
      // unused_begin @28, unused_end @32, size @60
      const uint8_t* page = a.filters + (begin - kPackedPageHeaderBytes);
      const uint4 h1 = *reinterpret_cast<const uint4*>(page + 16);
      const uint4 h2 = *reinterpret_cast<const uint4*>(page + 32);
      const uint4 h3 = *reinterpret_cast<const uint4*>(page + 48);
      const uint64_t layout = (uint64_t)h1.x | ((uint64_t)h1.y << 32);
      const uint32_t size = 1u << a.page_log2;
      page_ok = layout == (a.kind == TKV_AMQ_BLOOM ? kLayoutBloomId : kLayoutVqfId) &&
                h1.w == (uint32_t)kPackedPageHeaderBytes + g.payload_bytes && h2.x == size && h3.w == size;
      if (!page_ok) st = TKV_AMQ_OPEN_BAD_PAGE;
      g.page_flags = TKV_AMQ_PAGE_IMAGE | (a.page_log2 << 8);
    }
    if (st != TKV_AMQ_OPEN_OK) g = tkv_amq_segment{};  // the "no filter" segment
    g.out_offset = begin;
    ulonglong2* dst = reinterpret_cast<ulonglong2*>(a.segs + s);
    const ulonglong2* src = reinterpret_cast<const ulonglong2*>(&g);
#pragma unroll
    for (int i = 0; i < 4; ++i) dst[i] = src[i];
    a.status[s] = st;
  }
  if (a.summary) {
    // one atomic per code per wave
#pragma unroll
    for (uint32_t c = 0; c < 7; ++c) {
      const uint64_t m = bal(st == c);
      if (m != 0 && __lane_id() == 0) atomicAdd(a.summary + c, (uint32_t)__popcll(m));
    }
  }
}

// ---------------------------------------------------------------------------------------
// scan
// ---------------------------------------------------------------------------------------
struct ScanSeg {
  uint64_t out_offset;
  uint32_t n_blocks, tag_bits;  // n_blocks 0: nothing to scan
};

__device__ inline ScanSeg load_scan_seg(int kind, const tkv_amq_segment* segs, uint32_t s)
{
  const ulonglong2 v = *reinterpret_cast<const ulonglong2*>(segs + s);
  ScanSeg r;
  r.out_offset = v.x;
  r.n_blocks = (uint32_t)v.y;
  const uint32_t hash_count = (uint32_t)(v.y >> 32) & 0xffffu;
  r.tag_bits = (uint32_t)(v.y >> 48) & 0xffu;
  const bool has = kind == TKV_AMQ_BLOOM ? hash_count != 0 : (r.tag_bits == 8 || r.tag_bits == 16);
  if (!has) r.n_blocks = 0;
  return r;
}

// zeroes the stats, stores header_items and the segment's chunk count (pre[s + 1])
__global__ __launch_bounds__(256) void scan_init(int kind, const uint8_t* __restrict__ filters,
                                                 const tkv_amq_segment* __restrict__ segs, uint32_t n_segs,
                                                 tkv_amq_filter_stats* __restrict__ stats,
                                                 uint64_t* __restrict__ pre)
{
  const uint32_t s = blockIdx.x * 256 + threadIdx.x;
  if (s == 0) pre[0] = 0;
  if (s >= n_segs) return;
  const ScanSeg g = load_scan_seg(kind, segs, s);
  uint64_t items = 0;
  if (g.n_blocks) {
    const uint8_t* p = filters + g.out_offset;
    items = *reinterpret_cast<const uint64_t*>(p + (kind == TKV_AMQ_BLOOM ? 48 : kVqfHeader + 32));
  }
  ulonglong2* d = reinterpret_cast<ulonglong2*>(stats + s);
  d[0] = ulonglong2{0, items};
  d[1] = ulonglong2{0, 0};
  pre[s + 1] = ((uint64_t)g.n_blocks + kScanChunkBlocks - 1) / kScanChunkBlocks;
}

struct ScanAcc {
  uint32_t occ = 0, full = 0, empty = 0, maxb = 0, bad = 0;
};

// Adds the workgroup's counts to one segment's stats: reduced over each wave with shuffles, over
// the workgroup's waves through LDS, then one atomic per non-zero counter.  max_block takes its
// atomic only while it would still raise the stored value (the value only grows, so a stale read
// can cost a needless atomic but never lose a maximum): one filter spread over the whole grid
// would otherwise queue two same-address atomics per workgroup.
__device__ inline void scan_flush(ScanAcc& a, tkv_amq_filter_stats* st, uint32_t (*s_part)[5])
{
  const uint32_t v[5] = {wave_sum(a.occ), wave_sum(a.full), wave_sum(a.empty), wave_max32(a.maxb),
                         wave_sum(a.bad)};
  const uint32_t wave = threadIdx.x >> 6;
  __syncthreads();  // (the previous flush's readers are done with s_part)
  if (__lane_id() == 0) {
#pragma unroll
    for (int i = 0; i < 5; ++i) s_part[wave][i] = v[i];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t occ = 0;
    uint32_t full = 0, empty = 0, maxb = 0, bad = 0;
#pragma unroll
    for (uint32_t w = 0; w < kScanThreads / 64; ++w) {
      occ += s_part[w][0];
      full += s_part[w][1];
      empty += s_part[w][2];
      maxb = max(maxb, s_part[w][3]);
      bad += s_part[w][4];
    }
    if (occ) atomicAdd(reinterpret_cast<unsigned long long*>(&st->occupied), (unsigned long long)occ);
    if (full) atomicAdd(&st->full_blocks, full);
    if (empty) atomicAdd(&st->empty_blocks, empty);
    if (maxb > __hip_atomic_load(&st->max_block, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
      atomicMax(&st->max_block, maxb);
    if (bad) atomicAdd(&st->bad_blocks, bad);
  }
  a = ScanAcc{};
}

// What a workgroup has counted for the segment still open when its run of chunks ends.  A filter
// spread over the whole grid would otherwise take two same-address atomics from every workgroup
// at the same moment (one word serves some 90 atomics per microsecond: 4,096 of them were a
// 45 us tail behind a 30 us pass); the slots are combined by scan_fold instead.
struct ScanSlot {  // 32 bytes, 16-byte aligned in the workspace
  uint64_t occ;
  uint32_t seg;  // ~0u: the workgroup had no chunk
  uint32_t full, empty, maxb, bad, pad;
};

static_assert(sizeof(ScanSlot) == 32, "one 32-byte slot per workgroup");

__device__ inline void scan_finish(ScanAcc& a, ScanSlot* slot, uint32_t seg, uint32_t (*s_part)[5])
{
  const uint32_t v[5] = {wave_sum(a.occ), wave_sum(a.full), wave_sum(a.empty), wave_max32(a.maxb),
                         wave_sum(a.bad)};
  const uint32_t wave = threadIdx.x >> 6;
  __syncthreads();
  if (__lane_id() == 0) {
#pragma unroll
    for (int i = 0; i < 5; ++i) s_part[wave][i] = v[i];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    ScanSlot o{};
    o.seg = seg;
#pragma unroll
    for (uint32_t w = 0; w < kScanThreads / 64; ++w) {
      o.occ += s_part[w][0];
      o.full += s_part[w][1];
      o.empty += s_part[w][2];
      o.maxb = max(o.maxb, s_part[w][3]);
      o.bad += s_part[w][4];
    }
    ulonglong2* d = reinterpret_cast<ulonglong2*>(slot);
    d[0] = ulonglong2{o.occ, (uint64_t)o.seg | ((uint64_t)o.full << 32)};
    d[1] = ulonglong2{(uint64_t)o.empty | ((uint64_t)o.maxb << 32), (uint64_t)o.bad};
  }
}

// Folds the slots into the stats, one lane per slot.  The slots' segments never decrease
// (workgroup w took the chunks before workgroup w+1's), so equal segments are neighbours: a
// segmented scan over each wave by shuffles, and the last lane of every run adds the run's sums
// -- at most one set of atomics per segment per wave (32 waves for 2,048 slots).
__global__ __launch_bounds__(kFoldThreads) void scan_fold(const ScanSlot* __restrict__ slots, uint32_t n_slots,
                                                          tkv_amq_filter_stats* __restrict__ stats)
{
  const uint32_t lane = __lane_id();
  const uint32_t i = blockIdx.x * kFoldThreads + threadIdx.x;
  uint32_t seg = ~0u, full = 0, empty = 0, maxb = 0, bad = 0;
  uint64_t occ = 0;
  if (i < n_slots) {
    const ulonglong2* p = reinterpret_cast<const ulonglong2*>(slots + i);
    const ulonglong2 a = p[0];
    seg = (uint32_t)a.y;
    if (seg != ~0u) {  // (a workgroup without a chunk wrote the first half of its slot only)
      const ulonglong2 b = p[1];
      occ = a.x;
      full = (uint32_t)(a.y >> 32);
      empty = (uint32_t)b.x;
      maxb = (uint32_t)(b.x >> 32);
      bad = (uint32_t)b.y;
    }
  }
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t seg2 = __shfl_up(seg, o, 64);
    const uint64_t occ2 = __shfl_up(occ, o, 64);
    const uint32_t full2 = __shfl_up(full, o, 64), empty2 = __shfl_up(empty, o, 64),
                   maxb2 = __shfl_up(maxb, o, 64), bad2 = __shfl_up(bad, o, 64);
    if ((int)lane >= o && seg2 == seg) {
      occ += occ2;
      full += full2;
      empty += empty2;
      maxb = max(maxb, maxb2);
      bad += bad2;
    }
  }
  const uint32_t next = __shfl_down(seg, 1, 64);
  if (seg != ~0u && (lane == 63 || next != seg)) {
    tkv_amq_filter_stats* st = stats + seg;
    if (occ) atomicAdd(reinterpret_cast<unsigned long long*>(&st->occupied), (unsigned long long)occ);
    if (full) atomicAdd(&st->full_blocks, full);
    if (empty) atomicAdd(&st->empty_blocks, empty);
    if (maxb) atomicMax(&st->max_block, maxb);
    if (bad) atomicAdd(&st->bad_blocks, bad);
  }
}

// sum over the four lanes that share a block
__device__ inline uint32_t quad_sum(uint32_t v)
{
  v += __shfl_xor(v, 1, 64);
  v += __shfl_xor(v, 2, 64);
  return v;
}

// One quarter (lane q of its block's four) of a VQF block with T-bit tags.  The metadata rules
// (DESIGN.md 3.2): occ = select(md, B-1) - (B-1); bad if md has fewer than B set bits, if
// occ > S, if popcount(md) is not W-1 (occ 0) / W-occ, or if a tag slot at or past occ is not
// zero.  A block whose metadata gives no occ (the first two) counts as bad only.
template <int T>
__device__ inline void vqf_scan_block(const uint4& w, uint32_t q, bool live, ScanAcc& acc)
{
  constexpr int W = T == 8 ? 128 : 64, B = T == 8 ? 80 : 36, S = T == 8 ? 48 : 28;
  constexpr int kMdBytes = T == 8 ? 16 : 8, kUnit = T / 8, kPer = 4 / kUnit;
  // lane 0 of the four: the metadata
  const uint64_t lo = (uint64_t)w.x | ((uint64_t)w.y << 32);
  const uint64_t hi = T == 8 ? ((uint64_t)w.z | ((uint64_t)w.w << 32)) : 0ull;
  const int pop = __popcll(lo) + __popcll(hi);
  int occ = -1;
  bool bad = false;
  if (pop >= B) {
    occ = (T == 8 ? select128(lo, hi, B - 1) : select64(lo, B - 1)) - (B - 1);
    if (occ > S) occ = -1;
    else bad = pop != (occ == 0 ? W - 1 : W - occ);
  }
  // every lane takes the occ its block's lane 0 found
  const int bocc = __shfl(occ, (int)((__lane_id() & ~3u)), 64);
  // tag slots at or past occ must be zero
  uint32_t stray = 0;
  if (bocc >= 0) {
    const uint32_t wv[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      const int byte = (int)q * 16 + 4 * d;
      if (byte < kMdBytes) continue;
      const int first = (byte - kMdBytes) / kUnit;  // first slot of this dword
      int keep = bocc - first;                      // slots of it that may hold a tag
      keep = keep < 0 ? 0 : (keep > kPer ? kPer : keep);
      const uint32_t m = keep >= kPer ? 0u : ~0u << (8 * kUnit * keep);
      stray |= wv[d] & m;
    }
  }
  const uint32_t any_stray = quad_sum(live && stray != 0 ? 1u : 0u);
  if (q == 0 && live) {
    if (occ < 0) {
      acc.bad += 1;
    } else {
      acc.bad += (bad || any_stray) ? 1u : 0u;
      acc.occ += (uint32_t)occ;
      acc.full += occ == S;
      acc.empty += occ == 0;
      acc.maxb = max(acc.maxb, (uint32_t)occ);
    }
  }
}

template <int KIND>
__global__ __launch_bounds__(kScanThreads) void scan_blocks(const uint8_t* __restrict__ filters,
                                                            const tkv_amq_segment* __restrict__ segs,
                                                            uint32_t n_segs,
                                                            tkv_amq_filter_stats* __restrict__ stats,
                                                            const uint64_t* __restrict__ pre,
                                                            ScanSlot* __restrict__ slots)
{
  __shared__ uint32_t s_part[kScanThreads / 64][5];
  // pre[s] = chunks before segment s; pre[n_segs] = all chunks
  const uint64_t total = pre[n_segs];
  const uint64_t per = (total + gridDim.x - 1) / gridDim.x;
  const uint64_t c0 = per * blockIdx.x;
  if (c0 >= total) {
    if (threadIdx.x == 0) reinterpret_cast<ulonglong2*>(slots + blockIdx.x)[0] = ulonglong2{0, 0xffffffffull};
    return;
  }
  const uint64_t c1 = c0 + per < total ? c0 + per : total;
  // the segment of chunk c0: the last s with pre[s] <= c0 (uniform over the workgroup)
  uint32_t lo = 0, hi = n_segs;
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (pre[mid] <= c0) lo = mid;
    else hi = mid;
  }
  uint32_t s = lo;
  uint64_t s_begin = pre[s], s_end = pre[s + 1];
  const uint32_t tid = threadIdx.x, q = tid & 3u, grp = tid >> 2;
  ScanAcc acc;
  constexpr int kind = KIND;
  ScanSeg g = load_scan_seg(kind, segs, s);
  // the following segment's descriptor and end are fetched while this one's blocks stream, so a
  // segment change (every other chunk with 20 KB leaves) does not wait for two dependent loads
  ScanSeg g_next = g;
  uint64_t next_end = 0;
  if (s + 1 < n_segs) {
    g_next = load_scan_seg(kind, segs, s + 1);
    next_end = pre[s + 2];
  }
  for (uint64_t c = c0; c < c1; ++c) {
    if (c >= s_end) {
      scan_flush(acc, stats + s, s_part);
      if (c < next_end) {  // the usual case: the chunk belongs to segment s + 1
        ++s;
        s_begin = s_end;
        s_end = next_end;
        g = g_next;
      } else {  // segments without a chunk in between
        do {
          ++s;
          s_end = pre[s + 1];
        } while (c >= s_end);
        s_begin = pre[s];
        g = load_scan_seg(kind, segs, s);
      }
      next_end = 0;
      if (s + 1 < n_segs) {
        g_next = load_scan_seg(kind, segs, s + 1);
        next_end = pre[s + 2];
      }
    }
    const uint32_t first = (uint32_t)(c - s_begin) * kScanChunkBlocks;
    const uint32_t left = g.n_blocks - first;
    const uint8_t* blocks =
        filters + g.out_offset + (kind == TKV_AMQ_BLOOM ? kBloomHeader : kVqfHeader + kVqfMetadata) +
        64ull * first;
    uint4 w[kScanRows];
    bool live[kScanRows];
#pragma unroll
    for (uint32_t r = 0; r < kScanRows; ++r) {
      const uint32_t b = r * (kScanThreads / 4) + grp;
      live[r] = b < left;
      w[r] = uint4{0, 0, 0, 0};
      if (live[r]) w[r] = *reinterpret_cast<const uint4*>(blocks + 64ull * b + 16 * q);
    }
    if constexpr (KIND == TKV_AMQ_BLOOM) {
#pragma unroll
      for (uint32_t r = 0; r < kScanRows; ++r) {
        const uint32_t mine = __popc(w[r].x) + __popc(w[r].y) + __popc(w[r].z) + __popc(w[r].w);
        const uint32_t blk = quad_sum(mine);
        acc.occ += mine;
        if (q == 0 && live[r]) {
          acc.full += blk == 512u;
          acc.empty += blk == 0u;
          acc.maxb = max(acc.maxb, blk);
        }
      }
    } else if (g.tag_bits == 8) {
#pragma unroll
      for (uint32_t r = 0; r < kScanRows; ++r) vqf_scan_block<8>(w[r], q, live[r], acc);
    } else {
#pragma unroll
      for (uint32_t r = 0; r < kScanRows; ++r) vqf_scan_block<16>(w[r], q, live[r], acc);
    }
  }
  scan_finish(acc, slots + blockIdx.x, s, s_part);
}

// scan_blocks' grid: as many workgroups as are resident at once (no second, partial round), from
// the runtime's occupancy for the kernel; asked once per kind
template <int KIND>
inline uint32_t scan_grid()
{
  static const uint32_t g = [] {
    int dev = 0, cus = 0, per_cu = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
      cus = 256;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, scan_blocks<KIND>, (int)kScanThreads, 0) !=
            hipSuccess ||
        per_cu <= 0)
      per_cu = 4;
    const uint32_t g = (uint32_t)cus * (uint32_t)per_cu;
    return g < kScanMaxGrid ? g : kScanMaxGrid;
  }();
  return g;
}

// workspace: a 16-byte header (reserved), the chunk prefix pre[n_segs + 1], scan_blocks' slots
inline uint64_t scan_slots_offset(uint32_t n_segs)
{
  return kScanWsHeader + (((uint64_t)n_segs + 1) * 8 + 15) / 16 * 16;
}

inline uint64_t scan_ws_bytes(uint32_t n_segs)
{
  return scan_slots_offset(n_segs) + (uint64_t)kScanMaxGrid * sizeof(ScanSlot);
}

}  // namespace
}  // namespace tkv

using namespace tkv;

extern "C" {

int tkv_amq_open_filters(int kind, const uint8_t* d_filters, uint64_t total_bytes, const uint64_t* d_offsets,
                         uint64_t stride, uint32_t page_size_log2, uint32_t n_filters,
                         tkv_amq_segment* d_segs, uint32_t* d_status, uint32_t* d_summary, void* stream)
{
  // (the arguments are judged first, so a bad call is InvalidArgument with or without a device)
  if (kind != TKV_AMQ_BLOOM && kind != TKV_AMQ_VQF) return TKV_AMQ_INVALID_ARGUMENT;
  // exactly one location form
  const int forms = (d_offsets != nullptr) + (stride != 0) + (page_size_log2 != 0);
  if (forms > 1 || (forms == 0 && n_filters)) return TKV_AMQ_INVALID_ARGUMENT;
  if (page_size_log2 && (page_size_log2 < 7 || page_size_log2 > 31)) return TKV_AMQ_INVALID_ARGUMENT;
  if (reinterpret_cast<uintptr_t>(d_filters) & 15) return TKV_AMQ_INVALID_ARGUMENT;
  if (n_filters && (!d_segs || !d_status || (!d_filters && total_bytes))) return TKV_AMQ_INVALID_ARGUMENT;
  if (tkv_amq_device_count() == 0) return TKV_AMQ_UNAVAILABLE;
  const hipStream_t s = static_cast<hipStream_t>(stream);
  if (d_summary && hipMemsetAsync(d_summary, 0, 7 * sizeof(uint32_t), s) != hipSuccess)
    return TKV_AMQ_INTERNAL;
  if (n_filters == 0) return TKV_AMQ_OK;
  OpenArgs a;
  a.kind = kind;
  a.filters = d_filters;
  a.total_bytes = total_bytes;
  a.offsets = d_offsets;
  a.stride = stride;
  a.page_log2 = page_size_log2;
  a.n = n_filters;
  a.segs = d_segs;
  a.status = d_status;
  a.summary = d_summary;
  hipLaunchKernelGGL(open_filters_kernel, dim3((n_filters + 255u) / 256u), dim3(256), 0, s, a);
  return hipGetLastError() == hipSuccess ? TKV_AMQ_OK : TKV_AMQ_INTERNAL;
}

uint64_t tkv_amq_scan_filters_ws_bytes(uint32_t n_segs) { return scan_ws_bytes(n_segs); }

int tkv_amq_scan_filters(int kind, const uint8_t* d_filters, const tkv_amq_segment* d_segs, uint32_t n_segs,
                         tkv_amq_filter_stats* d_stats, void* d_workspace, uint64_t workspace_bytes,
                         void* stream)
{
  if (kind != TKV_AMQ_BLOOM && kind != TKV_AMQ_VQF) return TKV_AMQ_INVALID_ARGUMENT;
  if (n_segs) {
    if (!d_filters || !d_segs || !d_stats || !d_workspace) return TKV_AMQ_INVALID_ARGUMENT;
    if (workspace_bytes < scan_ws_bytes(n_segs) || (reinterpret_cast<uintptr_t>(d_workspace) & 15) ||
        (reinterpret_cast<uintptr_t>(d_filters) & 15) || (reinterpret_cast<uintptr_t>(d_stats) & 15))
      return TKV_AMQ_INVALID_ARGUMENT;
  }
  if (tkv_amq_device_count() == 0) return TKV_AMQ_UNAVAILABLE;
  if (n_segs == 0) return TKV_AMQ_OK;
  const hipStream_t s = static_cast<hipStream_t>(stream);
  uint64_t* pre = reinterpret_cast<uint64_t*>(static_cast<uint8_t*>(d_workspace) + kScanWsHeader);
  hipLaunchKernelGGL(scan_init, dim3((n_segs + 255u) / 256u), dim3(256), 0, s, kind, d_filters, d_segs,
                     n_segs, d_stats, pre);
  hipLaunchKernelGGL(prefix_inclusive_u64<kPrefixThreads>, dim3(1), dim3(kPrefixThreads), 0, s, pre + 1, n_segs);
  ScanSlot* slots = reinterpret_cast<ScanSlot*>(static_cast<uint8_t*>(d_workspace) + scan_slots_offset(n_segs));
  const uint32_t grid = kind == TKV_AMQ_BLOOM ? scan_grid<TKV_AMQ_BLOOM>() : scan_grid<TKV_AMQ_VQF>();
  if (kind == TKV_AMQ_BLOOM)
    hipLaunchKernelGGL(scan_blocks<TKV_AMQ_BLOOM>, dim3(grid), dim3(kScanThreads), 0, s, d_filters, d_segs,
                       n_segs, d_stats, static_cast<const uint64_t*>(pre), slots);
  else
    hipLaunchKernelGGL(scan_blocks<TKV_AMQ_VQF>, dim3(grid), dim3(kScanThreads), 0, s, d_filters, d_segs,
                       n_segs, d_stats, static_cast<const uint64_t*>(pre), slots);
  hipLaunchKernelGGL(scan_fold, dim3((grid + kFoldThreads - 1) / kFoldThreads), dim3(kFoldThreads), 0, s,
                     static_cast<const ScanSlot*>(slots), grid, d_stats);
  return hipGetLastError() == hipSuccess ? TKV_AMQ_OK : TKV_AMQ_INTERNAL;
}

}  // extern "C"
