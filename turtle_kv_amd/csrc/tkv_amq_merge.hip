// tkv_amq_merge.hip -- the leaf update on the device: tkv_amq_merge_leaves (records) and
// tkv_amq_gather_merged (bytes); and the same over a table of up to eight runs,
// the node merge: tkv_amq_merge_levels and tkv_amq_gather_levels, DESIGN.md section 19 (levels_plan,
// levels_rank, levels_emit and the gather_levels_* kernels, described where they stand).
//
// A job merges one leaf's update (the newer run) with the leaf's items (the older run).  Nothing
// walks the two runs in step: every item finds its place by a search in the other run (tkv::bound
// over OrderedQuery, the read side's key order), so the work splits by items.
//
//   merge_plan       one workgroup: per job the clamped item ranges, their saturating prefixes (the
//                    workspace slots of the job's items, per run) and the job's units -- up to `chunk`
//                    consecutive items of one run of one job -- as a prefix over the jobs
//   merge_rank       pass 1, one workgroup per unit (found through the prefix, as the membership
//                    audit finds its leaves): per item its bound in the other run, its partner or
//                    shadow, the candidate's resolved op and the keep flag; the flags' exclusive
//                    prefix over the unit (block_exclusive_scan); per slot the bound and
//                    prefix << 9 | op << 1 | keep; per unit the kept count; the counters
//   merge_offsets    one workgroup: the units' kept counts to their exclusive prefix, d_out_begin
//                    from it, *d_needed, out_count
//   merge_emit       pass 2, one workgroup per unit: a kept item's position is its job's begin + the
//                    kept items of its own run before it + the kept items of the other run before
//                    its bound, each a unit's prefix plus a slot's; the record goes there
//
//   gather_measure   one lane per record: the key's and the value's length; their prefix inside the
//                    workgroup's 1,024 records into the offset arrays, the workgroup's sums aside
//   scan_totals      (tkv_amq_scan.h) the sums to their prefix, and the totals
//   gather_move      sixteen lanes per record: the final offsets, and the bytes, eight per lane and
//                    step, as gather_values_kernel moves them
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "tkv_amq.h"
#include "tkv_amq_device.h"
#include "tkv_amq_launch.h"
#include "tkv_amq_scan.h"
#include "tkv_amq_value.h"

namespace tkv {
namespace {

constexpr uint32_t kMergeThreads = 256;
// the unit loops' workgroups at most (units past the grid are reached by its stride)
constexpr uint64_t kMergeMaxGrid = 1ull << 20;
// Items per unit, from the batch's size alone: about kMergeTargetUnits units over the batch (sixteen
// workgroups for each of 256 CUs), at least four rounds of a workgroup each, in multiples of a
// round, and below 2^21 so that a unit's prefix fits the slot word beside the op and the flag.
constexpr uint64_t kMergeTargetUnits = 4096;
constexpr uint64_t kMergeMinChunk = 4 * kMergeThreads;
constexpr uint64_t kMergeMaxChunk = 1ull << 20;
constexpr uint64_t kMergeWsHeader = 16;

inline uint32_t merge_chunk(uint64_t n_items)
{
  uint64_t c = div_up(n_items, kMergeTargetUnits);
  c = c < kMergeMinChunk ? kMergeMinChunk : c > kMergeMaxChunk ? kMergeMaxChunk : c;
  return (uint32_t)(div_up(c, kMergeThreads) * kMergeThreads);
}

// the units of `items` items of one run of one job
__host__ __device__ inline uint64_t merge_units_of(uint64_t items, uint32_t chunk) { return (items + chunk - 1) / chunk; }

// every job has at most one short unit per run
inline uint64_t merge_max_units(uint64_t n_jobs, uint64_t n_items)
{
  return n_items / merge_chunk(n_items) + 2 * n_jobs;
}

// the same for the smallest unit: what the workspace holds, so that its size is monotone in the counts
inline uint64_t merge_ws_units(uint64_t n_jobs, uint64_t n_items) { return n_items / kMergeMinChunk + 2 * n_jobs; }

inline uint64_t round16(uint64_t b) { return div_up(b, 16) * 16; }

// One run on the device: its keys, its values, the jobs' ranges.
struct MergeRun {
  KeyArray keys;
  ValueArray vals;
  const uint64_t* begin;
  uint64_t n;
};

inline MergeRun merge_run(const tkv_amq_merge_run& r)
{
  return MergeRun{KeyArray{r.keys, r.key_offsets, r.key_stride},
                  ValueArray{r.values, r.value_offsets, r.value_stride, r.values_bytes}, r.d_begin, r.n_items};
}

// The workspace: three prefixes over the jobs (the newer run's slots, the older run's, the units),
// the units' kept counts, and two words per slot.
struct MergeWs {
  uint64_t* slot[2];  // [n_jobs + 1] each: job j's items of run s own slots [slot[s][j], slot[s][j + 1])
  uint64_t* upre;     // [n_jobs + 1]: units before job j (a job's newer units come first)
  uint64_t* kept;     // [merge_ws_units + 1]: a unit's kept count, then the exclusive prefix of these
  uint32_t* rank[2];  // [n_items of the run]: the item's bound in the other run, relative to the job's range
  uint32_t* mark[2];  // [n_items of the run]: kept items of the unit before it << 9 | op << 1 | keep
  uint64_t bytes;
};

// (the pointers are offsets from `ws`; with ws == 0 only `bytes` means anything)
inline MergeWs merge_ws(void* ws, uint64_t n_jobs, uint64_t n_newer, uint64_t n_older)
{
  const uintptr_t base = reinterpret_cast<uintptr_t>(ws);
  uint64_t off = kMergeWsHeader;
  MergeWs w;
  auto take = [&](auto*& p, uint64_t bytes) {
    p = reinterpret_cast<std::remove_reference_t<decltype(p)>>(base + off);
    off += round16(bytes);
  };
  const uint64_t n[2] = {n_newer, n_older};
  for (int s = 0; s < 2; ++s) take(w.slot[s], (n_jobs + 1) * 8);
  take(w.upre, (n_jobs + 1) * 8);
  take(w.kept, (merge_ws_units(n_jobs, n_newer + n_older) + 1) * 8);
  for (int s = 0; s < 2; ++s) take(w.rank[s], n[s] * 4);
  for (int s = 0; s < 2; ++s) take(w.mark[s], n[s] * 4);
  w.bytes = off;
  return w;
}

struct MergeArgs {
  MergeRun run[2];  // 0 newer, 1 older
  MergeWs ws;
  uint32_t n_jobs, chunk, decay;
  uint64_t* out_begin;
  tkv_amq_merge_item* items;
  uint64_t out_capacity;
  uint64_t* needed;
  tkv_amq_merge_counts* counts;
};

// a job's range in a run: both ends clamped to the run's items, an end below its begin reads as empty
__device__ inline void merge_range(const MergeRun& r, uint32_t j, uint64_t& b, uint64_t& count)
{
  const uint64_t lo = r.begin[j], hi = r.begin[j + 1];
  b = lo < r.n ? lo : r.n;
  const uint64_t e = hi < r.n ? hi : r.n;
  count = e > b ? e - b : 0;
}

__global__ __launch_bounds__(kBlockScanThreads) void merge_plan(MergeArgs a)
{
  __shared__ uint64_t s_waves[kBlockScanThreads / 64];
  const uint32_t tid = threadIdx.x;
  uint64_t base[2] = {0, 0}, ubase = 0;
  for (uint32_t j0 = 0; j0 < a.n_jobs; j0 += kBlockScanThreads) {
    const uint32_t j = j0 + tid;
    uint64_t units = 0;
    for (int s = 0; s < 2; ++s) {
      uint64_t b, count = 0, total;
      if (j < a.n_jobs) merge_range(a.run[s], j, b, count);
      // the slots a job owns end where the run's items end: overlapping ranges read no more than that
      const uint64_t before = min(base[s] + block_exclusive_scan<uint64_t>(count, s_waves, &total), a.run[s].n);
      const uint64_t after = min(before + count, a.run[s].n);
      if (j < a.n_jobs) a.ws.slot[s][j] = before;
      units += merge_units_of(after - before, a.chunk);
      base[s] = min(base[s] + total, a.run[s].n);
    }
    uint64_t utotal;
    const uint64_t ubefore = ubase + block_exclusive_scan<uint64_t>(units, s_waves, &utotal);
    if (j < a.n_jobs) a.ws.upre[j] = ubefore;
    ubase += utotal;
  }
  if (tid == 0) {
    a.ws.slot[0][a.n_jobs] = base[0];
    a.ws.slot[1][a.n_jobs] = base[1];
    a.ws.upre[a.n_jobs] = ubase;
  }
}

// the job of unit u: the last j with upre[j] <= u (it has upre[j + 1] > u: jobs without a unit are skipped)
__device__ inline uint32_t merge_find_job(const uint64_t* __restrict__ upre, uint32_t n_jobs, uint64_t u)
{
  uint32_t lo = 0, hi = n_jobs;
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (upre[mid] <= u) lo = mid;
    else hi = mid;
  }
  return lo;
}

// What a unit is: items [i0, i1) (relative to the job's range) of run `side` of job `job`.
struct MergeUnit {
  uint32_t job, side;
  uint64_t b[2], count[2];  // the job's ranges: first item, items read
  uint64_t slot[2];         // the ranges' first slots
  uint64_t ubase[2];        // the first unit of either run
  uint64_t i0, i1;
};

__device__ inline MergeUnit merge_unit(const MergeArgs& a, uint64_t u)
{
  MergeUnit m;
  m.job = merge_find_job(a.ws.upre, a.n_jobs, u);
  for (int s = 0; s < 2; ++s) {
    uint64_t count;
    merge_range(a.run[s], m.job, m.b[s], count);
    m.slot[s] = a.ws.slot[s][m.job];
    m.count[s] = a.ws.slot[s][m.job + 1] - m.slot[s];
  }
  m.ubase[0] = a.ws.upre[m.job];
  m.ubase[1] = m.ubase[0] + merge_units_of(m.count[0], a.chunk);
  m.side = u >= m.ubase[1];
  m.i0 = (u - m.ubase[m.side]) * a.chunk;
  m.i1 = min(m.i0 + a.chunk, m.count[m.side]);
  return m;
}

// an item's op and integer: an empty value is a NOOP without data
__device__ inline void merge_value(const ValueArray& v, uint64_t i, uint32_t& op, uint32_t& i32)
{
  uint64_t vb, ve;
  value_range(v, i, vb, ve);
  op = ve > vb ? v.values[vb] : TKV_AMQ_OP_NOOP;
  i32 = ve > vb ? value_i32(v.values + vb + 1, ve - vb - 1) : 0u;
}

// The candidate of newer item i whose partner is older item p (or none): combine() of the two values
// (core/value_view.hpp:316-335).
struct MergeCandidate {
  uint32_t op, i32, flags;
};

__device__ inline MergeCandidate merge_candidate(const MergeArgs& a, uint64_t i, bool partner, uint64_t p)
{
  MergeCandidate c;
  uint32_t x;
  merge_value(a.run[0].vals, i, c.op, x);
  c.i32 = 0;
  c.flags = 0;
  if (partner && c.op == TKV_AMQ_OP_ADD_I32) {
    uint32_t older_op, y;
    merge_value(a.run[1].vals, p, older_op, y);
    if (older_op == TKV_AMQ_OP_WRITE || older_op == TKV_AMQ_OP_DELETE) {
      c.op = TKV_AMQ_OP_WRITE;
      c.i32 = older_op == TKV_AMQ_OP_WRITE ? x + y : x;
      c.flags = TKV_AMQ_VALUE_COMBINED;
    } else if (older_op == TKV_AMQ_OP_ADD_I32) {
      c.i32 = x + y;
      c.flags = TKV_AMQ_VALUE_COMBINED;
    } else {
      c.flags = TKV_AMQ_VALUE_BAD_COMBINE;
    }
  }
  return c;
}

// decays_to_item (core/value_view.hpp:372-398)
__device__ inline bool merge_op_stays(uint32_t op)
{
  return op == TKV_AMQ_OP_WRITE || op == TKV_AMQ_OP_ADD_I32 || op == TKV_AMQ_OP_PAGE_SLICE;
}

template <int ORDER>
__global__ __launch_bounds__(kMergeThreads) void merge_rank(MergeArgs a)
{
  __shared__ uint32_t s_waves[kMergeThreads / 64];
  const uint64_t n_units = a.ws.upre[a.n_jobs];
  const uint32_t tid = threadIdx.x;
  uint32_t n_pair = 0, n_combined = 0, n_bad = 0, n_dropped = 0, n_read[2] = {0, 0};
  for (uint64_t u = blockIdx.x; u < n_units; u += gridDim.x) {
    const MergeUnit m = merge_unit(a, u);
    const uint32_t s = m.side, t = s ^ 1u;
    const KeyArray& other = a.run[t].keys;
    uint32_t run_kept = 0;  // kept items of the unit before this round
    for (uint64_t i0 = m.i0; i0 < m.i1; i0 += kMergeThreads) {
      const uint64_t i = i0 + tid;
      uint32_t keep = 0, op = 0, rank = 0;
      if (i < m.i1) {
        const uint64_t g = m.b[s] + i;
        const OrderedQuery<ORDER> q(a.run[s].keys, g);
        ++n_read[s];
        if (s == 0) {
          // the lower bound: the partner, if there is one, stands there
          const uint64_t r = bound(m.b[1], m.count[1], [&](uint64_t k) { return q.less(other, k); });
          const bool partner = r < m.b[1] + m.count[1] && q.equal(other, r);
          const MergeCandidate c = merge_candidate(a, g, partner, r);
          rank = (uint32_t)(r - m.b[1]);
          op = c.op;
          keep = 1;
          n_combined += (c.flags & TKV_AMQ_VALUE_COMBINED) != 0;
          n_bad += (c.flags & TKV_AMQ_VALUE_BAD_COMBINE) != 0;
        } else {
          // the upper bound: the item that shadows this one, if there is one, stands before it
          const uint64_t r = bound(m.b[0], m.count[0], [&](uint64_t k) { return q.less_equal(other, k); });
          const bool shadowed = r > m.b[0] && q.equal(other, r - 1);
          uint32_t x;
          merge_value(a.run[1].vals, g, op, x);
          rank = (uint32_t)(r - m.b[0]);
          keep = !shadowed;
          n_pair += shadowed;
        }
        if (keep && a.decay && !merge_op_stays(op)) {
          keep = 0;
          ++n_dropped;
        }
      }
      uint32_t total;
      const uint32_t before = run_kept + block_exclusive_scan<uint32_t>(keep, s_waves, &total);
      if (i < m.i1) {
        a.ws.rank[s][m.slot[s] + i] = rank;
        a.ws.mark[s][m.slot[s] + i] = before << 9 | (op & 0xffu) << 1 | keep;
      }
      run_kept += total;
    }
    if (tid == 0) a.ws.kept[u] = run_kept;
  }
  if (a.counts) {
    // one atomic per non-zero counter per wave
    const uint32_t v[6] = {wave_sum(n_read[0]), wave_sum(n_read[1]), wave_sum(n_pair),
                           wave_sum(n_combined), wave_sum(n_bad),     wave_sum(n_dropped)};
    if (__lane_id() == 0) {
      unsigned long long* c = reinterpret_cast<unsigned long long*>(a.counts);
#pragma unroll
      for (int j = 0; j < 6; ++j)
        if (v[j]) atomicAdd(&c[j], (unsigned long long)v[j]);
    }
  }
}

// kept[u] <- the kept counts of the units before u, for u up to n_units; d_out_begin; the total.
// n_jobs == 0: the workspace is not touched.
__global__ __launch_bounds__(kBlockScanThreads) void merge_offsets(MergeArgs a)
{
  __shared__ uint64_t s_waves[kBlockScanThreads / 64];
  const uint32_t tid = threadIdx.x;
  uint64_t base = 0;
  if (a.n_jobs) {
    const uint64_t n_units = a.ws.upre[a.n_jobs];
    for (uint64_t u0 = 0; u0 < n_units; u0 += kBlockScanThreads) {
      const uint64_t u = u0 + tid;
      const uint64_t v = u < n_units ? a.ws.kept[u] : 0;
      uint64_t total;
      const uint64_t before = base + block_exclusive_scan<uint64_t>(v, s_waves, &total);
      if (u < n_units) a.ws.kept[u] = before;
      base += total;
    }
    if (tid == 0) a.ws.kept[n_units] = base;
    __syncthreads();  // (the prefixes are read back by other threads of this workgroup)
    for (uint64_t j = tid; j <= a.n_jobs; j += kBlockScanThreads) a.out_begin[j] = a.ws.kept[a.ws.upre[j]];
  } else if (tid == 0) {
    a.out_begin[0] = 0;
  }
  if (tid == 0) {
    if (a.needed) *a.needed = base;
    if (a.counts && base) atomicAdd(reinterpret_cast<unsigned long long*>(&a.counts->out_count), (unsigned long long)base);
  }
}

// the kept items of run s of the unit's job before its item i (relative to the job's range)
__device__ inline uint64_t merge_kept_before(const MergeArgs& a, const MergeUnit& m, uint32_t s, uint64_t i)
{
  if (i == 0) return 0;
  const uint32_t x = a.ws.mark[s][m.slot[s] + i - 1];
  return a.ws.kept[m.ubase[s] + (i - 1) / a.chunk] - a.ws.kept[m.ubase[s]] + (x >> 9) + (x & 1u);
}

template <int ORDER>
__global__ __launch_bounds__(kMergeThreads) void merge_emit(MergeArgs a)
{
  const uint64_t n_units = a.ws.upre[a.n_jobs];
  for (uint64_t u = blockIdx.x; u < n_units; u += gridDim.x) {
    const MergeUnit m = merge_unit(a, u);
    const uint32_t s = m.side, t = s ^ 1u;
    // the job's first record, and the kept items of this run in the job's units before this one
    const uint64_t first = a.ws.kept[m.ubase[0]] + a.ws.kept[u] - a.ws.kept[m.ubase[s]];
    for (uint64_t i = m.i0 + threadIdx.x; i < m.i1; i += kMergeThreads) {
      const uint32_t x = a.ws.mark[s][m.slot[s] + i];
      if (!(x & 1u)) continue;
      const uint64_t r = a.ws.rank[s][m.slot[s] + i];
      const uint64_t pos = first + (x >> 9) + merge_kept_before(a, m, t, r);
      if (pos >= a.out_capacity) continue;
      const uint64_t g = m.b[s] + i;
      MergeCandidate c{(x >> 1) & 0xffu, 0u, 0u};
      if (s == 0) {
        const bool partner = r < m.count[1] && OrderedQuery<ORDER>(a.run[0].keys, g).equal(a.run[1].keys, m.b[1] + r);
        c = merge_candidate(a, g, partner, m.b[1] + r);
      }
      *reinterpret_cast<ulonglong2*>(a.items + pos) =
          ulonglong2{(uint64_t)s << 63 | g, mk64(c.i32, c.op | c.flags << 8)};
    }
  }
}

// ---------------------------------------------------------------------------------------
// tkv_amq_merge_levels: the same four passes over a table of up to TKV_AMQ_MERGE_MAX_RUNS runs
// (DESIGN.md section 19).  Nothing here holds a per-run array in registers: what a unit needs of
// another run (its range, its slots, its first unit) is read from the run table and the workspace
// inside a loop over the runs, and an item's bounds go to the workspace as they are found, so the
// run count stays a runtime value and no kernel uses scratch.
constexpr uint32_t kLevelsMaxRuns = TKV_AMQ_MERGE_MAX_RUNS;
constexpr uint32_t kMarkPrefixMask = 0x1fffffu;  // bits 9..29 of a mark: a unit's prefix is below 2^20
constexpr uint32_t kMarkFlagsShift = 30;         // bits 30..31: the value flags of a kept head

static_assert(kMergeMaxChunk <= kMarkPrefixMask, "a unit's prefix fits its field of the mark");
static_assert((TKV_AMQ_VALUE_COMBINED | TKV_AMQ_VALUE_BAD_COMBINE) <= 3u, "the value flags fit two bits");

inline uint64_t levels_max_units(uint64_t n_jobs, uint32_t n_runs, uint64_t n_items)
{
  return n_items / merge_chunk(n_items) + n_runs * n_jobs;
}

inline uint64_t levels_ws_units(uint64_t n_jobs, uint32_t n_runs, uint64_t n_items)
{
  return n_items / kMergeMinChunk + n_runs * n_jobs;
}

// The workspace.  An item's words are indexed by its run's first item (LevelsArgs::ibase) plus its slot.
struct LevelsWs {
  uint64_t* slot;  // [n_runs][n_jobs + 1]: job j's items of run s own slots [slot[s][j], slot[s][j + 1])
  uint64_t* upre;  // [n_jobs + 1]: units before job j (a job's units run by run, the newest first)
  uint64_t* kept;  // [levels_ws_units + 1]: a unit's kept count, then the exclusive prefix of these
  uint32_t* rank;  // [n_runs - 1][n_total]: a kept head's bound in every other run, relative to the job's range
  uint32_t* mark;  // [n_total]: flags << 30 | kept items of the unit before it << 9 | op << 1 | keep
  uint32_t* fold;  // [n_total]: the folded integer of a kept head whose value is COMBINED
  uint64_t bytes;
};

inline LevelsWs levels_ws(void* ws, uint64_t n_jobs, uint32_t n_runs, uint64_t n_total)
{
  const uintptr_t base = reinterpret_cast<uintptr_t>(ws);
  uint64_t off = kMergeWsHeader;
  LevelsWs w;
  auto take = [&](auto*& p, uint64_t bytes) {
    p = reinterpret_cast<std::remove_reference_t<decltype(p)>>(base + off);
    off += round16(bytes);
  };
  take(w.slot, n_runs * (n_jobs + 1) * 8);
  take(w.upre, (n_jobs + 1) * 8);
  take(w.kept, (levels_ws_units(n_jobs, n_runs, n_total) + 1) * 8);
  take(w.rank, (n_runs - 1) * n_total * 4);
  take(w.mark, n_total * 4);
  take(w.fold, n_total * 4);
  w.bytes = off;
  return w;
}

struct LevelsArgs {
  MergeRun run[kLevelsMaxRuns];    // 0 the newest
  uint64_t ibase[kLevelsMaxRuns];  // the items of the runs before run s
  LevelsWs ws;
  uint64_t n_total;
  uint32_t n_runs, n_jobs, chunk, decay;
  tkv_amq_merge_item* items;
  uint64_t out_capacity;
};

__device__ inline uint64_t* levels_slots(const LevelsArgs& a, uint32_t s) { return a.ws.slot + (uint64_t)s * (a.n_jobs + 1); }

// One workgroup, run by run: the slots of every job, and the jobs' units summed into upre (thread
// tid alone touches upre[j0 + tid]); then upre to its exclusive prefix.
__global__ __launch_bounds__(kBlockScanThreads) void levels_plan(LevelsArgs a)
{
  __shared__ uint64_t s_waves[kBlockScanThreads / 64];
  const uint32_t tid = threadIdx.x;
  for (uint32_t s = 0; s < a.n_runs; ++s) {
    uint64_t* slot = levels_slots(a, s);
    const uint64_t n = a.run[s].n;
    uint64_t base = 0;
    for (uint32_t j0 = 0; j0 < a.n_jobs; j0 += kBlockScanThreads) {
      const uint32_t j = j0 + tid;
      uint64_t b, count = 0, total;
      if (j < a.n_jobs) merge_range(a.run[s], j, b, count);
      // the slots a job owns end where the run's items end: overlapping ranges read no more than that
      const uint64_t before = min(base + block_exclusive_scan<uint64_t>(count, s_waves, &total), n);
      const uint64_t after = min(before + count, n);
      if (j < a.n_jobs) {
        const uint64_t units = merge_units_of(after - before, a.chunk);
        slot[j] = before;
        a.ws.upre[j] = s ? a.ws.upre[j] + units : units;
      }
      base = min(base + total, n);
    }
    if (tid == 0) slot[a.n_jobs] = base;
  }
  uint64_t ubase = 0;
  for (uint32_t j0 = 0; j0 < a.n_jobs; j0 += kBlockScanThreads) {
    const uint32_t j = j0 + tid;
    uint64_t utotal;
    const uint64_t ubefore = ubase + block_exclusive_scan<uint64_t>(j < a.n_jobs ? a.ws.upre[j] : 0, s_waves, &utotal);
    if (j < a.n_jobs) a.ws.upre[j] = ubefore;
    ubase += utotal;
  }
  if (tid == 0) a.ws.upre[a.n_jobs] = ubase;
}

// a job's items of run t: the first one, and how many are read (what the plan left in the slots)
__device__ inline void levels_range(const LevelsArgs& a, uint32_t t, uint32_t job, uint64_t& b, uint64_t& count, uint64_t& slot)
{
  const uint64_t* st = levels_slots(a, t);
  const uint64_t lo = a.run[t].begin[job];
  b = lo < a.run[t].n ? lo : a.run[t].n;
  slot = st[job];
  count = st[job + 1] - slot;
}

// What a unit is: items [i0, i1) (relative to the job's range) of run `side` of job `job`.
struct LevelsUnit {
  uint32_t job, side;
  uint64_t b, count;  // the job's range in that run: first item, items read
  uint64_t word;      // the workspace word of the range's first item
  uint64_t ubase;     // the run's first unit
  uint64_t i0, i1;
};

__device__ inline LevelsUnit levels_unit(const LevelsArgs& a, uint64_t u)
{
  LevelsUnit m;
  m.job = merge_find_job(a.ws.upre, a.n_jobs, u);
  m.ubase = a.ws.upre[m.job];
  // (unit u is one of the job's, so a run holds it; the last run ends the search whatever the words say)
  for (m.side = 0;; ++m.side) {
    uint64_t slot;
    levels_range(a, m.side, m.job, m.b, m.count, slot);
    m.word = a.ibase[m.side] + slot;
    const uint64_t units = merge_units_of(m.count, a.chunk);
    if (u - m.ubase < units || m.side + 1 == a.n_runs) break;
    m.ubase += units;
  }
  m.i0 = min((u - m.ubase) * a.chunk, m.count);
  m.i1 = min(m.i0 + a.chunk, m.count);
  return m;
}

// Pass 1.  An item of run s looks for the item that shadows it in the newer runs (the upper bound of
// its key there, the item before it) and, a head, for its partners in the older ones (the lower
// bound, the item at it), folding its value through them in run order while it is an ADD_I32
// (run_compact, core/algo/parallel_compact.hpp:92-100).  Each bound goes to the item's own rank
// words as it is found; those of an item that is not kept are never read.
template <int ORDER>
__global__ __launch_bounds__(kMergeThreads) void levels_rank(LevelsArgs a, tkv_amq_merge_counts* counts)
{
  __shared__ uint32_t s_waves[kMergeThreads / 64];
  const uint64_t n_units = a.ws.upre[a.n_jobs];
  const uint32_t tid = threadIdx.x;
  uint32_t n_newer = 0, n_older = 0, n_pair = 0, n_combined = 0, n_bad = 0, n_dropped = 0;
  for (uint64_t u = blockIdx.x; u < n_units; u += gridDim.x) {
    const LevelsUnit m = levels_unit(a, u);
    const uint32_t s = m.side;
    uint32_t run_kept = 0;  // kept items of the unit before this round
    for (uint64_t i0 = m.i0; i0 < m.i1; i0 += kMergeThreads) {
      const uint64_t i = i0 + tid;
      uint32_t keep = 0, op = 0, acc = 0, flags = 0;
      if (i < m.i1) {
        const uint64_t g = m.b + i;
        const OrderedQuery<ORDER> q(a.run[s].keys, g);
        uint32_t* rank = a.ws.rank + m.word + i;
        n_newer += s == 0;
        n_older += s != 0;
        bool shadowed = false;
        for (uint32_t t = 0; t < s && !shadowed; ++t) {
          const KeyArray& other = a.run[t].keys;
          uint64_t b, count, slot;
          levels_range(a, t, m.job, b, count, slot);
          const uint64_t r = bound(b, count, [&](uint64_t k) { return q.less_equal(other, k); });
          shadowed = r > b && q.equal(other, r - 1);
          rank[t * a.n_total] = (uint32_t)(r - b);
        }
        if (shadowed) {
          ++n_pair;
        } else {
          merge_value(a.run[s].vals, g, op, acc);
          for (uint32_t t = s + 1; t < a.n_runs; ++t) {
            const KeyArray& other = a.run[t].keys;
            uint64_t b, count, slot;
            levels_range(a, t, m.job, b, count, slot);
            const uint64_t r = bound(b, count, [&](uint64_t k) { return q.less(other, k); });
            rank[(t - 1) * a.n_total] = (uint32_t)(r - b);
            if (op == TKV_AMQ_OP_ADD_I32 && r < b + count && q.equal(other, r)) {
              uint32_t older_op, y;
              merge_value(a.run[t].vals, r, older_op, y);
              if (older_op == TKV_AMQ_OP_WRITE || older_op == TKV_AMQ_OP_DELETE) {
                op = TKV_AMQ_OP_WRITE;
                acc = older_op == TKV_AMQ_OP_WRITE ? acc + y : acc;
                flags |= TKV_AMQ_VALUE_COMBINED;
              } else if (older_op == TKV_AMQ_OP_ADD_I32) {
                acc += y;
                flags |= TKV_AMQ_VALUE_COMBINED;
              } else {
                flags |= TKV_AMQ_VALUE_BAD_COMBINE;
                ++n_bad;
              }
            }
          }
          n_combined += (flags & TKV_AMQ_VALUE_COMBINED) != 0;
          keep = 1;
          if (a.decay && !merge_op_stays(op)) {
            keep = 0;
            ++n_dropped;
          }
        }
      }
      uint32_t total;
      const uint32_t before = run_kept + block_exclusive_scan<uint32_t>(keep, s_waves, &total);
      if (i < m.i1) {
        a.ws.mark[m.word + i] = flags << kMarkFlagsShift | before << 9 | (op & 0xffu) << 1 | keep;
        if (flags & TKV_AMQ_VALUE_COMBINED) a.ws.fold[m.word + i] = acc;
      }
      run_kept += total;
    }
    if (tid == 0) a.ws.kept[u] = run_kept;
  }
  if (counts) {
    // one atomic per non-zero counter per wave
    const uint32_t v[6] = {wave_sum(n_newer),    wave_sum(n_older), wave_sum(n_pair),
                           wave_sum(n_combined), wave_sum(n_bad),   wave_sum(n_dropped)};
    if (__lane_id() == 0) {
      unsigned long long* c = reinterpret_cast<unsigned long long*>(counts);
#pragma unroll
      for (int j = 0; j < 6; ++j)
        if (v[j]) atomicAdd(&c[j], (unsigned long long)v[j]);
    }
  }
}

// Pass 2 (merge_offsets between the two): a kept item's position is its job's begin + the kept items
// of its own run before it + for every other run the kept items before its bound there.  The record
// comes from the workspace alone: the op and the flags from the mark, the folded integer from `fold`.
__global__ __launch_bounds__(kMergeThreads) void levels_emit(LevelsArgs a)
{
  const uint64_t n_units = a.ws.upre[a.n_jobs];
  for (uint64_t u = blockIdx.x; u < n_units; u += gridDim.x) {
    const LevelsUnit m = levels_unit(a, u);
    const uint32_t s = m.side;
    const uint64_t job_units = a.ws.upre[m.job];
    // the job's first record, and the kept items of this run in the job's units before this one
    const uint64_t first = a.ws.kept[job_units] + a.ws.kept[u] - a.ws.kept[m.ubase];
    for (uint64_t i = m.i0 + threadIdx.x; i < m.i1; i += kMergeThreads) {
      const uint32_t x = a.ws.mark[m.word + i];
      if (!(x & 1u)) continue;
      uint64_t pos = first + ((x >> 9) & kMarkPrefixMask);
      uint64_t ubase = job_units;  // run t's first unit
      for (uint32_t t = 0; t < a.n_runs; ++t) {
        uint64_t b, count, slot;
        levels_range(a, t, m.job, b, count, slot);
        if (t != s) {
          const uint64_t r = a.ws.rank[m.word + i + (uint64_t)(t < s ? t : t - 1) * a.n_total];
          if (r) {
            const uint32_t y = a.ws.mark[a.ibase[t] + slot + r - 1];
            pos += a.ws.kept[ubase + (r - 1) / a.chunk] - a.ws.kept[ubase] + ((y >> 9) & kMarkPrefixMask) + (y & 1u);
          }
        }
        ubase += merge_units_of(count, a.chunk);
      }
      if (pos >= a.out_capacity) continue;
      const uint32_t flags = x >> kMarkFlagsShift;
      const uint32_t i32 = flags & TKV_AMQ_VALUE_COMBINED ? a.ws.fold[m.word + i] : 0u;
      *reinterpret_cast<ulonglong2*>(a.items + pos) =
          ulonglong2{(uint64_t)s << TKV_AMQ_LEVELS_SRC_SHIFT | (m.b + i), mk64(i32, ((x >> 1) & 0xffu) | flags << 8)};
    }
  }
}

// ---------------------------------------------------------------------------------------
// tkv_amq_gather_merged and tkv_amq_gather_levels
constexpr uint32_t kMeasurePerThread = 4;
constexpr uint32_t kMeasureSpan = kBlockScanThreads * kMeasurePerThread;  // records per workgroup
constexpr uint32_t kMoveLanes = 16, kMoveThreads = 256, kMovePerBlock = kMoveThreads / kMoveLanes;

struct GatherMergedArgs {
  const tkv_amq_merge_item* items;
  const uint64_t* out_begin;
  uint32_t n_jobs;
  uint64_t max_out;  // min(out_capacity, the runs' items)
  MergeRun run[2];
  uint8_t* out_keys;
  uint32_t out_key_stride;
  uint64_t* key_offs;
  uint64_t keys_capacity;
  uint8_t* out_vals;
  uint64_t* val_offs;
  uint64_t vals_capacity;
  uint64_t* needed;  // [2], or null
  uint64_t* sums[2];  // the workspace: per workgroup of gather_measure the keys' and the values' bytes
};

// The same over a run table: a record's run is bits 56..63 of its src.
struct GatherLevelsArgs {
  const tkv_amq_merge_item* items;
  const uint64_t* out_begin;
  uint32_t n_jobs, n_runs;
  uint64_t max_out;
  MergeRun run[kLevelsMaxRuns];
  uint8_t* out_keys;
  uint32_t out_key_stride;
  uint64_t* key_offs;
  uint64_t keys_capacity;
  uint8_t* out_vals;
  uint64_t* val_offs;
  uint64_t vals_capacity;
  uint64_t* needed;
  uint64_t* sums[2];
};

__device__ inline uint64_t gather_n_out(const GatherMergedArgs& a) { return min(a.out_begin[a.n_jobs], a.max_out); }

// What record p gives: its key and its value where they lie, or (combined) the 5 bytes of a folded
// value; a record that is not trusted: neither.
struct MergedItem {
  const uint8_t *ksrc, *vsrc;
  uint64_t klen, vlen;
  uint32_t op, i32;
  bool combined;
};

__device__ inline MergedItem merged_item(const GatherMergedArgs& a, uint64_t p)
{
  const ulonglong2 rec = *reinterpret_cast<const ulonglong2*>(a.items + p);
  const MergeRun& r = a.run[rec.x >> 63];
  const uint64_t i = rec.x & ~(1ull << 63);
  MergedItem it{nullptr, nullptr, 0, 0, (uint32_t)(rec.y >> 32) & 0xffu, (uint32_t)rec.y, false};
  if (i >= r.n) return it;  // (the records are caller memory)
  uint32_t klen;
  r.keys.at(i, it.ksrc, klen);
  it.klen = klen;
  if ((rec.y >> 40) & TKV_AMQ_VALUE_COMBINED) {
    it.combined = true;
    it.vlen = 5;
  } else {
    uint64_t vb, ve;
    value_range(r.vals, i, vb, ve);
    it.vsrc = r.vals.values + vb;
    it.vlen = ve - vb;
  }
  return it;
}

// Per record the bytes before it inside its workgroup's span, into the offset arrays; the span's
// sums aside.  Spans past n_out write zero sums: the grid is sized from the capacity.
__global__ __launch_bounds__(kBlockScanThreads) void gather_measure(GatherMergedArgs a)
{
  __shared__ uint64_t s_waves[kBlockScanThreads / 64];
  const uint64_t n_out = gather_n_out(a);
  const uint64_t p0 = ((uint64_t)blockIdx.x * kBlockScanThreads + threadIdx.x) * kMeasurePerThread;
  uint64_t klen[kMeasurePerThread], vlen[kMeasurePerThread], ksum = 0, vsum = 0;
#pragma unroll
  for (uint32_t r = 0; r < kMeasurePerThread; ++r) {
    klen[r] = vlen[r] = 0;
    if (p0 + r < n_out) {
      const MergedItem it = merged_item(a, p0 + r);
      klen[r] = it.klen;
      vlen[r] = it.vlen;
    }
    ksum += klen[r];
    vsum += vlen[r];
  }
  uint64_t ktotal, vtotal;
  uint64_t krun = block_exclusive_scan<uint64_t>(ksum, s_waves, &ktotal);
  uint64_t vrun = block_exclusive_scan<uint64_t>(vsum, s_waves, &vtotal);
#pragma unroll
  for (uint32_t r = 0; r < kMeasurePerThread; ++r) {
    if (p0 + r < n_out) {
      if (a.key_offs) a.key_offs[p0 + r] = krun;
      a.val_offs[p0 + r] = vrun;
    }
    krun += klen[r];
    vrun += vlen[r];
  }
  if (threadIdx.x == 0) {
    a.sums[0][blockIdx.x] = ktotal;
    a.sums[1][blockIdx.x] = vtotal;
    if (blockIdx.x == 0 && n_out == 0) {
      if (a.key_offs) a.key_offs[0] = 0;
      a.val_offs[0] = 0;
    }
  }
}

// the fixed key form's total (the offsets form's comes from the scan of the sums)
__global__ void gather_fixed_needed(GatherMergedArgs a) { a.needed[0] = gather_n_out(a) * a.out_key_stride; }

// n bytes from src to dst by the sixteen lanes of an item, eight bytes per lane and step; a byte
// tail where the destination is not 8-byte aligned or fewer than eight bytes are left
__device__ inline void move_bytes(uint8_t* dst, const uint8_t* src, uint64_t n, uint32_t sub)
{
  for (uint64_t o = 8 * sub; o < n; o += 8 * kMoveLanes) {
    if (o + 8 <= n && (reinterpret_cast<uintptr_t>(dst + o) & 7) == 0) {
      *reinterpret_cast<uint64_t*>(dst + o) = ld64_unaligned(src + o);
    } else {
      const uint32_t m = n - o < 8 ? (uint32_t)(n - o) : 8u;
      for (uint32_t j = 0; j < m; ++j) dst[o + j] = src[o + j];
    }
  }
}

__global__ __launch_bounds__(kMoveThreads) void gather_move(GatherMergedArgs a)
{
  const uint64_t n_out = gather_n_out(a);
  const uint64_t p = (uint64_t)blockIdx.x * kMovePerBlock + threadIdx.x / kMoveLanes;
  const uint32_t sub = threadIdx.x % kMoveLanes;
  if (p >= n_out) return;
  const MergedItem it = merged_item(a, p);
  // (each offset word is read and written by its own record's lanes alone)
  const uint64_t vb = a.val_offs[p] + a.sums[1][p / kMeasureSpan];
  const uint64_t kb = a.key_offs ? a.key_offs[p] + a.sums[0][p / kMeasureSpan] : p * a.out_key_stride;
  if (sub == 0) {
    a.val_offs[p] = vb;
    if (a.key_offs) a.key_offs[p] = kb;
    if (p + 1 == n_out) {
      a.val_offs[n_out] = vb + it.vlen;
      if (a.key_offs) a.key_offs[n_out] = kb + it.klen;
    }
  }
  // the fixed form: a key of the slot's size or (an untrusted record) none
  const bool key_fits = a.key_offs ? kb + it.klen <= a.keys_capacity
                                   : it.klen == a.out_key_stride && kb + it.klen <= a.keys_capacity;
  if (key_fits) move_bytes(a.out_keys + kb, it.ksrc, it.klen, sub);
  if (vb + it.vlen > a.vals_capacity) return;
  if (!it.combined) {
    move_bytes(a.out_vals + vb, it.vsrc, it.vlen, sub);
  } else if (sub == 0) {
    // the folded value: the op byte and the integer, little-endian
    uint8_t* dst = a.out_vals + vb;
    dst[0] = (uint8_t)it.op;
    for (uint32_t j = 0; j < 4; ++j) dst[1 + j] = (uint8_t)(it.i32 >> (8 * j));
  }
}

// tkv_amq_gather_levels: the three kernels above over a run table.  They are kernels of their own, not
// instantiations of one template with those: sharing the bodies changed the code generated for
// tkv_amq_gather_merged.
__device__ inline uint64_t gather_n_out(const GatherLevelsArgs& a) { return min(a.out_begin[a.n_jobs], a.max_out); }

// a record's run is bits 56..63 of its src; one at or past n_runs is trusted no further than an index past its run
__device__ inline MergedItem merged_item(const GatherLevelsArgs& a, uint64_t p)
{
  const ulonglong2 rec = *reinterpret_cast<const ulonglong2*>(a.items + p);
  const uint32_t s = (uint32_t)(rec.x >> TKV_AMQ_LEVELS_SRC_SHIFT);
  const uint64_t i = rec.x & ((1ull << TKV_AMQ_LEVELS_SRC_SHIFT) - 1);
  MergedItem it{nullptr, nullptr, 0, 0, (uint32_t)(rec.y >> 32) & 0xffu, (uint32_t)rec.y, false};
  if (s >= a.n_runs) return it;
  const MergeRun& r = a.run[s];
  if (i >= r.n) return it;
  uint32_t klen;
  r.keys.at(i, it.ksrc, klen);
  it.klen = klen;
  if ((rec.y >> 40) & TKV_AMQ_VALUE_COMBINED) {
    it.combined = true;
    it.vlen = 5;
  } else {
    uint64_t vb, ve;
    value_range(r.vals, i, vb, ve);
    it.vsrc = r.vals.values + vb;
    it.vlen = ve - vb;
  }
  return it;
}

__global__ __launch_bounds__(kBlockScanThreads) void gather_levels_measure(GatherLevelsArgs a)
{
  __shared__ uint64_t s_waves[kBlockScanThreads / 64];
  const uint64_t n_out = gather_n_out(a);
  const uint64_t p0 = ((uint64_t)blockIdx.x * kBlockScanThreads + threadIdx.x) * kMeasurePerThread;
  uint64_t klen[kMeasurePerThread], vlen[kMeasurePerThread], ksum = 0, vsum = 0;
#pragma unroll
  for (uint32_t r = 0; r < kMeasurePerThread; ++r) {
    klen[r] = vlen[r] = 0;
    if (p0 + r < n_out) {
      const MergedItem it = merged_item(a, p0 + r);
      klen[r] = it.klen;
      vlen[r] = it.vlen;
    }
    ksum += klen[r];
    vsum += vlen[r];
  }
  uint64_t ktotal, vtotal;
  uint64_t krun = block_exclusive_scan<uint64_t>(ksum, s_waves, &ktotal);
  uint64_t vrun = block_exclusive_scan<uint64_t>(vsum, s_waves, &vtotal);
#pragma unroll
  for (uint32_t r = 0; r < kMeasurePerThread; ++r) {
    if (p0 + r < n_out) {
      if (a.key_offs) a.key_offs[p0 + r] = krun;
      a.val_offs[p0 + r] = vrun;
    }
    krun += klen[r];
    vrun += vlen[r];
  }
  if (threadIdx.x == 0) {
    a.sums[0][blockIdx.x] = ktotal;
    a.sums[1][blockIdx.x] = vtotal;
    if (blockIdx.x == 0 && n_out == 0) {
      if (a.key_offs) a.key_offs[0] = 0;
      a.val_offs[0] = 0;
    }
  }
}

__global__ void gather_levels_fixed_needed(GatherLevelsArgs a) { a.needed[0] = gather_n_out(a) * a.out_key_stride; }

__global__ __launch_bounds__(kMoveThreads) void gather_levels_move(GatherLevelsArgs a)
{
  const uint64_t n_out = gather_n_out(a);
  const uint64_t p = (uint64_t)blockIdx.x * kMovePerBlock + threadIdx.x / kMoveLanes;
  const uint32_t sub = threadIdx.x % kMoveLanes;
  if (p >= n_out) return;
  const MergedItem it = merged_item(a, p);
  // (each offset word is read and written by its own record's lanes alone)
  const uint64_t vb = a.val_offs[p] + a.sums[1][p / kMeasureSpan];
  const uint64_t kb = a.key_offs ? a.key_offs[p] + a.sums[0][p / kMeasureSpan] : p * a.out_key_stride;
  if (sub == 0) {
    a.val_offs[p] = vb;
    if (a.key_offs) a.key_offs[p] = kb;
    if (p + 1 == n_out) {
      a.val_offs[n_out] = vb + it.vlen;
      if (a.key_offs) a.key_offs[n_out] = kb + it.klen;
    }
  }
  // the fixed form: a key of the slot's size or (an untrusted record) none
  const bool key_fits = a.key_offs ? kb + it.klen <= a.keys_capacity
                                   : it.klen == a.out_key_stride && kb + it.klen <= a.keys_capacity;
  if (key_fits) move_bytes(a.out_keys + kb, it.ksrc, it.klen, sub);
  if (vb + it.vlen > a.vals_capacity) return;
  if (!it.combined) {
    move_bytes(a.out_vals + vb, it.vsrc, it.vlen, sub);
  } else if (sub == 0) {
    // the folded value: the op byte and the integer, little-endian
    uint8_t* dst = a.out_vals + vb;
    dst[0] = (uint8_t)it.op;
    for (uint32_t j = 0; j < 4; ++j) dst[1 + j] = (uint8_t)(it.i32 >> (8 * j));
  }
}

constexpr uint64_t kCountMax = 0xffffffffull;

inline bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// what both entry points ask of a run
inline bool run_ok(const tkv_amq_merge_run* r)
{
  if (!r || r->n_items > kCountMax) return false;
  if (r->n_items && (!r->keys || (r->values_bytes && !r->values))) return false;
  return (r->key_offsets || r->key_stride) && (r->value_offsets || r->value_stride);
}

// the same of a table of 1 .. TKV_AMQ_MERGE_MAX_RUNS runs; n_total: their items, at most kCountMax
inline bool runs_ok(const tkv_amq_merge_run* runs, uint32_t n_runs, uint64_t& n_total)
{
  n_total = 0;
  if (!runs || n_runs == 0 || n_runs > kLevelsMaxRuns) return false;
  for (uint32_t r = 0; r < n_runs; ++r) {
    if (!run_ok(runs + r)) return false;
    n_total += runs[r].n_items;
  }
  return n_total <= kCountMax;
}

inline uint64_t gather_spans(uint64_t max_out) { return div_up(max_out, kMeasureSpan) + 1; }

inline uint64_t gather_ws_bytes(uint64_t out_capacity)
{
  const uint64_t cap = out_capacity < kCountMax ? out_capacity : kCountMax;
  return kMergeWsHeader + 2 * round16(gather_spans(cap) * 8);
}

// what the two gathers take besides their runs
struct GatherOut {
  const tkv_amq_merge_item* items;
  const uint64_t* out_begin;
  uint64_t n_jobs, out_capacity;
  uint8_t* keys;
  uint32_t key_stride;
  uint64_t* key_offsets;
  uint64_t keys_capacity;
  uint8_t* values;
  uint64_t* value_offsets;
  uint64_t values_capacity;
  uint64_t* needed_bytes;
  void* workspace;
  uint64_t workspace_bytes;
  void* stream;
};

// Either gather: the argument checks, `a` filled in (Args: GatherMergedArgs or GatherLevelsArgs, with
// what only it has already set) and the chain of launches with that form's kernels.
template <class Args, class Measure, class FixedNeeded, class Move>
int gather_call(Args& a, const tkv_amq_merge_run* runs, uint32_t n_runs, const GatherOut& o, Measure measure,
                FixedNeeded fixed_needed, Move move)
{
  uint64_t n_items;
  if (!runs_ok(runs, n_runs, n_items) || !o.out_begin || !o.value_offsets || !o.workspace) return TKV_AMQ_INVALID_ARGUMENT;
  if (o.n_jobs > kCountMax) return TKV_AMQ_INVALID_ARGUMENT;
  if ((o.out_capacity && !o.items) || !aligned(o.items, 16) || !aligned(o.out_begin, 8)) return TKV_AMQ_INVALID_ARGUMENT;
  if (o.key_stride) {
    for (uint32_t r = 0; r < n_runs; ++r)
      if (runs[r].key_offsets || runs[r].key_stride != o.key_stride) return TKV_AMQ_INVALID_ARGUMENT;
  } else if (!o.key_offsets) {
    return TKV_AMQ_INVALID_ARGUMENT;
  }
  if ((o.keys_capacity && !o.keys) || (o.values_capacity && !o.values)) return TKV_AMQ_INVALID_ARGUMENT;
  if (!aligned(o.key_offsets, 8) || !aligned(o.value_offsets, 8) || !aligned(o.needed_bytes, 8))
    return TKV_AMQ_INVALID_ARGUMENT;
  if (!aligned(o.workspace, 16) || o.workspace_bytes < gather_ws_bytes(o.out_capacity)) return TKV_AMQ_INVALID_ARGUMENT;
  if (tkv_amq_device_count() == 0) return TKV_AMQ_UNAVAILABLE;
  const hipStream_t s = as_stream(o.stream);
  a.items = o.items;
  a.out_begin = o.out_begin;
  a.n_jobs = (uint32_t)o.n_jobs;
  a.max_out = o.out_capacity < n_items ? o.out_capacity : n_items;
  for (uint32_t r = 0; r < n_runs; ++r) a.run[r] = merge_run(runs[r]);
  a.out_keys = o.keys;
  a.out_key_stride = o.key_stride;
  a.key_offs = o.key_stride ? nullptr : o.key_offsets;
  a.keys_capacity = o.keys_capacity;
  a.out_vals = o.values;
  a.val_offs = o.value_offsets;
  a.vals_capacity = o.values_capacity;
  a.needed = o.needed_bytes;
  const uint32_t spans = (uint32_t)gather_spans(a.max_out);
  uint8_t* ws = static_cast<uint8_t*>(o.workspace) + kMergeWsHeader;
  a.sums[0] = reinterpret_cast<uint64_t*>(ws);
  a.sums[1] = reinterpret_cast<uint64_t*>(ws + (gather_ws_bytes(o.out_capacity) - kMergeWsHeader) / 2);
  hipLaunchKernelGGL(measure, dim3(spans), dim3(kBlockScanThreads), 0, s, a);
  if (a.key_offs)
    hipLaunchKernelGGL(scan_totals<uint64_t>, dim3(1), dim3(kBlockScanThreads), 0, s, a.sums[0], spans, nullptr, 0u,
                       o.needed_bytes);
  else if (o.needed_bytes)
    hipLaunchKernelGGL(fixed_needed, dim3(1), dim3(1), 0, s, a);
  hipLaunchKernelGGL(scan_totals<uint64_t>, dim3(1), dim3(kBlockScanThreads), 0, s, a.sums[1], spans, nullptr, 0u,
                     o.needed_bytes ? o.needed_bytes + 1 : nullptr);
  if (a.max_out)
    hipLaunchKernelGGL(move, dim3((uint32_t)div_up(a.max_out, kMovePerBlock)), dim3(kMoveThreads), 0, s, a);
  return hipGetLastError() == hipSuccess ? TKV_AMQ_OK : TKV_AMQ_INTERNAL;
}

}  // namespace
}  // namespace tkv

using namespace tkv;

extern "C" {

uint64_t tkv_amq_merge_leaves_ws_bytes(uint64_t n_jobs, uint64_t n_newer, uint64_t n_older)
{
  if (n_jobs > kCountMax || n_newer > kCountMax || n_older > kCountMax || n_newer + n_older > kCountMax) return 0;
  return merge_ws(nullptr, n_jobs, n_newer, n_older).bytes;
}

int tkv_amq_merge_leaves(const tkv_amq_merge_run* newer, const tkv_amq_merge_run* older, uint64_t n_jobs,
                         uint32_t flags, uint64_t* d_out_begin, tkv_amq_merge_item* d_items, uint64_t out_capacity,
                         uint64_t* d_needed, tkv_amq_merge_counts* d_counts, void* d_workspace,
                         uint64_t workspace_bytes, void* stream)
{
  // (the arguments are judged first, so a bad call is InvalidArgument with or without a device)
  if (flags & ~TKV_AMQ_MERGE_DECAY_TO_ITEMS) return TKV_AMQ_INVALID_ARGUMENT;
  if (!run_ok(newer) || !run_ok(older) || !d_out_begin) return TKV_AMQ_INVALID_ARGUMENT;
  if (n_jobs > kCountMax || newer->n_items + older->n_items > kCountMax) return TKV_AMQ_INVALID_ARGUMENT;
  if ((out_capacity && !d_items) || !aligned(d_items, 16) || !aligned(d_needed, 8) || !aligned(d_counts, 8) ||
      !aligned(d_out_begin, 8))
    return TKV_AMQ_INVALID_ARGUMENT;
  if (n_jobs) {
    if (!newer->d_begin || !older->d_begin || !d_workspace || !aligned(d_workspace, 16)) return TKV_AMQ_INVALID_ARGUMENT;
    if (workspace_bytes < tkv_amq_merge_leaves_ws_bytes(n_jobs, newer->n_items, older->n_items))
      return TKV_AMQ_INVALID_ARGUMENT;
  }
  if (tkv_amq_device_count() == 0) return TKV_AMQ_UNAVAILABLE;
  const hipStream_t s = as_stream(stream);
  MergeArgs a;
  a.run[0] = merge_run(*newer);
  a.run[1] = merge_run(*older);
  a.n_jobs = (uint32_t)n_jobs;
  a.chunk = merge_chunk(newer->n_items + older->n_items);
  a.decay = flags & TKV_AMQ_MERGE_DECAY_TO_ITEMS;
  a.out_begin = d_out_begin;
  a.items = d_items;
  a.out_capacity = out_capacity;
  a.needed = d_needed;
  a.counts = d_counts;
  if (n_jobs == 0) {
    a.ws = MergeWs{};
    hipLaunchKernelGGL(merge_offsets, dim3(1), dim3(kBlockScanThreads), 0, s, a);
    return hipGetLastError() == hipSuccess ? TKV_AMQ_OK : TKV_AMQ_INTERNAL;
  }
  a.ws = merge_ws(d_workspace, n_jobs, newer->n_items, older->n_items);
  const uint64_t units = merge_max_units(n_jobs, newer->n_items + older->n_items);
  const dim3 grid((uint32_t)(units < kMergeMaxGrid ? units : kMergeMaxGrid)), block(kMergeThreads);
  const int order = key_order_mode(a.run[0].keys, a.run[1].keys);
  hipLaunchKernelGGL(merge_plan, dim3(1), dim3(kBlockScanThreads), 0, s, a);
  if (order == kOrder16) hipLaunchKernelGGL(merge_rank<kOrder16>, grid, block, 0, s, a);
  else if (order == kOrder24) hipLaunchKernelGGL(merge_rank<kOrder24>, grid, block, 0, s, a);
  else hipLaunchKernelGGL(merge_rank<kOrderAny>, grid, block, 0, s, a);
  hipLaunchKernelGGL(merge_offsets, dim3(1), dim3(kBlockScanThreads), 0, s, a);
  if (order == kOrder16) hipLaunchKernelGGL(merge_emit<kOrder16>, grid, block, 0, s, a);
  else if (order == kOrder24) hipLaunchKernelGGL(merge_emit<kOrder24>, grid, block, 0, s, a);
  else hipLaunchKernelGGL(merge_emit<kOrderAny>, grid, block, 0, s, a);
  return hipGetLastError() == hipSuccess ? TKV_AMQ_OK : TKV_AMQ_INTERNAL;
}

uint64_t tkv_amq_merge_values_bound(uint64_t newer_bytes, uint64_t older_bytes, uint64_t n_newer)
{
  return newer_bytes + older_bytes + 4 * n_newer;
}

uint64_t tkv_amq_gather_merged_ws_bytes(uint64_t out_capacity) { return gather_ws_bytes(out_capacity); }

int tkv_amq_gather_merged(const tkv_amq_merge_item* d_items, const uint64_t* d_out_begin, uint64_t n_jobs,
                          uint64_t out_capacity, const tkv_amq_merge_run* newer, const tkv_amq_merge_run* older,
                          uint8_t* d_out_keys, uint32_t out_key_stride, uint64_t* d_out_key_offsets,
                          uint64_t out_keys_capacity, uint8_t* d_out_values, uint64_t* d_out_value_offsets,
                          uint64_t out_values_capacity, uint64_t* d_needed_bytes, void* d_workspace,
                          uint64_t workspace_bytes, void* stream)
{
  if (!newer || !older) return TKV_AMQ_INVALID_ARGUMENT;
  const tkv_amq_merge_run runs[2] = {*newer, *older};
  GatherMergedArgs a;
  return gather_call(a, runs, 2, GatherOut{d_items, d_out_begin, n_jobs, out_capacity, d_out_keys, out_key_stride,
                                           d_out_key_offsets, out_keys_capacity, d_out_values, d_out_value_offsets,
                                           out_values_capacity, d_needed_bytes, d_workspace, workspace_bytes, stream},
                     gather_measure, gather_fixed_needed, gather_move);
}

uint64_t tkv_amq_merge_levels_ws_bytes(uint64_t n_jobs, uint32_t n_runs, uint64_t n_items_total)
{
  if (n_runs == 0 || n_runs > kLevelsMaxRuns || n_jobs > kCountMax || n_items_total > kCountMax) return 0;
  return levels_ws(nullptr, n_jobs, n_runs, n_items_total).bytes;
}

int tkv_amq_merge_levels(const tkv_amq_merge_run* runs, uint32_t n_runs, uint64_t n_jobs, uint32_t flags,
                         uint64_t* d_out_begin, tkv_amq_merge_item* d_items, uint64_t out_capacity,
                         uint64_t* d_needed, tkv_amq_merge_counts* d_counts, void* d_workspace,
                         uint64_t workspace_bytes, void* stream)
{
  // (the arguments are judged first, so a bad call is InvalidArgument with or without a device)
  if (flags & ~TKV_AMQ_MERGE_DECAY_TO_ITEMS) return TKV_AMQ_INVALID_ARGUMENT;
  uint64_t n_total;
  if (!runs_ok(runs, n_runs, n_total) || n_jobs > kCountMax || !d_out_begin) return TKV_AMQ_INVALID_ARGUMENT;
  if ((out_capacity && !d_items) || !aligned(d_items, 16) || !aligned(d_needed, 8) || !aligned(d_counts, 8) ||
      !aligned(d_out_begin, 8))
    return TKV_AMQ_INVALID_ARGUMENT;
  if (n_jobs) {
    for (uint32_t r = 0; r < n_runs; ++r)
      if (!runs[r].d_begin) return TKV_AMQ_INVALID_ARGUMENT;
    if (!d_workspace || !aligned(d_workspace, 16)) return TKV_AMQ_INVALID_ARGUMENT;
    if (workspace_bytes < tkv_amq_merge_levels_ws_bytes(n_jobs, n_runs, n_total)) return TKV_AMQ_INVALID_ARGUMENT;
  }
  if (tkv_amq_device_count() == 0) return TKV_AMQ_UNAVAILABLE;
  const hipStream_t s = as_stream(stream);
  // merge_offsets reads of its arguments the job count, upre, kept and the outputs alone
  MergeArgs o{};
  o.n_jobs = (uint32_t)n_jobs;
  o.out_begin = d_out_begin;
  o.needed = d_needed;
  o.counts = d_counts;
  if (n_jobs == 0) {
    hipLaunchKernelGGL(merge_offsets, dim3(1), dim3(kBlockScanThreads), 0, s, o);
    return hipGetLastError() == hipSuccess ? TKV_AMQ_OK : TKV_AMQ_INTERNAL;
  }
  LevelsArgs a{};
  KeyArray keys[kLevelsMaxRuns];
  uint64_t before = 0;
  for (uint32_t r = 0; r < n_runs; ++r) {
    a.run[r] = merge_run(runs[r]);
    a.ibase[r] = before;
    keys[r] = a.run[r].keys;
    before += runs[r].n_items;
  }
  a.ws = levels_ws(d_workspace, n_jobs, n_runs, n_total);
  a.n_total = n_total;
  a.n_runs = n_runs;
  a.n_jobs = (uint32_t)n_jobs;
  a.chunk = merge_chunk(n_total);
  a.decay = flags & TKV_AMQ_MERGE_DECAY_TO_ITEMS;
  a.items = d_items;
  a.out_capacity = out_capacity;
  o.ws.upre = a.ws.upre;
  o.ws.kept = a.ws.kept;
  const uint64_t units = levels_max_units(n_jobs, n_runs, n_total);
  const dim3 grid((uint32_t)(units < kMergeMaxGrid ? units : kMergeMaxGrid)), block(kMergeThreads);
  const int order = key_order_mode(keys, n_runs);
  hipLaunchKernelGGL(levels_plan, dim3(1), dim3(kBlockScanThreads), 0, s, a);
  if (order == kOrder16) hipLaunchKernelGGL(levels_rank<kOrder16>, grid, block, 0, s, a, d_counts);
  else if (order == kOrder24) hipLaunchKernelGGL(levels_rank<kOrder24>, grid, block, 0, s, a, d_counts);
  else hipLaunchKernelGGL(levels_rank<kOrderAny>, grid, block, 0, s, a, d_counts);
  hipLaunchKernelGGL(merge_offsets, dim3(1), dim3(kBlockScanThreads), 0, s, o);
  hipLaunchKernelGGL(levels_emit, grid, block, 0, s, a);
  return hipGetLastError() == hipSuccess ? TKV_AMQ_OK : TKV_AMQ_INTERNAL;
}

uint64_t tkv_amq_merge_levels_values_bound(uint64_t values_bytes_total, uint64_t n_items_not_in_oldest_run)
{
  return values_bytes_total + 4 * n_items_not_in_oldest_run;
}

uint64_t tkv_amq_gather_levels_ws_bytes(uint64_t out_capacity) { return gather_ws_bytes(out_capacity); }

int tkv_amq_gather_levels(const tkv_amq_merge_item* d_items, const uint64_t* d_out_begin, uint64_t n_jobs,
                          uint64_t out_capacity, const tkv_amq_merge_run* runs, uint32_t n_runs,
                          uint8_t* d_out_keys, uint32_t out_key_stride, uint64_t* d_out_key_offsets,
                          uint64_t out_keys_capacity, uint8_t* d_out_values, uint64_t* d_out_value_offsets,
                          uint64_t out_values_capacity, uint64_t* d_needed_bytes, void* d_workspace,
                          uint64_t workspace_bytes, void* stream)
{
  GatherLevelsArgs a{};
  a.n_runs = n_runs;
  return gather_call(a, runs, n_runs, GatherOut{d_items, d_out_begin, n_jobs, out_capacity, d_out_keys, out_key_stride,
                                                d_out_key_offsets, out_keys_capacity, d_out_values, d_out_value_offsets,
                                                out_values_capacity, d_needed_bytes, d_workspace, workspace_bytes, stream},
                     gather_levels_measure, gather_levels_fixed_needed, gather_levels_move);
}

}  // extern "C"
