// merge_levels of the header-only host mirror (include/turtle_kv_amd/filter_builder.hpp) and the K-way merge entry
// points of libtkv_amq.so.  With or without a device: the layouts the entry points share with the leaf merge, the
// host functions' values, the argument checks of both entry points (a bad call is InvalidArgument, judged before a
// device is looked for) and of the mirror.  On the GPU merge_levels over two jobs of five levels of 16-byte keys must
// equal a cascade of std::merge (each stable, the newer level first) followed by the compaction loop, written here
// from include/tkv_amq.h: records' bytes, ranges and counts, with and without decay, for every run count from 1 to 5.
// Exits non-zero on any failed expectation; without a device prints NODEVICE-OK.
#include <turtle_kv_amd/filter_builder.hpp>

#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

using namespace turtle_kv_amd;

static int failures = 0;
#define EXPECT(c)                                                   \
  do {                                                              \
    if (!(c)) {                                                     \
      std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      ++failures;                                                   \
    }                                                               \
  } while (0)

static std::string key(u32 i)
{
  std::string k(16, '\x40');
  for (int b = 0; b < 4; ++b) k[12 + b] = (char)(i >> (24 - 8 * b));
  return k;
}

// a packed value: the op byte and a 4-byte integer
static std::string val(u32 op, int32_t x)
{
  std::string v(1, (char)op);
  for (int b = 0; b < 4; ++b) v.push_back((char)((u32)x >> (8 * b)));
  return v;
}

static int32_t int_of(const std::string& v)
{
  u32 x = 0;
  for (int b = 0; b < 4; ++b) x |= (u32)(u8)v[1 + b] << (8 * b);
  return (int32_t)x;
}

struct Item {
  std::string key, value;
};

// The levels merged pairwise by std::merge, the newest first (each merge stable with the newer side first among
// equals, so a group of equal keys stays in level order), then the compaction loop: the first item of a group
// stands and is folded with the ones behind it while it is an ADD_I32; with decay DELETE and NOOP go.
static std::vector<Item> merge_host(const std::vector<std::vector<Item>>& levels, bool decay, tkv_amq_merge_counts& c)
{
  std::vector<Item> all;
  for (usize s = 0; s < levels.size(); ++s) {
    std::vector<Item> next(all.size() + levels[s].size());
    std::merge(all.begin(), all.end(), levels[s].begin(), levels[s].end(), next.begin(),
               [](const Item& a, const Item& b) { return a.key < b.key; });
    all.swap(next);
    (s == 0 ? c.newer_count : c.older_count) += levels[s].size();
  }
  std::vector<Item> out;
  for (usize i = 0; i < all.size();) {
    usize e = i + 1;
    while (e < all.size() && all[e].key == all[i].key) ++e;
    Item it = all[i];
    c.pair_count += e - i - 1;
    bool combined = false;
    for (usize p = i + 1; p < e && (u8)it.value[0] == TKV_AMQ_OP_ADD_I32; ++p) {
      const u32 older_op = (u8)all[p].value[0];
      const u32 a = (u32)int_of(it.value), b = (u32)int_of(all[p].value);
      if (older_op == TKV_AMQ_OP_WRITE) it.value = val(TKV_AMQ_OP_WRITE, (int32_t)(a + b));
      else if (older_op == TKV_AMQ_OP_DELETE) it.value = val(TKV_AMQ_OP_WRITE, (int32_t)a);
      else if (older_op == TKV_AMQ_OP_ADD_I32) it.value = val(TKV_AMQ_OP_ADD_I32, (int32_t)(a + b));
      if (older_op == TKV_AMQ_OP_WRITE || older_op == TKV_AMQ_OP_DELETE || older_op == TKV_AMQ_OP_ADD_I32) combined = true;
      else ++c.bad_combine_count;
    }
    c.combined_count += combined;
    const u32 op = (u8)it.value[0];
    if (decay && (op == TKV_AMQ_OP_DELETE || op == TKV_AMQ_OP_NOOP)) ++c.dropped_count;
    else out.push_back(it);
    i = e;
  }
  c.out_count += out.size();
  return out;
}

static void check_layouts()
{
  EXPECT(sizeof(tkv_amq_merge_item) == 16 && sizeof(tkv_amq_merge_counts) == 56 && sizeof(tkv_amq_merge_run) == 64);
  EXPECT(TKV_AMQ_MERGE_MAX_RUNS == 8u && TKV_AMQ_LEVELS_SRC_SHIFT == 56 && TKV_AMQ_ABI_VERSION == 3);
  EXPECT(tkv_amq_merge_levels_ws_bytes(0, 1, 0) >= 16 && tkv_amq_gather_levels_ws_bytes(0) >= 16);
  EXPECT(tkv_amq_merge_levels_ws_bytes(1, 0, 1) == 0 && tkv_amq_merge_levels_ws_bytes(1, 9, 1) == 0);
  EXPECT(tkv_amq_merge_levels_ws_bytes(1, 2, u64{1} << 32) == 0 && tkv_amq_merge_levels_ws_bytes(u64{1} << 32, 2, 1) == 0);
  EXPECT(tkv_amq_merge_levels_ws_bytes(3, 4, 1000) >= tkv_amq_merge_levels_ws_bytes(3, 4, 999));
  EXPECT(tkv_amq_merge_levels_ws_bytes(3, 5, 1000) >= tkv_amq_merge_levels_ws_bytes(3, 4, 1000));
  EXPECT(tkv_amq_merge_levels_ws_bytes(4, 4, 1000) >= tkv_amq_merge_levels_ws_bytes(3, 4, 1000));
  EXPECT(tkv_amq_merge_levels_values_bound(30, 3) == 42 && tkv_amq_merge_levels_values_bound(0, 0) == 0);
}

// the argument checks: `some` stands for every buffer (nothing is read before a device is looked for, so the
// calls that pass the checks are made only without one)
static void check_arguments(bool no_device)
{
  alignas(16) static u8 some[8192] = {};
  const u64* begin = reinterpret_cast<const u64*>(some);
  const tkv_amq_merge_run run{some, nullptr, some, nullptr, begin, 10, 50, 16, 5};
  std::vector<tkv_amq_merge_run> runs(9, run);
  auto merge = [&](const tkv_amq_merge_run* r, u32 n_runs, u32 flags, u32 items_off, u64 ws_bytes) {
    return tkv_amq_merge_levels(r, n_runs, 2, flags, reinterpret_cast<u64*>(some),
                                reinterpret_cast<tkv_amq_merge_item*>(some + items_off), 80, nullptr, nullptr, some,
                                ws_bytes, nullptr);
  };
  const u64 ws = tkv_amq_merge_levels_ws_bytes(2, 8, 80);
  EXPECT(ws <= sizeof(some));
  if (no_device) {
    for (u32 k = 1; k <= 8; ++k) EXPECT(merge(runs.data(), k, 0, 0, ws) == TKV_AMQ_UNAVAILABLE);
    EXPECT(merge(runs.data(), 3, TKV_AMQ_MERGE_DECAY_TO_ITEMS, 16, ws) == TKV_AMQ_UNAVAILABLE);
  }
  EXPECT(merge(runs.data(), 0, 0, 0, ws) == TKV_AMQ_INVALID_ARGUMENT);
  EXPECT(merge(runs.data(), 9, 0, 0, ws) == TKV_AMQ_INVALID_ARGUMENT);
  EXPECT(merge(nullptr, 3, 0, 0, ws) == TKV_AMQ_INVALID_ARGUMENT);
  EXPECT(merge(runs.data(), 3, 2, 0, ws) == TKV_AMQ_INVALID_ARGUMENT);
  EXPECT(merge(runs.data(), 3, 0, 8, ws) == TKV_AMQ_INVALID_ARGUMENT);
  EXPECT(merge(runs.data(), 3, 0, 0, tkv_amq_merge_levels_ws_bytes(2, 3, 30) - 1) == TKV_AMQ_INVALID_ARGUMENT);
  for (u32 s = 0; s < 4; ++s) {  // every run is checked
    auto with = [&](auto change) {
      std::vector<tkv_amq_merge_run> t(4, run);
      change(t[s]);
      return merge(t.data(), 4, 0, 0, ws);
    };
    EXPECT(with([](tkv_amq_merge_run& r) { r.key_stride = 0; }) == TKV_AMQ_INVALID_ARGUMENT);
    EXPECT(with([](tkv_amq_merge_run& r) { r.value_stride = 0; }) == TKV_AMQ_INVALID_ARGUMENT);
    EXPECT(with([](tkv_amq_merge_run& r) { r.keys = nullptr; }) == TKV_AMQ_INVALID_ARGUMENT);
    EXPECT(with([](tkv_amq_merge_run& r) { r.values = nullptr; }) == TKV_AMQ_INVALID_ARGUMENT);
    EXPECT(with([](tkv_amq_merge_run& r) { r.d_begin = nullptr; }) == TKV_AMQ_INVALID_ARGUMENT);
    EXPECT(with([](tkv_amq_merge_run& r) { r.n_items = u64{1} << 32; }) == TKV_AMQ_INVALID_ARGUMENT);
    EXPECT(with([](tkv_amq_merge_run& r) { r.n_items = 0xfffffff0u; }) == TKV_AMQ_INVALID_ARGUMENT);  // the sum
  }
  auto gather = [&](const tkv_amq_merge_run* r, u32 n_runs, u32 out_key_stride, u64* key_offsets, u64 gws) {
    return tkv_amq_gather_levels(reinterpret_cast<const tkv_amq_merge_item*>(some), begin, 2, 80, r, n_runs, some,
                                 out_key_stride, key_offsets, 1280, some, reinterpret_cast<u64*>(some), 400, nullptr,
                                 some, gws, nullptr);
  };
  const u64 gws = tkv_amq_gather_levels_ws_bytes(80);
  if (no_device) {
    EXPECT(gather(runs.data(), 3, 16, nullptr, gws) == TKV_AMQ_UNAVAILABLE);
    EXPECT(gather(runs.data(), 8, 0, reinterpret_cast<u64*>(some), gws) == TKV_AMQ_UNAVAILABLE);
  }
  EXPECT(gather(runs.data(), 0, 16, nullptr, gws) == TKV_AMQ_INVALID_ARGUMENT);
  EXPECT(gather(runs.data(), 9, 16, nullptr, gws) == TKV_AMQ_INVALID_ARGUMENT);
  EXPECT(gather(nullptr, 3, 16, nullptr, gws) == TKV_AMQ_INVALID_ARGUMENT);
  EXPECT(gather(runs.data(), 3, 24, nullptr, gws) == TKV_AMQ_INVALID_ARGUMENT);  // not the runs' stride
  EXPECT(gather(runs.data(), 3, 0, nullptr, gws) == TKV_AMQ_INVALID_ARGUMENT);
  EXPECT(gather(runs.data(), 3, 16, nullptr, gws - 1) == TKV_AMQ_INVALID_ARGUMENT);
  std::vector<tkv_amq_merge_run> mixed(3, run);
  mixed[2].key_stride = 24;
  EXPECT(gather(mixed.data(), 3, 16, nullptr, gws) == TKV_AMQ_INVALID_ARGUMENT);  // fixed slots: every run that stride
  // the mirror: run counts and item counts the entry point refuses, a stride of 0
  MergedLeaves out;
  EXPECT(merge_levels(runs.data(), 0, 2, false, out).code == TKV_AMQ_INVALID_ARGUMENT);
  EXPECT(merge_levels(runs.data(), 9, 2, false, out).code == TKV_AMQ_INVALID_ARGUMENT);
  EXPECT(merge_levels(nullptr, 2, 2, false, out).code == TKV_AMQ_INVALID_ARGUMENT);
  std::vector<tkv_amq_merge_run> t(3, run);
  t[1].n_items = u64{1} << 32;
  EXPECT(merge_levels(t.data(), 3, 2, false, out).code == TKV_AMQ_INVALID_ARGUMENT);
  t[1] = run;
  t[2].value_stride = 0;
  EXPECT(merge_levels(t.data(), 3, 2, false, out).code == TKV_AMQ_INVALID_ARGUMENT);
  EXPECT(out.begin.size() == 1 && out.n_items == 0);
}

// one level on the device: 16-byte keys in the fixed form, values in the offsets form
struct DeviceRun {
  DeviceBuffer keys, values, value_offsets, begin;
  tkv_amq_merge_run run{};
  void upload(const std::vector<std::vector<Item>>& jobs)
  {
    std::string kblob, vblob;
    std::vector<u64> voffs{0}, b{0};
    for (const auto& job : jobs) {
      for (const auto& it : job) {
        kblob += it.key;
        vblob += it.value;
        voffs.push_back(vblob.size());
      }
      b.push_back(voffs.size() - 1);
    }
    EXPECT(keys.resize(kblob.size()) && values.resize(vblob.size()) && value_offsets.resize(8 * voffs.size()) &&
           begin.resize(8 * b.size()));
    EXPECT(hipMemcpy(keys.get(), kblob.data(), kblob.size(), hipMemcpyHostToDevice) == hipSuccess);
    EXPECT(hipMemcpy(values.get(), vblob.data(), vblob.size(), hipMemcpyHostToDevice) == hipSuccess);
    EXPECT(hipMemcpy(value_offsets.get(), voffs.data(), 8 * voffs.size(), hipMemcpyHostToDevice) == hipSuccess);
    EXPECT(hipMemcpy(begin.get(), b.data(), 8 * b.size(), hipMemcpyHostToDevice) == hipSuccess);
    run = tkv_amq_merge_run{keys.get(), nullptr, values.get(), value_offsets.get<u64>(), begin.get<u64>(),
                            voffs.size() - 1, vblob.size(), 16, 0};
  }
};

int main()
{
  check_layouts();
  if (tkv_amq_device_count() == 0) {
    check_arguments(true);
    MergedLeaves out;
    alignas(16) static u8 some[64] = {};
    const tkv_amq_merge_run run{some, nullptr, some, nullptr, reinterpret_cast<const u64*>(some), 1, 5, 16, 5};
    const tkv_amq_merge_run three[3] = {run, run, run};
    EXPECT(merge_levels(three, 3, 1, false, out).code == TKV_AMQ_UNAVAILABLE);
    std::printf("%s (no device; %d failures)\n", failures ? "FAIL" : "NODEVICE-OK", failures);
    return failures ? 1 : 0;
  }

  // five levels over two jobs: key i is in level s by a rule of its own per level, so groups of one to five items
  // occur; more than half the values are deltas, so folds of three and more occur
  constexpr u32 kLevels = 5;
  const u32 ops[7] = {TKV_AMQ_OP_ADD_I32, TKV_AMQ_OP_WRITE,   TKV_AMQ_OP_ADD_I32,   TKV_AMQ_OP_DELETE,
                      TKV_AMQ_OP_ADD_I32, TKV_AMQ_OP_ADD_I32, TKV_AMQ_OP_PAGE_SLICE};
  const u32 mod[kLevels] = {2, 3, 5, 7, 4}, rest[kLevels] = {0, 1, 2, 3, 0};
  std::vector<std::vector<std::vector<Item>>> levels(kLevels, std::vector<std::vector<Item>>(2));  // [level][job]
  for (u32 s = 0; s < kLevels; ++s)
    for (u32 j = 0; j < 2; ++j)
      for (u32 i = 0; i < 900; ++i)
        if (i % mod[s] != rest[s] || i % 11 == s)
          levels[s][j].push_back(Item{key(1000 * j + i), val(ops[(i / (s + 1) + s) % 7], (int32_t)(0x7ffffff0u + 9 * s + i % 32))});
  std::vector<DeviceRun> dev(kLevels);
  for (u32 s = 0; s < kLevels; ++s) dev[s].upload(levels[s]);
  for (u32 n_runs = 1; n_runs <= kLevels; ++n_runs) {
    std::vector<tkv_amq_merge_run> runs;
    for (u32 s = 0; s < n_runs; ++s) runs.push_back(dev[s].run);
    for (bool decay : {false, true}) {
      tkv_amq_merge_counts wc{};
      std::vector<Item> want;
      std::vector<u64> begin{0};
      for (u32 j = 0; j < 2; ++j) {
        std::vector<std::vector<Item>> job;
        for (u32 s = 0; s < n_runs; ++s) job.push_back(levels[s][j]);
        const std::vector<Item> m = merge_host(job, decay, wc);
        want.insert(want.end(), m.begin(), m.end());
        begin.push_back(want.size());
      }
      if (n_runs >= 3)
        EXPECT(wc.pair_count > 500 && wc.combined_count > 100 && wc.bad_combine_count > 0 && (!decay || wc.dropped_count > 20));
      MergedLeaves out;
      const Status s = merge_levels(runs.data(), n_runs, 2, decay, out);
      EXPECT(s.ok());
      EXPECT(out.begin == begin && out.n_items == want.size() && out.key_stride == 16 && out.key_bytes == 16 * want.size());
      EXPECT(std::memcmp(&out.counts, &wc, sizeof(wc)) == 0);
      std::string kblob, vblob;
      std::vector<u64> voffs{0};
      for (const auto& it : want) {
        kblob += it.key;
        vblob += it.value;
        voffs.push_back(vblob.size());
      }
      EXPECT(out.value_bytes == vblob.size());
      std::string gk(kblob.size(), 0), gv(vblob.size(), 0);
      std::vector<u64> go(voffs.size());
      if (failures == 0) {
        EXPECT(hipMemcpy(gk.data(), out.keys.get(), gk.size(), hipMemcpyDeviceToHost) == hipSuccess);
        EXPECT(hipMemcpy(gv.data(), out.values.get(), gv.size(), hipMemcpyDeviceToHost) == hipSuccess);
        EXPECT(hipMemcpy(go.data(), out.value_offsets.get(), 8 * go.size(), hipMemcpyDeviceToHost) == hipSuccess);
        EXPECT(gk == kblob && gv == vblob && go == voffs);
      }
    }
  }
  check_arguments(false);
  std::printf("%s (%d failures)\n", failures ? "FAIL" : "OK", failures);
  return failures ? 1 : 0;
}
