// merge_leaves of the header-only host mirror (include/turtle_kv_amd/filter_builder.hpp) and the merge entry
// points of libtkv_amq.so.  With or without a device: the layouts of tkv_amq_merge_run, tkv_amq_merge_item and
// tkv_amq_merge_counts, the host functions' values, the argument checks of both entry points (a bad call is
// InvalidArgument, judged before a device is looked for) and of the mirror.  On the GPU merge_leaves over two jobs
// of 16-byte keys must equal std::merge followed by the compaction loop, written here from include/tkv_amq.h:
// records' bytes, ranges and counts, with and without decay.  Exits non-zero on any failed expectation; without a
// device prints NODEVICE-OK.
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

// std::merge (stable: the newer run first among equals), then the compaction loop: the first item of a group of
// equal keys stands, an ADD_I32 is folded with the one behind it, and with decay DELETE and NOOP go
static std::vector<Item> merge_host(const std::vector<Item>& newer, const std::vector<Item>& older, bool decay,
                                    tkv_amq_merge_counts& c)
{
  std::vector<Item> all(newer.size() + older.size()), out;
  std::merge(newer.begin(), newer.end(), older.begin(), older.end(), all.begin(),
             [](const Item& a, const Item& b) { return a.key < b.key; });
  c.newer_count += newer.size();
  c.older_count += older.size();
  for (usize i = 0; i < all.size();) {
    usize e = i + 1;
    while (e < all.size() && all[e].key == all[i].key) ++e;
    Item it = all[i];
    c.pair_count += e - i - 1;
    if (e - i > 1 && (u8)it.value[0] == TKV_AMQ_OP_ADD_I32) {
      const u32 older_op = (u8)all[i + 1].value[0];
      const u32 a = (u32)int_of(it.value), b = (u32)int_of(all[i + 1].value);
      if (older_op == TKV_AMQ_OP_WRITE) it.value = val(TKV_AMQ_OP_WRITE, (int32_t)(a + b));
      else if (older_op == TKV_AMQ_OP_DELETE) it.value = val(TKV_AMQ_OP_WRITE, (int32_t)a);
      else if (older_op == TKV_AMQ_OP_ADD_I32) it.value = val(TKV_AMQ_OP_ADD_I32, (int32_t)(a + b));
      if (older_op == TKV_AMQ_OP_WRITE || older_op == TKV_AMQ_OP_DELETE || older_op == TKV_AMQ_OP_ADD_I32) ++c.combined_count;
      else ++c.bad_combine_count;
    }
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
  EXPECT(sizeof(tkv_amq_merge_item) == 16 && offsetof(tkv_amq_merge_item, i32) == 8);
  EXPECT(offsetof(tkv_amq_merge_item, op) == 12 && offsetof(tkv_amq_merge_item, flags) == 13);
  EXPECT(offsetof(tkv_amq_merge_item, reserved) == 14);
  EXPECT(sizeof(tkv_amq_merge_counts) == 56 && offsetof(tkv_amq_merge_counts, out_count) == 48);
  EXPECT(sizeof(tkv_amq_merge_run) == 64 && offsetof(tkv_amq_merge_run, d_begin) == 32);
  EXPECT(offsetof(tkv_amq_merge_run, n_items) == 40 && offsetof(tkv_amq_merge_run, key_stride) == 56);
  EXPECT(offsetof(tkv_amq_merge_run, value_stride) == 60);
  EXPECT(tkv_amq_merge_leaves_ws_bytes(0, 0, 0) >= 16 && tkv_amq_gather_merged_ws_bytes(0) >= 16);
  EXPECT(tkv_amq_merge_leaves_ws_bytes(1, u64{1} << 32, 0) == 0);
  EXPECT(tkv_amq_merge_leaves_ws_bytes(3, 100, 1000) >= tkv_amq_merge_leaves_ws_bytes(3, 100, 999));
  EXPECT(tkv_amq_merge_values_bound(10, 20, 3) == 42);
}

// the argument checks: `some` stands for every buffer (nothing is read before a device is looked for, so the
// calls that pass the checks are made only without one)
static void check_arguments(bool no_device)
{
  alignas(16) static u8 some[4096] = {};
  const u64* begin = reinterpret_cast<const u64*>(some);
  const tkv_amq_merge_run run{some, nullptr, some, nullptr, begin, 10, 50, 16, 5};
  auto merge = [&](const tkv_amq_merge_run* n, const tkv_amq_merge_run* o, u32 flags, u32 items_off, u64 ws_bytes) {
    return tkv_amq_merge_leaves(n, o, 2, flags, reinterpret_cast<u64*>(some), reinterpret_cast<tkv_amq_merge_item*>(some + items_off),
                                20, nullptr, nullptr, some, ws_bytes, nullptr);
  };
  const u64 ws = tkv_amq_merge_leaves_ws_bytes(2, 10, 10);
  EXPECT(ws <= sizeof(some));
  if (no_device) {
    EXPECT(merge(&run, &run, 0, 0, ws) == TKV_AMQ_UNAVAILABLE);
    EXPECT(merge(&run, &run, TKV_AMQ_MERGE_DECAY_TO_ITEMS, 16, ws) == TKV_AMQ_UNAVAILABLE);
  }
  EXPECT(merge(&run, &run, 2, 0, ws) == TKV_AMQ_INVALID_ARGUMENT);
  EXPECT(merge(nullptr, &run, 0, 0, ws) == TKV_AMQ_INVALID_ARGUMENT);
  EXPECT(merge(&run, &run, 0, 8, ws) == TKV_AMQ_INVALID_ARGUMENT);
  EXPECT(merge(&run, &run, 0, 0, ws - 1) == TKV_AMQ_INVALID_ARGUMENT);
  tkv_amq_merge_run bad = run;
  bad.key_stride = 0;
  EXPECT(merge(&bad, &run, 0, 0, ws) == TKV_AMQ_INVALID_ARGUMENT);
  bad = run;
  bad.value_stride = 0;
  EXPECT(merge(&run, &bad, 0, 0, ws) == TKV_AMQ_INVALID_ARGUMENT);
  bad = run;
  bad.keys = nullptr;
  EXPECT(merge(&bad, &run, 0, 0, ws) == TKV_AMQ_INVALID_ARGUMENT);
  bad = run;
  bad.d_begin = nullptr;
  EXPECT(merge(&run, &bad, 0, 0, ws) == TKV_AMQ_INVALID_ARGUMENT);
  bad = run;
  bad.n_items = u64{1} << 32;
  EXPECT(merge(&bad, &run, 0, 0, ws) == TKV_AMQ_INVALID_ARGUMENT);
  auto gather = [&](u32 out_key_stride, u64* key_offsets, u64 gws) {
    return tkv_amq_gather_merged(reinterpret_cast<const tkv_amq_merge_item*>(some), begin, 2, 20, &run, &run, some,
                                 out_key_stride, key_offsets, 320, some, reinterpret_cast<u64*>(some), 100, nullptr,
                                 some, gws, nullptr);
  };
  const u64 gws = tkv_amq_gather_merged_ws_bytes(20);
  if (no_device) {
    EXPECT(gather(16, nullptr, gws) == TKV_AMQ_UNAVAILABLE);
    EXPECT(gather(0, reinterpret_cast<u64*>(some), gws) == TKV_AMQ_UNAVAILABLE);
  }
  EXPECT(gather(24, nullptr, gws) == TKV_AMQ_INVALID_ARGUMENT);  // not the runs' stride
  EXPECT(gather(0, nullptr, gws) == TKV_AMQ_INVALID_ARGUMENT);
  EXPECT(gather(16, nullptr, gws - 1) == TKV_AMQ_INVALID_ARGUMENT);
  // the mirror: counts the entry point refuses, a stride of 0
  MergedLeaves out;
  bad = run;
  bad.n_items = u64{1} << 32;
  EXPECT(merge_leaves(bad, run, 2, false, out).code == TKV_AMQ_INVALID_ARGUMENT);
  bad = run;
  bad.value_stride = 0;
  EXPECT(merge_leaves(run, bad, 2, false, out).code == TKV_AMQ_INVALID_ARGUMENT);
  EXPECT(out.begin.size() == 1 && out.n_items == 0);
}

// one side on the device: 16-byte keys in the fixed form, values in the offsets form
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
    EXPECT(merge_leaves(run, run, 1, false, out).code == TKV_AMQ_UNAVAILABLE);
    std::printf("%s (no device; %d failures)\n", failures ? "FAIL" : "NODEVICE-OK", failures);
    return failures ? 1 : 0;
  }

  // two leaves: an update of every op over every op, keys of the update that the leaf lacks, and the other way
  const u32 ops[5] = {TKV_AMQ_OP_DELETE, TKV_AMQ_OP_NOOP, TKV_AMQ_OP_WRITE, TKV_AMQ_OP_ADD_I32, TKV_AMQ_OP_PAGE_SLICE};
  std::vector<std::vector<Item>> newer(2), older(2);
  for (u32 j = 0; j < 2; ++j)
    for (u32 i = 0; i < 600; ++i) {
      const u32 k = 1000 * j + i;
      if (i % 3 != 1) older[j].push_back(Item{key(k), val(ops[(i / 3) % 5], (int32_t)(7 * i) - 900)});
      if (i % 3 != 2 && i % 7 < 4) newer[j].push_back(Item{key(k), val(ops[(i / 15) % 5], (int32_t)(0x7ffffff0u + i % 32))});
    }
  DeviceRun dn, dold;
  dn.upload(newer);
  dold.upload(older);
  for (bool decay : {false, true}) {
    tkv_amq_merge_counts wc{};
    std::vector<Item> want;
    std::vector<u64> begin{0};
    for (u32 j = 0; j < 2; ++j) {
      const std::vector<Item> m = merge_host(newer[j], older[j], decay, wc);
      want.insert(want.end(), m.begin(), m.end());
      begin.push_back(want.size());
    }
    EXPECT(wc.pair_count > 100 && wc.combined_count > 10 && wc.bad_combine_count > 0 && (!decay || wc.dropped_count > 50));
    MergedLeaves out;
    const Status s = merge_leaves(dn.run, dold.run, 2, decay, out);
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
  check_arguments(false);
  std::printf("%s (%d failures)\n", failures ? "FAIL" : "OK", failures);
  return failures ? 1 : 0;
}
