// TreeIndex::get_values_host and KeyQuery::get_values of the header-only host mirror (include/turtle_kv_amd/
// filter_builder.hpp) over libtkv_amq.so.  get_values_host is checked against a hand-written expectation
// on a small tree of height 2 -- ADD over ADD over ADD over WRITE across two root levels, a node's level and
// a child leaf; a delta resolved by a tombstone; a tombstone met first; a flushed ADD that is not taken; an
// ADD taken at its bound; a delta that stays pending -- with or without a device; on the GPU
// KeyQuery::get_values must equal get_values_host in every field of the record, in the counts and in the
// gathered bytes on a tree of height 3 with a mix of ops (the result does not depend on the filters' answers
// as long as they have no false negatives, so the host's "always maybe" is a valid host side).  Exits
// non-zero on any failed expectation; without a device prints NODEVICE-OK.
#include <turtle_kv_amd/filter_builder.hpp>

#include <algorithm>
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

// a packed value: the op byte, then `width` bytes of x, little-endian
static std::string val(u32 op, int32_t x = 0, int width = 0)
{
  std::string v(1, (char)op);
  for (int b = 0; b < width; ++b) v.push_back((char)((u32)x >> (8 * b)));
  return v;
}

static TreeIndex::Segment seg(u32 leaf, u64 active, std::vector<std::pair<u32, u32>> flushed = {})
{
  TreeIndex::Segment s;
  s.leaf = leaf;
  s.page_id = 9000 + leaf;
  s.active_pivots = active;
  s.flushed = std::move(flushed);
  return s;
}

// a node of height 1 over leaves [first, first + n), leaf i covering [key(10 i), key(10 (i + 1)))
static TreeIndex::Node bottom(u32 first, u32 n)
{
  TreeIndex::Node d;
  for (u32 i = 0; i <= n; ++i) d.pivot_keys.push_back(key(10 * (first + i)));
  for (u32 i = 0; i < n; ++i) d.leaves.push_back(TreeIndex::Leaf{first + i, 9000 + first + i});
  d.page_id = 500 + first;
  return d;
}

static TreeIndex::Node above(std::vector<TreeIndex::Node> kids, u32 first)
{
  TreeIndex::Node d;
  d.page_id = 600 + first;
  for (const auto& k : kids) {
    d.pivot_keys.push_back(key(10 * first));
    first += (u32)(k.leaves.empty() ? 0 : k.leaves.size());
  }
  d.pivot_keys.push_back(key(10 * first));
  d.children = std::move(kids);
  return d;
}

// the leaves' keys and values, leaf by leaf, and their ranges
struct Leaves {
  std::vector<std::string> keys, values;
  std::vector<u64> begin{0};
  void add(std::vector<std::pair<u32, std::string>> items)
  {
    std::sort(items.begin(), items.end());
    for (auto& [k, v] : items) {
      keys.push_back(key(k));
      values.push_back(v);
    }
    begin.push_back(keys.size());
  }
  std::vector<std::string_view> key_views() const { return {keys.begin(), keys.end()}; }
  std::vector<std::string_view> value_views() const { return {values.begin(), values.end()}; }
};

static bool same(const tkv_amq_value_result& r, u64 key_index, u64 last_index, u32 leaf, u32 where, int32_t i32, u32 op,
                 u32 flags, u32 n_items)
{
  return r.key_index == key_index && r.last_index == last_index && r.leaf == leaf && r.where == where && r.i32 == i32 &&
         r.op == op && r.flags == flags && r.n_items == n_items;
}

static bool equal(const tkv_amq_value_result& a, const tkv_amq_value_result& b)
{
  return same(a, b.key_index, b.last_index, b.leaf, b.where, b.i32, b.op, b.flags, b.n_items);
}

int main()
{
  static_assert(sizeof(tkv_amq_value_result) == 32 && sizeof(tkv_amq_value_counts) == 64, "value records");
  const u32 kLeaf = TKV_AMQ_WALK_LEAF_LEVEL, kNone = ~u32{0};
  const u64 kNoKey = ~u64{0};
  const u32 DEL = TKV_AMQ_OP_DELETE, NOOP = TKV_AMQ_OP_NOOP, WR = TKV_AMQ_OP_WRITE, ADD = TKV_AMQ_OP_ADD_I32,
            SLICE = TKV_AMQ_OP_PAGE_SLICE, COMB = TKV_AMQ_VALUE_COMBINED, BAD = TKV_AMQ_VALUE_BAD_COMBINE;

  // as_i32 by data length
  EXPECT(TreeIndex::value_i32("") == 0 && TreeIndex::value_i32(std::string_view("\x80", 1)) == (u32)-128);
  EXPECT(TreeIndex::value_i32(std::string_view("\xfe\xff", 2)) == (u32)-2);
  EXPECT(TreeIndex::value_i32(std::string_view("\x00\x00\x80", 3)) == (u32) - (1 << 23));
  EXPECT(TreeIndex::value_i32(std::string_view("\x70\x11\x01", 3)) == 70000u);
  EXPECT(TreeIndex::value_i32(std::string_view("\xff\xff\xff\x7f\xaa\xbb", 6)) == 0x7fffffffu);

  // ---- height 2, by hand: a root of 2 pivots (cut at key(30)) over a node of 3 leaves and a node of 1 ----
  // leaves 0..3 are the bottom leaves; 4 (root level 0), 5 (root level 1) and 6 (the left node's level 0)
  Leaves lv;
  lv.add({{1, val(WR) + "one"}, {5, val(WR, 100, 4)}});                                     // leaf 0
  lv.add({{12, val(DEL)}});                                                                  // leaf 1
  lv.add({});                                                                                // leaf 2: empty
  lv.add({{31, val(WR, 7, 4)}, {35, val(WR, 1000, 2)}});                                     // leaf 3
  // leaf 4: root level 0, active for both pivots; pivot 1 flushed below index 4 (key 33 is at 3, key 35 at 4)
  lv.add({{2, val(ADD, 8, 1)}, {5, val(ADD, 1, 4)}, {12, val(ADD, 3, 4)}, {33, val(ADD, 50, 4)}, {35, val(ADD, 2, 4)}});
  lv.add({{5, val(ADD, 10, 4)}, {33, val(WR, 9, 4)}, {40, val(DEL)}, {41, val(ADD, -1, 1)}});  // leaf 5: root level 1
  lv.add({{5, val(ADD, 20, 4)}, {12, val(ADD, 4, 4)}});                                      // leaf 6: the left node's level 0
  TreeIndex::Node a = bottom(0, 3), b = bottom(3, 1);
  a.levels = {{seg(6, 0b111)}};
  TreeIndex::Node root = above({a, b}, 0);
  root.levels = {{seg(4, 0b11, {{1, 4}})}, {seg(5, 0b11)}};
  TreeIndex small;
  EXPECT(TreeIndex::build(root, small).ok());
  const std::vector<std::string> qs{key(5), key(12), key(40), key(33), key(35), key(31), key(1), key(99), key(25), key(2),
                                    key(41)};
  const std::vector<std::string_view> items(qs.begin(), qs.end());
  const std::vector<std::string_view> leaf_keys = lv.key_views(), leaf_values = lv.value_views();
  std::vector<tkv_amq_value_result> host;
  std::vector<u32> visits;
  tkv_amq_value_counts hc{};
  const auto all = [](u32, std::string_view) { return true; };
  small.get_values_host(items, leaf_keys, leaf_values, lv.begin, host, all, &visits, &hc);
  const auto at = [&](u32 leaf, u32 k) {
    return (u64)(std::find(lv.keys.begin() + lv.begin[leaf], lv.keys.begin() + lv.begin[leaf + 1], key(k)) - lv.keys.begin());
  };
  // key(5): ADD 1 (root level 0) over ADD 10 (root level 1) over ADD 20 (the left node) over WRITE 100 (leaf 0)
  EXPECT(same(host[0], at(4, 5), at(0, 5), 4, 0, 131, WR, COMB, 4) && visits[0] == 4);
  // key(12): ADD 3, absent from level 1, ADD 4, then the tombstone of leaf 1: WRITE of the accumulator
  EXPECT(same(host[1], at(4, 12), at(1, 12), 4, 0, 7, WR, COMB, 3) && visits[1] == 4);
  // key(40): a tombstone met first ends the lookup as a tombstone; leaf 3 is not visited
  EXPECT(same(host[2], at(5, 40), at(5, 40), 5, 1, 0, DEL, 0, 1) && visits[2] == 2);
  // key(33): its ADD 50 in leaf 4 lies below the flushed bound -- not taken -- and level 1's WRITE is the value
  EXPECT(same(host[3], at(5, 33), at(5, 33), 5, 1, 0, WR, 0, 1) && visits[3] == 2);
  // key(35): AT the bound: taken; absent from level 1; WRITE 1000 (two data bytes) in leaf 3
  EXPECT(same(host[4], at(4, 35), at(3, 35), 4, 0, 1002, WR, COMB, 2) && visits[4] == 3);
  EXPECT(same(host[5], at(3, 31), at(3, 31), 3, 1 << 8 | kLeaf, 0, WR, 0, 1) && visits[5] == 3);
  EXPECT(same(host[6], at(0, 1), at(0, 1), 0, 1 << 8 | kLeaf, 0, WR, 0, 1) && visits[6] == 4);
  EXPECT(same(host[7], kNoKey, kNoKey, kNone, kNone, 0, TKV_AMQ_OP_NONE, 0, 0) && visits[7] == 3);
  EXPECT(same(host[8], kNoKey, kNoKey, kNone, kNone, 0, TKV_AMQ_OP_NONE, 0, 0) && visits[8] == 4);
  // key(2): one ADD (one data byte) and nothing below it: pending
  EXPECT(same(host[9], at(4, 2), at(4, 2), 4, 0, 8, ADD, 0, 1) && visits[9] == 4);
  // key(41): ADD -1 in level 1, sign-extended from one byte; leaf 3 does not hold it
  EXPECT(same(host[10], at(5, 41), at(5, 41), 5, 1, -1, ADD, 0, 1) && visits[10] == 3);
  EXPECT(hc.found_count == 9 && hc.item_count == 4 + 3 + 1 + 1 + 2 + 1 + 1 + 1 + 1 && hc.bad_combine_count == 0);
  // a filter that rejects everything but leaf 5: visits stay, only leaf 5's items are taken
  small.get_values_host(items, leaf_keys, leaf_values, lv.begin, host, [](u32 leaf, std::string_view) { return leaf == 5; },
                        &visits);
  EXPECT(same(host[0], at(5, 5), at(5, 5), 5, 1, 10, ADD, 0, 1) && visits[0] == 4);
  EXPECT(same(host[4], kNoKey, kNoKey, kNone, kNone, 0, TKV_AMQ_OP_NONE, 0, 0) && visits[4] == 3);
  // bad combinations: a NOOP behind an ADD in the same node goes on; as the first item of the child it ends the lookup
  {
    Leaves bl = lv;
    bl.values[at(5, 5)] = val(NOOP);                        // root level 1, behind root level 0's ADD: goes on
    bl.values[at(6, 12)] = val(SLICE) + "s";                // the left node's first item for key(12): ends it
    const std::vector<std::string_view> bv = bl.value_views();
    tkv_amq_value_counts bc{};
    small.get_values_host(items, leaf_keys, bv, lv.begin, host, all, &visits, &bc);
    EXPECT(same(host[0], at(4, 5), at(0, 5), 4, 0, 121, WR, COMB | BAD, 4) && visits[0] == 4);
    EXPECT(same(host[1], at(4, 12), at(6, 12), 4, 0, 3, ADD, BAD, 2) && visits[1] == 3);   // leaf 1 is not visited
    EXPECT(bc.bad_combine_count == 2);
  }

  // ---- height 3: 2 / 2, 1 / 3, 1, 2 bottom leaves; every node dressed with segments whose leaves hold copies ----
  uint64_t st = 77;
  auto rnd = [&st] {
    st ^= st << 13;
    st ^= st >> 7;
    st ^= st << 17;
    return st;
  };
  const u32 ops[] = {ADD, ADD, ADD, WR, WR, DEL, NOOP, SLICE};
  auto random_value = [&] {
    std::string v = val(ops[rnd() % 8]);
    for (u32 n = (u32)(rnd() % 7); n > 0; --n) v.push_back((char)rnd());
    return v;
  };
  const u32 kBottom = 6;
  Leaves tl;
  for (u32 i = 0; i < kBottom; ++i) {
    std::vector<std::pair<u32, std::string>> ks;
    for (u32 r : {1u, 4u, 7u, 9u}) ks.push_back({10 * i + r, val(WR) + "bottom-value-" + std::to_string(10 * i + r)});
    tl.add(ks);
  }
  u32 next_seg_leaf = kBottom;
  std::vector<std::vector<std::pair<u32, std::string>>> seg_items;
  auto dress = [&](TreeIndex::Node& n) {
    const u32 pivots = (u32)(n.children.empty() ? n.leaves.size() : n.children.size());
    for (u32 l = 0; l < 2; ++l) {
      std::vector<TreeIndex::Segment> level;
      for (u32 s = 1 + rnd() % 2; s > 0; --s) {
        std::vector<std::pair<u32, u32>> fl;
        for (u32 p = 0; p < pivots; ++p)
          if (rnd() % 3 == 0) fl.push_back({p, (u32)(rnd() % 12)});
        std::vector<std::pair<u32, std::string>> ks;
        for (u32 k = 0; k < 10 * kBottom; ++k)
          if (rnd() % 5 == 0) ks.push_back({k, random_value()});
        seg_items.push_back(ks);
        level.push_back(seg(next_seg_leaf++, (u64{1} << pivots) - 1, fl));
      }
      n.levels.push_back(level);
    }
  };
  TreeIndex::Node b0 = bottom(0, 3), b1 = bottom(3, 1), b2 = bottom(4, 2);
  dress(b0);
  dress(b1);
  dress(b2);
  TreeIndex::Node m0 = above({b0, b1}, 0), m1 = above({b2}, 4);
  dress(m0);
  dress(m1);
  TreeIndex::Node top;
  top.pivot_keys = {key(0), key(40), key(60)};
  top.children = {m0, m1};
  dress(top);
  TreeIndex tall;
  EXPECT(TreeIndex::build(top, tall).ok());
  EXPECT(tall.nodes().size() == 6 && tall.nodes()[0].height == 3);
  for (const auto& ks : seg_items) tl.add(ks);  // (dress() numbered the segments' leaves in this order)
  std::vector<std::string> tq;
  for (u32 i = 0; i <= 10 * kBottom + 3; ++i) tq.push_back(key(i));
  const std::vector<std::string_view> titems(tq.begin(), tq.end());
  const std::vector<std::string_view> tkeys = tl.key_views(), tvalues = tl.value_views();
  std::vector<tkv_amq_value_result> want;
  std::vector<u32> tvisits;
  tkv_amq_value_counts wc{};
  tall.get_values_host(titems, tkeys, tvalues, tl.begin, want, all, &tvisits, &wc);
  u32 n_combined = 0, n_bad = 0;
  for (const auto& r : want) {
    n_combined += (r.flags & COMB) != 0;
    n_bad += (r.flags & BAD) != 0;
  }
  EXPECT(wc.found_count > 30 && wc.item_count > wc.found_count + 10 && n_combined > 5 && n_bad > 0);
  EXPECT(wc.found_count < titems.size());

  KeyQuery q(titems);
  std::vector<tkv_amq_value_result> got;
  if (tkv_amq_device_count() == 0) {
    // no GPU: the device path must fail loudly
    const std::vector<tkv_amq_segment> no_segs(tl.begin.size() - 1);
    const Status s = q.get_values(FilterKind::kBloom, nullptr, nullptr, no_segs, tall, nullptr, nullptr, 16, 0, nullptr,
                                  nullptr, 1, 0, false, got);
    EXPECT(s.code == TKV_AMQ_UNAVAILABLE && got.size() == titems.size());
    EXPECT(same(got[0], kNoKey, kNoKey, kNone, kNone, 0, TKV_AMQ_OP_NONE, 0, 0));
    // the entry points themselves: a bad call is InvalidArgument, a good one Unavailable
    alignas(16) u8 some[64] = {};
    auto call = [&](int kind, u32 flags, const u8* values, u32 vstride, u32 result_off) {
      return tkv_amq_get_values(kind, some, reinterpret_cast<const tkv_amq_segment*>(some), 1,
                                reinterpret_cast<const tkv_amq_tree_node*>(some), 1,
                                reinterpret_cast<const tkv_amq_tree_segment*>(some), 1,
                                reinterpret_cast<const tkv_amq_tree_child*>(some), 1, reinterpret_cast<const u32*>(some),
                                1, some, nullptr, 16, 2, some, nullptr, 16, 1, some, nullptr, 16, 1, nullptr, values,
                                nullptr, vstride, 5, flags, reinterpret_cast<tkv_amq_value_result*>(some + result_off),
                                nullptr, nullptr, nullptr, nullptr);
    };
    EXPECT(call(0, 0, some, 5, 0) == TKV_AMQ_UNAVAILABLE);
    EXPECT(call(1, TKV_AMQ_GET_CHECK_PAGE_ID, some + 3, 1, 16) == TKV_AMQ_UNAVAILABLE);
    EXPECT(call(2, 0, some, 5, 0) == TKV_AMQ_INVALID_ARGUMENT);
    EXPECT(call(0, 2, some, 5, 0) == TKV_AMQ_INVALID_ARGUMENT);
    EXPECT(call(0, 0, nullptr, 5, 0) == TKV_AMQ_INVALID_ARGUMENT);
    EXPECT(call(0, 0, some, 0, 0) == TKV_AMQ_INVALID_ARGUMENT);
    EXPECT(call(0, 0, some, 5, 8) == TKV_AMQ_INVALID_ARGUMENT);
    u32 len = 0;
    EXPECT(tkv_amq_gather_values(reinterpret_cast<const tkv_amq_value_result*>(some), 1, some, nullptr, 5, 5, 1, some + 32,
                                 8, &len, nullptr) == TKV_AMQ_UNAVAILABLE);
    EXPECT(tkv_amq_gather_values(reinterpret_cast<const tkv_amq_value_result*>(some), 1, some, nullptr, 5, 5, 1, nullptr,
                                 8, &len, nullptr) == TKV_AMQ_INVALID_ARGUMENT);
    std::printf("%s (no device; %d failures)\n", failures ? "FAIL" : "NODEVICE-OK", failures);
    return failures ? 1 : 0;
  }

  std::string blob, vblob;
  std::vector<u64> voffs{0};
  for (const auto& k : tl.keys) blob += k;
  for (const auto& v : tl.values) {
    vblob += v;
    voffs.push_back(vblob.size());
  }
  DeviceBuffer d_keys(blob.size()), d_values(vblob.size()), d_voffs(8 * voffs.size());
  EXPECT(hipMemcpy(d_keys.get(), blob.data(), blob.size(), hipMemcpyHostToDevice) == hipSuccess);
  EXPECT(hipMemcpy(d_values.get(), vblob.data(), vblob.size(), hipMemcpyHostToDevice) == hipSuccess);
  EXPECT(hipMemcpy(d_voffs.get(), voffs.data(), 8 * voffs.size(), hipMemcpyHostToDevice) == hipSuccess);
  const u32 kSlot = 12;
  for (FilterKind kind : {FilterKind::kBloom, FilterKind::kQuotient}) {
    FilterBatchBuilder fb{kind, kind == FilterKind::kBloom ? usize{10} : usize{12}, 32704};
    for (usize l = 0; l + 1 < tl.begin.size(); ++l) fb.add_leaf(9000 + l, tl.begin[l + 1] - tl.begin[l]);
    EXPECT(fb.plan().ok());
    DeviceBuffer d_out(fb.total_out_bytes());
    EXPECT(fb.build_all(d_keys.get(), 16, nullptr, d_out.get()).ok());
    EXPECT(fb.check().ok());
    auto& m = KeyQuery::metrics();
    const u64 t0 = m.total_filter_query_count.get();
    tkv_amq_value_counts counts{};
    std::vector<u8> slots;
    std::vector<u32> lengths;
    EXPECT(q.get_values(kind, d_out.get(), fb.device_segments(), fb.segments(), tall, d_keys.get(), nullptr, 16,
                        tl.keys.size(), d_values.get(), d_voffs.get<u64>(), 0, vblob.size(), true, got, &counts, &slots,
                        &lengths, kSlot)
               .ok());
    EXPECT(got.size() == want.size() && lengths.size() == want.size() && slots.size() == kSlot * want.size());
    u64 total_visits = 0;
    for (usize i = 0; i < want.size() && i < got.size(); ++i) {
      EXPECT(equal(got[i], want[i]));
      total_visits += tvisits[i];
      // the gathered bytes: the integer of a combined value, nothing for none or a tombstone, else the item's data
      std::string data;
      if (want[i].n_items) {
        if (want[i].flags & COMB)
          data.assign(reinterpret_cast<const char*>(&want[i].i32), 4);
        else if (want[i].op != DEL && !tl.values[want[i].key_index].empty())
          data = tl.values[want[i].key_index].substr(1);
      }
      EXPECT(lengths[i] == data.size());
      EXPECT(std::memcmp(slots.data() + kSlot * i, data.data(), std::min<usize>(data.size(), kSlot)) == 0);
    }
    EXPECT(counts.found_count == wc.found_count && counts.item_count == wc.item_count);
    EXPECT(counts.bad_combine_count == wc.bad_combine_count && counts.visit_count == total_visits);
    EXPECT(m.total_filter_query_count.get() - t0 == counts.visit_count);
    EXPECT(counts.leaf_search_count == counts.item_count + counts.absent_count + counts.flushed_count);
    EXPECT(counts.flushed_count > 0 && counts.unsearchable_count == 0);
  }
  std::printf("%s (%d failures)\n", failures ? "FAIL" : "OK", failures);
  return failures ? 1 : 0;
}
