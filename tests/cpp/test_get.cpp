// TreeIndex::get_host and KeyQuery::get_keys of the header-only host mirror (include/turtle_kv_amd/
// filter_builder.hpp) over libtkv_amq.so.  get_host is checked against a hand-written expectation
// on a small tree of height 2 -- one flushed skip, one early exit, a key flushed everywhere -- with
// or without a device; on the GPU KeyQuery::get_keys must equal get_host in (key_index, leaf,
// where) on a tree of height 3 (the result does not depend on the filters' answers as long as they
// have no false negatives, so get_host's "always maybe" is a valid host side).  Exits non-zero on
// any failed expectation; without a device prints NODEVICE-OK.
#include <turtle_kv_amd/filter_builder.hpp>

#include <algorithm>
#include <cstdio>
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

// the leaves' keys, leaf by leaf, and their ranges
struct Leaves {
  std::vector<std::string> keys;
  std::vector<u64> begin{0};
  void add(std::vector<u32> ks)
  {
    std::sort(ks.begin(), ks.end());
    for (u32 k : ks) keys.push_back(key(k));
    begin.push_back(keys.size());
  }
  std::vector<std::string_view> views() const { return {keys.begin(), keys.end()}; }
};

static bool same(const tkv_amq_get_result& r, u64 key_index, u32 leaf, u32 where)
{
  return r.key_index == key_index && r.leaf == leaf && r.where == where;
}

int main()
{
  static_assert(sizeof(tkv_amq_get_result) == 16 && sizeof(tkv_amq_get_counts) == 48, "get records");
  const u32 kLeaf = TKV_AMQ_WALK_LEAF_LEVEL, kNone = ~u32{0};

  // ---- height 2, by hand: a root of 2 pivots (cut at key(30)) over a node of 3 leaves and a node of 1 ----
  // leaves 0..3 are the bottom leaves; 4, 5 (root level 0), 6 (root level 1) and 7 (the left node's level 0)
  Leaves lv;
  lv.add({1, 5});              // leaf 0
  lv.add({12});                // leaf 1
  lv.add({});                  // leaf 2: empty
  lv.add({31, 35});            // leaf 3
  lv.add({2, 5, 33, 35});      // leaf 4: root level 0, active for both pivots; pivot 1 flushed below 3
  lv.add({5, 35, 40});         // leaf 5: root level 0, after leaf 4
  lv.add({35, 36});            // leaf 6: root level 1; pivot 1 flushed below 1
  lv.add({5, 12});             // leaf 7: the left node's level 0
  TreeIndex::Node a = bottom(0, 3), b = bottom(3, 1);
  a.levels = {{seg(7, 0b111)}};
  TreeIndex::Node root = above({a, b}, 0);
  root.levels = {{seg(4, 0b11, {{1, 3}}), seg(5, 0b11)}, {seg(6, 0b10, {{1, 1}})}};
  TreeIndex small;
  EXPECT(TreeIndex::build(root, small).ok());
  const std::vector<std::string> qs{key(5), key(35), key(33), key(36), key(12), key(25), key(31), key(40), key(99)};
  const std::vector<std::string_view> items(qs.begin(), qs.end());
  const std::vector<std::string_view> leaf_keys = lv.views();
  std::vector<tkv_amq_get_result> host;
  std::vector<u32> visits;
  small.get_host(items, leaf_keys, lv.begin, host, [](u32, std::string_view) { return true; }, &visits);
  const auto at = [&](u32 leaf, u32 k) {
    return (u64)(std::find(lv.keys.begin() + lv.begin[leaf], lv.keys.begin() + lv.begin[leaf + 1], key(k)) - lv.keys.begin());
  };
  // key(5), pivot 0: leaf 4's bound is pivot 1's and does not apply -- the early exit, one visit
  EXPECT(same(host[0], at(4, 5), 4, 0) && visits[0] == 1);
  // key(35), pivot 1: index 3 in leaf 4, AT its bound 3 -- found there
  EXPECT(same(host[1], at(4, 35), 4, 0) && visits[1] == 1);
  // key(33), pivot 1: index 2 in leaf 4, below the bound -- flushed; leaf 5 is skipped with the level; level 1's
  // leaf 6 and the right node's leaf 3 do not hold it: four entries on the path, three visited
  EXPECT(same(host[2], ~u64{0}, kNone, kNone) && visits[2] == 3);
  // key(36): not in level 0 (two visits), index 1 in leaf 6, at its bound 1 -- found in level 1
  EXPECT(same(host[3], at(6, 36), 6, 1) && visits[3] == 3);
  // key(12), pivot 0 / pivot 1 of the left node: past both root segments, found in the left node's segment
  EXPECT(same(host[4], at(7, 12), 7, 1 << 8) && visits[4] == 3);
  // key(25): in no segment, and the child of its pivot is leaf 2, which is empty
  EXPECT(same(host[5], ~u64{0}, kNone, kNone) && visits[5] == 4);
  EXPECT(same(host[6], at(3, 31), 3, 1 << 8 | kLeaf) && visits[6] == 4);
  EXPECT(same(host[7], at(5, 40), 5, 0) && visits[7] == 2);
  EXPECT(same(host[8], ~u64{0}, kNone, kNone) && visits[8] == 4);
  // a filter that rejects everything but leaf 6: visits stay, only leaf 6 is searched
  small.get_host(items, leaf_keys, lv.begin, host, [](u32 leaf, std::string_view) { return leaf == 6; }, &visits);
  EXPECT(same(host[3], at(6, 36), 6, 1) && same(host[0], ~u64{0}, kNone, kNone) && visits[0] == 4);
  EXPECT(same(host[1], ~u64{0}, kNone, kNone) && visits[1] == 4);  // key(35) sits below leaf 6's bound

  // ---- height 3: 2 / 2, 1 / 3, 1, 2 bottom leaves; every node dressed with segments whose leaves hold copies ----
  uint64_t st = 77;
  auto rnd = [&st] {
    st ^= st << 13;
    st ^= st >> 7;
    st ^= st << 17;
    return st;
  };
  const u32 kBottom = 6;
  Leaves tl;
  for (u32 i = 0; i < kBottom; ++i) tl.add({10 * i + 1, 10 * i + 4, 10 * i + 7, 10 * i + 9});
  u32 next_seg_leaf = kBottom;
  std::vector<std::vector<u32>> seg_keys;
  auto dress = [&](TreeIndex::Node& n) {
    const u32 pivots = (u32)(n.children.empty() ? n.leaves.size() : n.children.size());
    for (u32 l = 0; l < 2; ++l) {
      std::vector<TreeIndex::Segment> level;
      for (u32 s = 1 + rnd() % 2; s > 0; --s) {
        std::vector<std::pair<u32, u32>> fl;
        for (u32 p = 0; p < pivots; ++p)
          if (rnd() % 3 == 0) fl.push_back({p, (u32)(rnd() % 12)});
        std::vector<u32> ks;
        for (u32 k = 0; k < 10 * kBottom; ++k)
          if (rnd() % 5 == 0) ks.push_back(k);
        seg_keys.push_back(ks);
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
  for (const auto& ks : seg_keys) tl.add(ks);  // (dress() numbered the segments' leaves in this order)
  std::vector<std::string> tq;
  for (u32 i = 0; i <= 10 * kBottom + 3; ++i) tq.push_back(key(i));
  const std::vector<std::string_view> titems(tq.begin(), tq.end());
  const std::vector<std::string_view> tkeys = tl.views();
  std::vector<tkv_amq_get_result> want;
  std::vector<u32> tvisits;
  tall.get_host(titems, tkeys, tl.begin, want, [](u32, std::string_view) { return true; }, &tvisits);
  u32 n_found = 0, n_top = 0, n_bottom = 0;
  for (const auto& r : want) {
    n_found += r.leaf != kNone;
    n_top += r.leaf != kNone && (r.where >> 8) == 0;
    n_bottom += r.leaf != kNone && r.where == (2u << 8 | kLeaf);
  }
  EXPECT(n_found > 30 && n_top > 5 && n_bottom > 0 && n_found < titems.size());

  KeyQuery q(titems);
  std::vector<tkv_amq_get_result> got;
  if (tkv_amq_device_count() == 0) {
    // no GPU: the device path must fail loudly
    const std::vector<tkv_amq_segment> no_segs(tl.begin.size() - 1);
    const Status s = q.get_keys(FilterKind::kBloom, nullptr, nullptr, no_segs, tall, nullptr, nullptr, 16, 0, false, got);
    EXPECT(s.code == TKV_AMQ_UNAVAILABLE && got.size() == titems.size());
    EXPECT(same(got[0], ~u64{0}, kNone, kNone));
    // the entry point itself: a bad call is InvalidArgument, a good one Unavailable
    alignas(16) u8 some[64] = {};
    auto call = [&](int kind, u32 flags, u32 kstride) {
      return tkv_amq_get_keys(kind, some, reinterpret_cast<const tkv_amq_segment*>(some), 1,
                              reinterpret_cast<const tkv_amq_tree_node*>(some), 1,
                              reinterpret_cast<const tkv_amq_tree_segment*>(some), 1,
                              reinterpret_cast<const tkv_amq_tree_child*>(some), 1, reinterpret_cast<const u32*>(some), 1,
                              some, nullptr, 16, 2, some, nullptr, 16, 1, some, nullptr, kstride, 1, nullptr, flags,
                              reinterpret_cast<tkv_amq_get_result*>(some), nullptr, nullptr, nullptr, nullptr);
    };
    EXPECT(call(0, 0, 16) == TKV_AMQ_UNAVAILABLE);
    EXPECT(call(1, TKV_AMQ_GET_CHECK_PAGE_ID, 24) == TKV_AMQ_UNAVAILABLE);
    EXPECT(call(2, 0, 16) == TKV_AMQ_INVALID_ARGUMENT);
    EXPECT(call(0, 2, 16) == TKV_AMQ_INVALID_ARGUMENT);
    EXPECT(call(0, 0, 0) == TKV_AMQ_INVALID_ARGUMENT);
    std::printf("%s (no device; %d failures)\n", failures ? "FAIL" : "NODEVICE-OK", failures);
    return failures ? 1 : 0;
  }

  std::string blob;
  for (const auto& k : tl.keys) blob += k;
  DeviceBuffer d_keys(blob.size());
  EXPECT(hipMemcpy(d_keys.get(), blob.data(), blob.size(), hipMemcpyHostToDevice) == hipSuccess);
  for (FilterKind kind : {FilterKind::kBloom, FilterKind::kQuotient}) {
    FilterBatchBuilder fb{kind, kind == FilterKind::kBloom ? usize{10} : usize{12}, 32704};
    for (usize l = 0; l + 1 < tl.begin.size(); ++l) fb.add_leaf(9000 + l, tl.begin[l + 1] - tl.begin[l]);
    EXPECT(fb.plan().ok());
    DeviceBuffer d_out(fb.total_out_bytes());
    EXPECT(fb.build_all(d_keys.get(), 16, nullptr, d_out.get()).ok());
    EXPECT(fb.check().ok());
    auto& m = KeyQuery::metrics();
    const u64 t0 = m.total_filter_query_count.get(), mis0 = m.page_id_mismatch_count.get();
    tkv_amq_get_counts counts{};
    EXPECT(q.get_keys(kind, d_out.get(), fb.device_segments(), fb.segments(), tall, d_keys.get(), nullptr, 16,
                      tl.keys.size(), true, got, &counts)
               .ok());
    EXPECT(got.size() == want.size());
    u64 total_visits = 0;
    for (usize i = 0; i < want.size(); ++i) {
      EXPECT(same(got[i], want[i].key_index, want[i].leaf, want[i].where));
      total_visits += tvisits[i];
    }
    // the page ids of the tree are the filters' own; a filter can only take visits away
    EXPECT(m.page_id_mismatch_count.get() == mis0);
    EXPECT(counts.found_count == n_found && counts.visit_count == total_visits);
    EXPECT(m.total_filter_query_count.get() - t0 == counts.visit_count);
    EXPECT(counts.leaf_search_count == counts.found_count + counts.absent_count + counts.flushed_count);
    EXPECT(counts.flushed_count > 0 && counts.unsearchable_count == 0);
  }
  std::printf("%s (%d failures)\n", failures ? "FAIL" : "OK", failures);
  return failures ? 1 : 0;
}
