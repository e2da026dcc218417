// TreeIndex and KeyQuery::walk_paths of the header-only host mirror (include/turtle_kv_amd/
// filter_builder.hpp) over libtkv_amq.so.  TreeIndex::walk_host (std::upper_bound) is checked
// against a hand-written expectation on a small tree of height 2, with or without a device; on the
// GPU KeyQuery::walk_paths must equal walk_host entry for entry on a tree of height 3.  Exits
// non-zero on any failed expectation; without a device prints NODEVICE-OK.
#include <turtle_kv_amd/filter_builder.hpp>

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
  for (u32 i = 0; i < n; ++i) d.leaves.push_back(TreeIndex::Leaf{first + i, 7000 + first + i});
  d.page_id = 500 + first;
  return d;
}

// a node of height 2 over `kids` (nodes of height 1), the first of which starts at leaf `first`
static TreeIndex::Node above(std::vector<TreeIndex::Node> kids, u32 first)
{
  TreeIndex::Node d;
  d.page_id = 600 + first;
  for (const auto& k : kids) {
    d.pivot_keys.push_back(key(10 * first));
    first += (u32)k.leaves.size();
  }
  d.pivot_keys.push_back(key(10 * first));
  d.children = std::move(kids);
  return d;
}

struct Entry {
  u32 leaf;
  u64 page_id;
  u32 flushed;
  u16 where;
};

static void expect_path(const TreePaths& p, usize i, const std::vector<Entry>& want)
{
  EXPECT(p.begin[i + 1] - p.begin[i] == want.size());
  if (p.begin[i + 1] - p.begin[i] != want.size()) return;
  for (usize j = 0; j < want.size(); ++j) {
    const usize e = p.begin[i] + j;
    EXPECT(p.leaf[e] == want[j].leaf && p.page_id[e] == want[j].page_id && p.flushed[e] == want[j].flushed &&
           p.where[e] == want[j].where);
  }
}

int main()
{
  static_assert(sizeof(tkv_amq_tree_node) == 32 && sizeof(tkv_amq_tree_segment) == 32 &&
                    sizeof(tkv_amq_tree_child) == 16,
                "tree records");
  const u16 kLeaf = TKV_AMQ_WALK_LEAF_LEVEL;

  // ---- height 2, by hand: a root of 2 pivots over a node of 3 leaves and a node of 1 ----
  TreeIndex::Node a = bottom(0, 3), b = bottom(3, 1);
  a.levels = {{seg(7, 0b101, {{2, 9}, {0, 5}})}};
  TreeIndex::Node root = above({a, b}, 0);
  root.levels = {{seg(8, 0b11), seg(9, 0b10, {{1, 77}})}, {}, {seg(10, 0b01)}};
  TreeIndex small;
  EXPECT(TreeIndex::build(root, small).ok());
  EXPECT(small.nodes().size() == 3 && small.segments().size() == 4 && small.children().size() == 6);
  EXPECT(small.nodes()[0].height == 2 && small.nodes()[0].level_count == 3 && small.nodes()[0].pivot_count == 2);
  EXPECT(small.nodes()[0].level_start[1] == 2 && small.nodes()[0].level_start[2] == 2 &&
         small.nodes()[0].level_start[3] == 3 && small.nodes()[0].level_start[7] == 3);
  EXPECT(small.children()[0].index == 1 && small.children()[1].index == 2 && small.children()[2].index == 0);
  // bounds in pivot order behind flushed_begin: segment 9's {1: 77}, then segment 7's {0: 5, 2: 9}
  EXPECT((small.flushed_bounds() == std::vector<u32>{77, 5, 9}));
  const std::vector<std::string> qs{key(0), key(5), key(10), key(9), key(25), key(30), key(29), key(1000),
                                    std::string(16, '\0')};
  std::vector<std::string_view> items(qs.begin(), qs.end());
  TreePaths host;
  small.walk_host(items, host);
  const std::vector<Entry> left0{{8, 9008, 0, 0}, {10, 9010, 0, 2}, {7, 9007, 5, 1 << 8}, {0, 7000, 0, (u16)(1 << 8 | kLeaf)}};
  const std::vector<Entry> left1{{8, 9008, 0, 0}, {10, 9010, 0, 2}, {1, 7001, 0, (u16)(1 << 8 | kLeaf)}};
  const std::vector<Entry> left2{{8, 9008, 0, 0}, {10, 9010, 0, 2}, {7, 9007, 9, 1 << 8}, {2, 7002, 0, (u16)(1 << 8 | kLeaf)}};
  const std::vector<Entry> right{{8, 9008, 0, 0}, {9, 9009, 77, 0}, {3, 7003, 0, (u16)(1 << 8 | kLeaf)}};
  expect_path(host, 0, left0);  // key(0): below the first interior key
  expect_path(host, 1, left0);
  expect_path(host, 2, left1);  // equal to an interior key: it goes right
  expect_path(host, 3, left0);
  expect_path(host, 4, left2);
  expect_path(host, 5, right);  // equal to the root's interior key
  expect_path(host, 6, left2);
  expect_path(host, 7, right);  // above every key (kp is never compared)
  expect_path(host, 8, left0);  // below every key (k0 is never compared)
  TreePaths host4;
  small.walk_host(items, host4, 4);
  EXPECT(host4.begin == host.begin && host4.leaf == host.leaf && host4.where == host.where);

  // the limits
  {
    TreeIndex t;
    TreeIndex::Node wide = bottom(0, 65);
    EXPECT(TreeIndex::build(wide, t).code == TKV_AMQ_INVALID_ARGUMENT);
    wide = bottom(0, 64);
    EXPECT(TreeIndex::build(wide, t).ok());
    wide.levels.assign(8, {seg(1, 1)});
    EXPECT(TreeIndex::build(wide, t).code == TKV_AMQ_INVALID_ARGUMENT);
    wide.levels.assign(2, std::vector<TreeIndex::Segment>(32, seg(1, 1)));
    EXPECT(TreeIndex::build(wide, t).code == TKV_AMQ_INVALID_ARGUMENT);
    wide.levels.assign(7, std::vector<TreeIndex::Segment>(9, seg(1, 1)));
    EXPECT(TreeIndex::build(wide, t).ok() && t.segments().size() == 63);
    TreeIndex::Node four = bottom(0, 4);
    four.levels = {{seg(1, 1 << 4)}};
    EXPECT(TreeIndex::build(four, t).code == TKV_AMQ_INVALID_ARGUMENT);
  }

  // ---- height 3 with uneven fan-out: 3 / 2, 1, 4 / 3, 1, 5, 1, 2, 1, 2 ----
  uint64_t st = 77;
  auto rnd = [&st] {
    st ^= st << 13;
    st ^= st >> 7;
    st ^= st << 17;
    return st;
  };
  u32 next_seg_leaf = 100;
  auto dress = [&](TreeIndex::Node& n) {
    const u32 pivots = (u32)(n.children.empty() ? n.leaves.size() : n.children.size());
    const u32 n_levels = 1 + rnd() % 3;
    for (u32 l = 0; l < n_levels; ++l) {
      std::vector<TreeIndex::Segment> level;
      for (u32 s = rnd() % 4; s > 0; --s) {
        std::vector<std::pair<u32, u32>> fl;
        for (u32 p = 0; p < pivots; ++p)
          if (rnd() % 3 == 0) fl.push_back({p, (u32)(rnd() % 100000 + 1)});
        level.push_back(seg(next_seg_leaf++, rnd() & ((u64{1} << pivots) - 1), fl));
      }
      n.levels.push_back(level);
    }
  };
  const std::vector<std::vector<u32>> shape{{3, 1}, {5}, {1, 2, 1, 2}};
  std::vector<TreeIndex::Node> mids;
  u32 first = 0;
  for (const auto& group : shape) {
    std::vector<TreeIndex::Node> kids;
    const u32 group_first = first;
    for (u32 n : group) {
      kids.push_back(bottom(first, n));
      dress(kids.back());
      first += n;
    }
    TreeIndex::Node mid = above(std::move(kids), group_first);
    dress(mid);
    mids.push_back(std::move(mid));
  }
  TreeIndex::Node top;
  top.pivot_keys = {key(0), key(10 * 4), key(10 * 9), key(10 * first)};
  top.children = std::move(mids);
  dress(top);
  TreeIndex tall;
  EXPECT(TreeIndex::build(top, tall).ok());
  EXPECT(tall.nodes().size() == 11 && tall.nodes()[0].height == 3 && tall.nodes()[1].height == 2 &&
         tall.nodes()[4].height == 1 && first == 15);
  std::vector<std::string> tq;
  for (u32 i = 0; i <= 10 * first + 5; ++i) tq.push_back(key(i));
  tq.push_back(std::string(16, '\0'));
  tq.push_back(std::string(16, '\xff'));
  std::vector<std::string_view> titems(tq.begin(), tq.end());
  TreePaths want;
  tall.walk_host(titems, want, 3);
  EXPECT(want.begin.back() == want.leaf.size() && want.leaf.size() >= titems.size());
  // every path ends in the leaf that covers its key, two nodes down
  for (usize i = 0; i + 2 < titems.size(); ++i) {
    const usize e = want.begin[i + 1] - 1;
    EXPECT(want.leaf[e] == std::min<u32>((u32)i / 10, first - 1) && want.where[e] == (u16)(2 << 8 | kLeaf));
  }

  KeyQuery q(titems);
  TreePaths got;
  if (tkv_amq_device_count() == 0) {
    // no GPU: the device path must fail loudly
    EXPECT(q.walk_paths(tall, got).code == TKV_AMQ_UNAVAILABLE && got.begin.size() == titems.size() + 1);
    EXPECT(tall.upload().code == TKV_AMQ_UNAVAILABLE);
    // the entry point itself: a bad call is InvalidArgument, a good one Unavailable
    alignas(16) u8 some[64] = {};
    auto call = [&](u64 n_queries, u32 qstride, void* ws, u64 ws_bytes) {
      return tkv_amq_walk_paths(reinterpret_cast<const tkv_amq_tree_node*>(some), 1,
                                reinterpret_cast<const tkv_amq_tree_segment*>(some), 1,
                                reinterpret_cast<const tkv_amq_tree_child*>(some), 1,
                                reinterpret_cast<const u32*>(some), 1, some, nullptr, 16, 2, some, nullptr, qstride,
                                n_queries, reinterpret_cast<u32*>(some), reinterpret_cast<u32*>(some), nullptr, nullptr,
                                nullptr, 4, nullptr, ws, ws_bytes, nullptr);
    };
    const u64 need = tkv_amq_walk_paths_ws_bytes(1);
    EXPECT(need >= 16 && tkv_amq_walk_paths_ws_bytes(u64{1} << 32) == 0);
    EXPECT(call(1, 16, some, need) == TKV_AMQ_UNAVAILABLE);
    EXPECT(call(1, 0, some, need) == TKV_AMQ_INVALID_ARGUMENT);
    EXPECT(call(1, 16, some, need - 1) == TKV_AMQ_INVALID_ARGUMENT);
    EXPECT(call(1, 16, some + 8, need) == TKV_AMQ_INVALID_ARGUMENT);
    EXPECT(call(u64{1} << 32, 16, some, ~u64{0}) == TKV_AMQ_INVALID_ARGUMENT);
    std::printf("%s (no device; %d failures)\n", failures ? "FAIL" : "NODEVICE-OK", failures);
    return failures ? 1 : 0;
  }

  EXPECT(q.walk_paths(tall, got).ok());
  EXPECT(got.begin == want.begin && got.leaf == want.leaf && got.page_id == want.page_id &&
         got.flushed == want.flushed && got.where == want.where);
  // the small tree too (variable work per key: 3 or 4 entries)
  KeyQuery qsmall(items);
  EXPECT(qsmall.walk_paths(small, got).ok());
  EXPECT(got.begin == host.begin && got.leaf == host.leaf && got.page_id == host.page_id &&
         got.flushed == host.flushed && got.where == host.where);
  std::printf("%s (%d failures)\n", failures ? "FAIL" : "OK", failures);
  return failures ? 1 : 0;
}
