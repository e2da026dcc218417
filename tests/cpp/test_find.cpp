// KeyQuery::find_in_leaves of the header-only host mirror (include/turtle_kv_amd/filter_builder.hpp)
// over libtkv_amq.so: three small sorted leaves built through FilterBatchBuilder, a few hundred
// keys walked over CSR path lists by candidate_leaves (no truth given), their candidates searched
// on the device and compared with std::lower_bound over the same leaves on the host -- the found
// index, the leaf, the candidate position and the false-positive count the search adds to
// KeyQuery::metrics().  Exits non-zero on any failed expectation; without a device prints
// NODEVICE-OK.
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

int main()
{
  static_assert(sizeof(tkv_amq_find_result) == 16, "tkv_amq_find_result is 16 bytes");
  static_assert(sizeof(tkv_amq_find_counts) == 32, "tkv_amq_find_counts is 32 bytes");
  const u32 kLeaves = 3, kPerLeaf = 400, kKeyLen = 24;
  uint64_t st = 2025;
  auto rnd = [&st] {
    st ^= st << 13;
    st ^= st >> 7;
    st ^= st << 17;
    return st;
  };
  auto make_key = [&](const char* tag) {
    std::string k(kKeyLen, '\0');
    for (auto& c : k) c = (char)rnd();
    k[kKeyLen - 1] = tag[0];  // hits and misses cannot collide
    return k;
  };
  std::vector<std::string> leaf_keys, miss_keys;
  for (u32 i = 0; i < kLeaves * kPerLeaf; ++i) leaf_keys.push_back(make_key("h"));
  for (u32 i = 0; i < 300; ++i) miss_keys.push_back(make_key("m"));
  // each leaf ascending in std::string_view's order
  auto by_bytes = [](const std::string& a, const std::string& b) { return std::string_view{a} < std::string_view{b}; };
  for (u32 l = 0; l < kLeaves; ++l)
    std::sort(leaf_keys.begin() + l * kPerLeaf, leaf_keys.begin() + (l + 1) * kPerLeaf, by_bytes);

  // queries: every fourth built key (its own leaf first or second on its path), then the misses
  // (all three leaves, then a leaf outside the plan)
  std::vector<std::string_view> items;
  std::vector<u32> path_begin{0}, path_leaf, own;
  std::vector<u64> own_index;
  for (u32 i = 0; i < leaf_keys.size(); i += 4) {
    const u32 leaf = i / kPerLeaf;
    items.push_back(leaf_keys[i]);
    own.push_back(leaf);
    own_index.push_back(i);
    const u32 first = (i / 4) % 2;  // odd queries visit another leaf before their own
    for (u32 j = 0; j < kLeaves; ++j) path_leaf.push_back((leaf + j + (first ? kLeaves - 1 : 0)) % kLeaves);
    path_begin.push_back((u32)path_leaf.size());
  }
  const usize n_hits = items.size();
  for (const auto& k : miss_keys) {
    items.push_back(k);
    for (u32 j = 0; j <= kLeaves; ++j) path_leaf.push_back(j);
    path_begin.push_back((u32)path_leaf.size());
  }
  KeyQuery q(items);
  std::vector<u32> cand_begin, cand_leaf;
  std::vector<tkv_amq_find_result> found;

  if (tkv_amq_device_count() == 0) {
    // no GPU: the device path must fail loudly
    const std::vector<tkv_amq_segment> no_segs(kLeaves);
    cand_begin.assign(items.size() + 1, 0);
    const Status s = q.find_in_leaves(FilterKind::kBloom, nullptr, nullptr, no_segs, cand_begin, cand_leaf, nullptr,
                                      nullptr, kKeyLen, 0, found);
    EXPECT(s.code == TKV_AMQ_UNAVAILABLE && found.size() == items.size());
    EXPECT(found[0].key_index == ~u64{0} && found[0].leaf == ~u32{0} && found[0].cand == ~u32{0});
    // the entry point itself: a bad call is InvalidArgument, a good one Unavailable
    alignas(16) u8 some[64] = {};
    auto call = [&](int kind, u32 flags, u32 qstride) {
      return tkv_amq_find_keys(kind, nullptr, reinterpret_cast<const tkv_amq_segment*>(some), 1, some, nullptr,
                               qstride, 1, reinterpret_cast<const u32*>(some), reinterpret_cast<const u32*>(some),
                               nullptr, 1, some, nullptr, 16, 1, nullptr, flags,
                               reinterpret_cast<tkv_amq_find_result*>(some), nullptr, nullptr, nullptr, nullptr);
    };
    EXPECT(call(0, 0, 16) == TKV_AMQ_UNAVAILABLE);
    EXPECT(call(1, TKV_AMQ_FIND_ALL, 24) == TKV_AMQ_UNAVAILABLE);
    EXPECT(call(2, 0, 16) == TKV_AMQ_INVALID_ARGUMENT);
    EXPECT(call(0, 2, 16) == TKV_AMQ_INVALID_ARGUMENT);
    EXPECT(call(0, 0, 0) == TKV_AMQ_INVALID_ARGUMENT);
    std::printf("%s (no device; %d failures)\n", failures ? "FAIL" : "NODEVICE-OK", failures);
    return failures ? 1 : 0;
  }

  std::string blob;
  for (const auto& k : leaf_keys) blob += k;
  DeviceBuffer d_keys(blob.size());
  EXPECT(hipMemcpy(d_keys.get(), blob.data(), blob.size(), hipMemcpyHostToDevice) == hipSuccess);
  for (FilterKind kind : {FilterKind::kBloom, FilterKind::kQuotient}) {
    FilterBatchBuilder b{kind, kind == FilterKind::kBloom ? usize{10} : usize{12}, 32704};
    for (u32 l = 0; l < kLeaves; ++l) b.add_leaf(100 + l, kPerLeaf);
    EXPECT(b.plan().ok());
    DeviceBuffer d_out(b.total_out_bytes());
    EXPECT(b.build_all(d_keys.get(), kKeyLen, nullptr, d_out.get()).ok());
    EXPECT(b.check().ok());

    auto& m = KeyQuery::metrics();
    EXPECT(q.candidate_leaves(kind, d_out.get(), b.device_segments(), b.segments(), path_begin, path_leaf,
                              cand_begin, cand_leaf).ok());
    const u64 f0 = m.filter_false_positive_count.get(), p0 = m.filter_positive_count.get();
    EXPECT(q.find_in_leaves(kind, d_out.get(), b.device_segments(), b.segments(), cand_begin, cand_leaf,
                            d_keys.get(), nullptr, kKeyLen, leaf_keys.size(), found).ok());
    EXPECT(found.size() == items.size());
    EXPECT(m.filter_positive_count.get() == p0);  // (the search counts false positives only)

    // the same walk on the host: std::lower_bound over each candidate leaf, ended at the first hit
    u64 want_fp = 0;
    for (usize i = 0; i < items.size(); ++i) {
      tkv_amq_find_result want{~u64{0}, ~u32{0}, ~u32{0}};
      for (u32 c = cand_begin[i]; c < cand_begin[i + 1]; ++c) {
        const u32 leaf = cand_leaf[c];
        if (leaf >= kLeaves) continue;
        const auto lo = leaf_keys.begin() + leaf * kPerLeaf, hi = lo + kPerLeaf;
        const auto it = std::lower_bound(lo, hi, std::string(items[i]), by_bytes);
        if (it != hi && *it == items[i]) {
          want = tkv_amq_find_result{(u64)(it - leaf_keys.begin()), leaf, c};
          break;
        }
        ++want_fp;
      }
      EXPECT(found[i].key_index == want.key_index && found[i].leaf == want.leaf && found[i].cand == want.cand);
    }
    // no false negatives and a correct search: every built key at exactly its own index
    for (usize i = 0; i < n_hits; ++i) EXPECT(found[i].key_index == own_index[i] && found[i].leaf == own[i]);
    for (usize i = n_hits; i < items.size(); ++i) EXPECT(found[i].key_index == ~u64{0});
    EXPECT(m.filter_false_positive_count.get() - f0 == want_fp);
  }
  std::printf("%s (%d failures)\n", failures ? "FAIL" : "OK", failures);
  return failures ? 1 : 0;
}
