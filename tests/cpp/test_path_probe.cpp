// KeyQuery::candidate_leaves of the header-only host mirror
// (include/turtle_kv_amd/filter_builder.hpp) over libtkv_amq.so: three small leaves built
// through FilterBatchBuilder, a few hundred keys walked over CSR path lists.  Exits non-zero on
// any failed expectation; without a device prints NODEVICE-OK.
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

int main()
{
  const u32 kLeaves = 3, kPerLeaf = 400, kKeyLen = 24;
  uint64_t st = 2024;
  auto rnd = [&st] {
    st ^= st << 13;
    st ^= st >> 7;
    st ^= st << 17;
    return st;
  };
  auto make_key = [&](const char* tag) {
    std::string k(kKeyLen, '\0');
    for (auto& c : k) c = (char)rnd();
    k[0] = tag[0];  // hits and misses cannot collide
    return k;
  };
  std::vector<std::string> leaf_keys, miss_keys;
  for (u32 i = 0; i < kLeaves * kPerLeaf; ++i) leaf_keys.push_back(make_key("h"));
  for (u32 i = 0; i < 300; ++i) miss_keys.push_back(make_key("m"));

  // queries: every fourth built key (its own leaf first, then the two others), then the misses
  // (all three leaves, then a leaf outside the plan)
  std::vector<std::string_view> items;
  std::vector<u32> path_begin{0}, path_leaf, own;
  std::vector<u8> truth;
  for (u32 i = 0; i < leaf_keys.size(); i += 4) {
    const u32 leaf = i / kPerLeaf;
    items.push_back(leaf_keys[i]);
    own.push_back(leaf);
    for (u32 j = 0; j < kLeaves; ++j) {
      path_leaf.push_back((leaf + j) % kLeaves);
      truth.push_back(j == 0);
    }
    path_begin.push_back((u32)path_leaf.size());
  }
  const usize n_hits = items.size();
  for (const auto& k : miss_keys) {
    items.push_back(k);
    for (u32 j = 0; j <= kLeaves; ++j) {
      path_leaf.push_back(j);
      truth.push_back(0);
    }
    path_begin.push_back((u32)path_leaf.size());
  }
  KeyQuery q(items);
  std::vector<u32> cand_begin, cand_leaf;

  if (tkv_amq_device_count() == 0) {
    // no GPU: the device path must fail loudly
    const std::vector<tkv_amq_segment> no_segs(kLeaves);
    const Status s = q.candidate_leaves(FilterKind::kBloom, nullptr, nullptr, no_segs, path_begin, path_leaf,
                                        cand_begin, cand_leaf);
    EXPECT(s.code == TKV_AMQ_UNAVAILABLE && cand_leaf.empty());
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
    const u64 t0 = m.total_filter_query_count.get(), r0 = m.filter_reject_count.get(),
              p0 = m.filter_positive_count.get(), f0 = m.filter_false_positive_count.get(),
              x0 = m.page_id_mismatch_count.get(), z0 = m.no_filter_page_count.get();
    const Status s = q.candidate_leaves(kind, d_out.get(), b.device_segments(), b.segments(), path_begin,
                                        path_leaf, cand_begin, cand_leaf, &truth);
    EXPECT(s.ok());
    // cand_begin is consistent with cand_leaf, and each list is a subsequence of its path
    EXPECT(cand_begin.size() == items.size() + 1 && cand_begin.front() == 0);
    EXPECT(cand_begin.back() == cand_leaf.size());
    for (usize i = 0; i < items.size(); ++i) {
      EXPECT(cand_begin[i] <= cand_begin[i + 1]);
      u32 p = path_begin[i];
      for (u32 c = cand_begin[i]; c < cand_begin[i + 1]; ++c) {
        while (p < path_begin[i + 1] && path_leaf[p] != cand_leaf[c]) ++p;
        EXPECT(p < path_begin[i + 1]);
        ++p;
      }
    }
    // no false negatives: a built key's own leaf is its first candidate
    for (usize i = 0; i < n_hits; ++i)
      EXPECT(cand_begin[i] < cand_begin[i + 1] && cand_leaf[cand_begin[i]] == own[i]);
    // a miss keeps the leaf outside the plan (cannot reject), as its last candidate
    usize miss_cands = 0;
    for (usize i = n_hits; i < items.size(); ++i) {
      EXPECT(cand_begin[i] < cand_begin[i + 1] && cand_leaf[cand_begin[i + 1] - 1] == kLeaves);
      miss_cands += cand_begin[i + 1] - cand_begin[i];
    }
    EXPECT(miss_cands < 2 * miss_keys.size());  // nearly every in-plan entry of a miss is rejected
    // the metrics delta adds up
    const u64 total = m.total_filter_query_count.get() - t0, rej = m.filter_reject_count.get() - r0,
              pos = m.filter_positive_count.get() - p0, fp = m.filter_false_positive_count.get() - f0,
              mism = m.page_id_mismatch_count.get() - x0, nof = m.no_filter_page_count.get() - z0;
    EXPECT(total == path_leaf.size());
    EXPECT(rej + pos + nof + mism == total);
    EXPECT(nof == miss_keys.size() && mism == 0);
    EXPECT(pos + nof == cand_leaf.size());
    EXPECT(pos >= n_hits && fp == pos - n_hits);
  }
  std::printf("%s (%d failures)\n", failures ? "FAIL" : "OK", failures);
  return failures ? 1 : 0;
}
