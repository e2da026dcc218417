// verify_members / FilterBatchBuilder::verify of the header-only host mirror
// (include/turtle_kv_amd/filter_builder.hpp) over libtkv_amq.so: one Bloom and one VQF batch built
// through FilterBatchBuilder and verified clean; then a damaged copy (half of one leaf's blocks
// zeroed, two equal leaves' payloads swapped) whose per-leaf counts must equal what tkv_amq_probe
// answers for every (key, own leaf) pair; then the opened segments with the key CSR.  Exits
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

int main()
{
  static_assert(sizeof(tkv_amq_member_check) == 16, "tkv_amq_member_check is 16 bytes");
  if (tkv_amq_device_count() == 0) {
    // no GPU: the device path must fail loudly, bad arguments first
    std::vector<tkv_amq_member_check> r;
    alignas(16) u8 some[64] = {};
    EXPECT(verify_members(FilterKind::kBloom, nullptr, nullptr, 0, 0, nullptr, 16, nullptr, 0, nullptr, r).code ==
           TKV_AMQ_UNAVAILABLE);
    EXPECT(verify_members(FilterKind::kQuotient, some, reinterpret_cast<const tkv_amq_segment*>(some), 1, 0, some, 16,
                          nullptr, 4, nullptr, r).code == TKV_AMQ_UNAVAILABLE);
    EXPECT(r.size() == 1 && r[0].missing == 0 && r[0].first_missing == ~u64{0});
    // a null filter array with a leaf to check, fixed keys with stride 0
    EXPECT(verify_members(FilterKind::kBloom, nullptr, reinterpret_cast<const tkv_amq_segment*>(some), 1, 0, some, 16,
                          nullptr, 4, nullptr, r).code == TKV_AMQ_INVALID_ARGUMENT);
    EXPECT(verify_members(FilterKind::kBloom, some, reinterpret_cast<const tkv_amq_segment*>(some), 1, 0, some, 0,
                          nullptr, 4, nullptr, r).code == TKV_AMQ_INVALID_ARGUMENT);
    FilterBatchBuilder b{FilterKind::kBloom, 10, 0};
    b.add_leaf(1, 100);
    EXPECT(b.verify(some, 16, nullptr, some, r).code == TKV_AMQ_INVALID_ARGUMENT);  // (not planned)
    EXPECT(tkv_amq_verify_members_ws_bytes(0) >= 16);
    std::printf("%s (no device; %d failures)\n", failures ? "FAIL" : "NODEVICE-OK", failures);
    return failures ? 1 : 0;
  }

  // leaves 0 and 3 have the same geometry (their payloads are swapped below)
  const std::vector<u64> counts{3000, 0, 5, 3000, 9000, 1};
  const u32 kKeyLen = 16, n_leaves = (u32)counts.size();
  u64 total_keys = 0;
  std::vector<u64> csr{0};
  std::vector<u32> own;  // the leaf of every key
  for (u32 l = 0; l < n_leaves; ++l) {
    total_keys += counts[l];
    csr.push_back(total_keys);
    own.insert(own.end(), counts[l], l);
  }
  uint64_t rs = 91;
  auto rnd = [&rs] {
    rs ^= rs << 13;
    rs ^= rs >> 7;
    rs ^= rs << 17;
    return rs;
  };
  std::string blob(total_keys * kKeyLen, '\0');
  for (auto& c : blob) c = (char)rnd();
  DeviceBuffer d_keys(blob.size()), d_own(4 * total_keys), d_res(total_keys), d_csr(8 * csr.size());
  EXPECT(hipMemcpy(d_keys.get(), blob.data(), blob.size(), hipMemcpyHostToDevice) == hipSuccess);
  EXPECT(hipMemcpy(d_own.get(), own.data(), 4 * total_keys, hipMemcpyHostToDevice) == hipSuccess);
  EXPECT(hipMemcpy(d_csr.get(), csr.data(), 8 * csr.size(), hipMemcpyHostToDevice) == hipSuccess);

  for (FilterKind kind : {FilterKind::kBloom, FilterKind::kQuotient}) {
    const usize bpk = kind == FilterKind::kBloom ? 10 : 12;
    const usize hdr = kind == FilterKind::kBloom ? 64 : 80;
    FilterBatchBuilder b{kind, bpk, 32704};
    for (u32 l = 0; l < n_leaves; ++l) b.add_leaf(500 + l, counts[l]);
    EXPECT(b.plan().ok());
    DeviceBuffer d_out(b.total_out_bytes());
    EXPECT(hipMemset(d_out.get(), 0, b.total_out_bytes()) == hipSuccess);
    EXPECT(b.build_all(d_keys.get(), kKeyLen, nullptr, d_out.get()).ok());
    EXPECT(b.check().ok());

    // every key against its own leaf through tkv_amq_probe: the per-leaf rejects and the first
    auto by_probe = [&](const u8* d_filters, const tkv_amq_segment* d_segs) {
      std::vector<u8> r(total_keys, 0xEE);
      EXPECT(tkv_amq_probe((int)kind, d_filters, d_segs, n_leaves, d_keys.get(), nullptr, kKeyLen, total_keys,
                           d_own.get<u32>(), d_res.get(), nullptr) == TKV_AMQ_OK);
      EXPECT(hipMemcpy(r.data(), d_res.get(), total_keys, hipMemcpyDeviceToHost) == hipSuccess);
      std::vector<tkv_amq_member_check> want(n_leaves, tkv_amq_member_check{~u64{0}, 0, 0});
      for (u64 i = 0; i < total_keys; ++i)
        if (r[i] == 0) {
          if (want[own[i]].missing++ == 0) want[own[i]].first_missing = i;
        }
      return want;
    };
    auto same = [&](const std::vector<tkv_amq_member_check>& got, const std::vector<tkv_amq_member_check>& want) {
      bool ok = got.size() == want.size();
      for (usize l = 0; ok && l < got.size(); ++l)
        ok = got[l].missing == want[l].missing && got[l].first_missing == want[l].first_missing;
      return ok;
    };

    // clean: nothing missing, no flag
    std::vector<tkv_amq_member_check> got;
    EXPECT(b.verify(d_keys.get(), kKeyLen, nullptr, d_out.get(), got).ok());
    EXPECT(got.size() == n_leaves);
    for (const auto& m : got) EXPECT(m.missing == 0 && m.first_missing == ~u64{0} && m.flags == 0);
    EXPECT(same(got, by_probe(d_out.get(), b.device_segments())));

    // damaged: the first half of leaf 4's blocks zeroed, the payloads of leaves 0 and 3 swapped
    std::vector<u8> host(b.total_out_bytes());
    EXPECT(hipMemcpy(host.data(), d_out.get(), host.size(), hipMemcpyDeviceToHost) == hipSuccess);
    const auto& g = b.segments();
    EXPECT(g[0].n_blocks == g[3].n_blocks && g[0].payload_bytes == g[3].payload_bytes);
    std::memset(host.data() + g[4].out_offset + hdr, 0, 64 * usize{g[4].n_blocks / 2});
    std::vector<u8> p0(host.begin() + g[0].out_offset, host.begin() + g[0].out_offset + g[0].payload_bytes);
    std::memcpy(host.data() + g[0].out_offset, host.data() + g[3].out_offset, g[3].payload_bytes);
    std::memcpy(host.data() + g[3].out_offset, p0.data(), p0.size());
    DeviceBuffer d_bad(host.size());
    EXPECT(hipMemcpy(d_bad.get(), host.data(), host.size(), hipMemcpyHostToDevice) == hipSuccess);
    const std::vector<tkv_amq_member_check> want = by_probe(d_bad.get(), b.device_segments());
    EXPECT(want[4].missing > 2000 && want[0].missing > 2700 && want[3].missing > 2700);  // (the precondition)
    u64 total = 0, sum = 0;
    for (u32 hint : {0u, 1u}) {
      EXPECT(verify_members(kind, d_bad.get(), b.device_segments(), n_leaves, hint, d_keys.get(), kKeyLen, nullptr,
                            total_keys, nullptr, got, &total).ok());
      EXPECT(same(got, want));
      sum = 0;
      for (u32 l = 0; l < n_leaves; ++l) {
        sum += got[l].missing;
        EXPECT(got[l].flags == ((l == 0 || l == 3) ? TKV_AMQ_VERIFY_ID_MISMATCH : 0u));
      }
      EXPECT(total == sum);
    }
    EXPECT(got[1].missing == 0 && got[2].missing == 0 && got[5].missing == 0);

    // the opened segments (key_begin 0) with the key CSR
    std::vector<u64> offs;
    for (const auto& sg : g) offs.push_back(sg.out_offset);
    DeviceBuffer d_offs(8 * offs.size());
    EXPECT(hipMemcpy(d_offs.get(), offs.data(), 8 * offs.size(), hipMemcpyHostToDevice) == hipSuccess);
    FilterLocation where;
    where.d_offsets = d_offs.get<u64>();
    OpenedFilterPages o;
    EXPECT(open_filter_pages(kind, d_out.get(), b.total_out_bytes(), where, n_leaves, o).ok());
    EXPECT(o.all_ok());
    EXPECT(verify_members(kind, d_out.get(), o.device_segments(), n_leaves, 0, d_keys.get(), kKeyLen, nullptr,
                          total_keys, d_csr.get<u64>(), got, &total).ok());
    EXPECT(total == 0);
    for (const auto& m : got) EXPECT(m.missing == 0 && m.flags == 0);
  }
  std::printf("%s (%d failures)\n", failures ? "FAIL" : "OK", failures);
  return failures ? 1 : 0;
}
