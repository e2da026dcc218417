// open_filter_pages / scan_filters of the header-only host mirror
// (include/turtle_kv_amd/filter_builder.hpp) over libtkv_amq.so: one Bloom and one VQF batch
// built through FilterBatchBuilder, opened again from the bytes alone (offsets and page images),
// probed through the opened segments, corrupted and refused, and scanned against counts the
// host takes from the bytes.  Exits non-zero on any failed expectation; without a device prints
// NODEVICE-OK.
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

static u64 rd64(const std::vector<u8>& b, usize off)
{
  u64 v;
  std::memcpy(&v, b.data() + off, 8);
  return v;
}

// what the scan must report for one payload, counted on the host from its bytes
static tkv_amq_filter_stats host_stats(FilterKind kind, const std::vector<u8>& b, const tkv_amq_segment& g)
{
  tkv_amq_filter_stats st{};
  const usize p = g.out_offset;
  if (kind == FilterKind::kBloom) {
    st.header_items = rd64(b, p + 48);
    for (u32 blk = 0; blk < g.n_blocks; ++blk) {
      u32 c = 0;
      for (u32 w = 0; w < 8; ++w) c += (u32)__builtin_popcountll(rd64(b, p + 64 + 64 * usize{blk} + 8 * w));
      st.occupied += c;
      st.full_blocks += c == 512;
      st.empty_blocks += c == 0;
      if (c > st.max_block) st.max_block = c;
    }
    return st;
  }
  st.header_items = rd64(b, p + 64);  // nelts
  const int T = g.tag_bits, W = T == 8 ? 128 : 64, B = T == 8 ? 80 : 36, S = T == 8 ? 48 : 28;
  for (u32 blk = 0; blk < g.n_blocks; ++blk) {
    const u8* blkp = b.data() + p + 80 + 64 * usize{blk};
    int pop = 0, sel = -1;
    for (int i = 0; i < W; ++i)
      if ((blkp[i / 8] >> (i % 8)) & 1) {
        if (++pop == B) sel = i;
      }
    const int occ = sel < 0 ? -1 : sel - (B - 1);
    if (occ < 0 || occ > S) {
      ++st.bad_blocks;
      continue;
    }
    bool bad = pop != (occ == 0 ? W - 1 : W - occ);
    for (int sl = occ; sl < S; ++sl)
      for (int k = 0; k < T / 8; ++k) bad |= blkp[W / 8 + sl * (T / 8) + k] != 0;
    st.bad_blocks += bad;
    st.occupied += (u64)occ;
    st.full_blocks += occ == S;
    st.empty_blocks += occ == 0;
    if ((u32)occ > st.max_block) st.max_block = (u32)occ;
  }
  return st;
}

static bool same_stats(const tkv_amq_filter_stats& a, const tkv_amq_filter_stats& b)
{
  return a.occupied == b.occupied && a.header_items == b.header_items && a.full_blocks == b.full_blocks &&
         a.empty_blocks == b.empty_blocks && a.max_block == b.max_block && a.bad_blocks == b.bad_blocks;
}

static bool same_segment(const tkv_amq_segment& a, const tkv_amq_segment& b)
{
  return a.out_offset == b.out_offset && a.n_blocks == b.n_blocks && a.hash_count == b.hash_count &&
         a.tag_bits == b.tag_bits && a.hash_val_shift == b.hash_val_shift && a.mod_magic == b.mod_magic &&
         a.src_page_id == b.src_page_id && a.payload_bytes == b.payload_bytes && a.page_flags == b.page_flags &&
         a.bits_per_key == 0 && a.key_begin == 0 && a.block_base == 0;
}

int main()
{
  if (tkv_amq_device_count() == 0) {
    // no GPU: the device path must fail loudly, bad arguments first
    OpenedFilterPages o;
    FilterLocation where;
    where.stride = 64;
    EXPECT(open_filter_pages(FilterKind::kBloom, nullptr, 0, where, 0, o).code == TKV_AMQ_UNAVAILABLE);
    where.page_size_log2 = 12;
    EXPECT(open_filter_pages(FilterKind::kBloom, nullptr, 0, where, 0, o).code == TKV_AMQ_INVALID_ARGUMENT);
    std::vector<tkv_amq_filter_stats> st;
    EXPECT(scan_filters(FilterKind::kQuotient, nullptr, nullptr, 0, st).code == TKV_AMQ_UNAVAILABLE);
    EXPECT(tkv_amq_scan_filters_ws_bytes(0) >= 16);
    std::printf("%s (no device; %d failures)\n", failures ? "FAIL" : "NODEVICE-OK", failures);
    return failures ? 1 : 0;
  }

  const std::vector<u64> counts{3000, 0, 5, 9000, 1};
  const u32 kKeyLen = 16, n_leaves = (u32)counts.size();
  u64 total_keys = 0;
  for (u64 c : counts) total_keys += c;
  uint64_t rs = 77;
  auto rnd = [&rs] {
    rs ^= rs << 13;
    rs ^= rs >> 7;
    rs ^= rs << 17;
    return rs;
  };
  std::string blob(total_keys * kKeyLen, '\0'), miss(2000 * kKeyLen, '\0');
  for (auto& c : blob) c = (char)rnd();
  for (auto& c : miss) c = (char)rnd();
  // queries: every third built key against its own leaf, then the misses round-robin
  std::string qbytes;
  std::vector<u32> qleaf;
  {
    u64 k = 0;
    for (u32 l = 0; l < n_leaves; ++l)
      for (u64 i = 0; i < counts[l]; ++i, ++k)
        if (k % 3 == 0) {
          qbytes.append(blob, k * kKeyLen, kKeyLen);
          qleaf.push_back(l);
        }
  }
  const usize n_hits = qleaf.size();
  for (u32 i = 0; i < 2000; ++i) {
    qbytes.append(miss, usize{i} * kKeyLen, kKeyLen);
    qleaf.push_back(i % n_leaves);
  }
  const usize nq = qleaf.size();
  DeviceBuffer d_keys(blob.size()), d_q(qbytes.size()), d_qleaf(4 * nq), d_res(nq);
  EXPECT(hipMemcpy(d_keys.get(), blob.data(), blob.size(), hipMemcpyHostToDevice) == hipSuccess);
  EXPECT(hipMemcpy(d_q.get(), qbytes.data(), qbytes.size(), hipMemcpyHostToDevice) == hipSuccess);
  EXPECT(hipMemcpy(d_qleaf.get(), qleaf.data(), 4 * nq, hipMemcpyHostToDevice) == hipSuccess);
  auto probe = [&](FilterKind kind, const u8* d_filters, const tkv_amq_segment* d_segs) {
    std::vector<u8> r(nq, 0xEE);
    EXPECT(tkv_amq_probe((int)kind, d_filters, d_segs, n_leaves, d_q.get(), nullptr, kKeyLen, nq,
                         d_qleaf.get<u32>(), d_res.get(), nullptr) == TKV_AMQ_OK);
    EXPECT(hipMemcpy(r.data(), d_res.get(), nq, hipMemcpyDeviceToHost) == hipSuccess);
    return r;
  };

  for (FilterKind kind : {FilterKind::kBloom, FilterKind::kQuotient}) {
    const usize bpk = kind == FilterKind::kBloom ? 10 : 12;
    for (int pages = 0; pages < 2; ++pages) {
      FilterBatchBuilder b = pages ? FilterBatchBuilder::pages(kind, bpk, 15) : FilterBatchBuilder{kind, bpk, 32704};
      for (u32 l = 0; l < n_leaves; ++l) b.add_leaf(500 + l, counts[l]);
      EXPECT(b.plan().ok());
      DeviceBuffer d_out(b.total_out_bytes());
      EXPECT(hipMemset(d_out.get(), 0, b.total_out_bytes()) == hipSuccess);
      EXPECT(b.build_all(d_keys.get(), kKeyLen, nullptr, d_out.get()).ok());
      EXPECT(b.check().ok());
      std::vector<u8> host(b.total_out_bytes());
      EXPECT(hipMemcpy(host.data(), d_out.get(), host.size(), hipMemcpyDeviceToHost) == hipSuccess);

      // open from the bytes alone
      std::vector<u64> offs;
      for (const auto& g : b.segments()) offs.push_back(g.out_offset);
      DeviceBuffer d_offs(8 * offs.size());
      EXPECT(hipMemcpy(d_offs.get(), offs.data(), 8 * offs.size(), hipMemcpyHostToDevice) == hipSuccess);
      FilterLocation where;
      if (pages) where.page_size_log2 = 15;
      else where.d_offsets = d_offs.get<u64>();
      OpenedFilterPages o;
      EXPECT(open_filter_pages(kind, d_out.get(), host.size(), where, n_leaves, o).ok());
      EXPECT(o.all_ok() && o.summary[TKV_AMQ_OPEN_OK] == n_leaves);
      for (u32 l = 0; l < n_leaves; ++l) {
        EXPECT(o.status[l] == TKV_AMQ_OPEN_OK);
        EXPECT(same_segment(o.segments[l], b.segments()[l]));
        EXPECT(o.segments[l].n_keys == counts[l]);  // (no leaf here is truncated by hash_val_shift)
      }
      // the probes answer alike through the opened and the planned segments; no false negatives
      const std::vector<u8> planned = probe(kind, d_out.get(), b.device_segments());
      const std::vector<u8> opened = probe(kind, d_out.get(), o.device_segments());
      EXPECT(planned == opened);
      usize rejected = 0;
      for (usize i = 0; i < nq; ++i) {
        if (i < n_hits) EXPECT(opened[i] == 1);
        else rejected += opened[i] == 0;
      }
      EXPECT(rejected > 1800);

      // scan: the host's counts from the same bytes
      std::vector<tkv_amq_filter_stats> st;
      EXPECT(scan_filters(kind, d_out.get(), o.device_segments(), n_leaves, st).ok());
      for (u32 l = 0; l < n_leaves; ++l) {
        const tkv_amq_filter_stats want = host_stats(kind, host, b.segments()[l]);
        EXPECT(same_stats(st[l], want));
        EXPECT(st[l].bad_blocks == 0 && st[l].header_items == counts[l]);
        if (kind == FilterKind::kQuotient) EXPECT(st[l].occupied == counts[l]);
        EXPECT(filter_fill(o.segments[l], st[l]) <= 1.0);
      }
      if (pages) continue;

      // refusal: leaf 3's magic zeroed -> BAD_MAGIC for it alone; it then cannot reject
      std::vector<u8> bad = host;
      std::memset(bad.data() + offs[3], 0, 8);
      DeviceBuffer d_bad(bad.size());
      EXPECT(hipMemcpy(d_bad.get(), bad.data(), bad.size(), hipMemcpyHostToDevice) == hipSuccess);
      OpenedFilterPages ob;
      EXPECT(open_filter_pages(kind, d_bad.get(), bad.size(), where, n_leaves, ob).ok());
      EXPECT(!ob.all_ok() && ob.summary[TKV_AMQ_OPEN_BAD_MAGIC] == 1 && ob.summary[TKV_AMQ_OPEN_OK] == n_leaves - 1);
      for (u32 l = 0; l < n_leaves; ++l) EXPECT(ob.status[l] == (l == 3 ? TKV_AMQ_OPEN_BAD_MAGIC : TKV_AMQ_OPEN_OK));
      EXPECT(ob.segments[3].hash_count == 0 && ob.segments[3].tag_bits == 0 && ob.segments[3].out_offset == offs[3]);
      const std::vector<u8> refused = probe(kind, d_bad.get(), ob.device_segments());
      for (usize i = 0; i < nq; ++i) EXPECT(refused[i] == (qleaf[i] == 3 ? 1 : opened[i]));
      // a truncated buffer: the last filter no longer fits
      OpenedFilterPages ot;
      EXPECT(open_filter_pages(kind, d_out.get(), offs[n_leaves - 1] + 40, where, n_leaves, ot).ok());
      EXPECT(ot.status[n_leaves - 1] == TKV_AMQ_OPEN_OUT_OF_BOUNDS && ot.summary[TKV_AMQ_OPEN_OK] == n_leaves - 1);

      if (kind == FilterKind::kQuotient) {
        // a block of leaf 3 with 0 < occ < 48: clearing its top metadata bit breaks popcount == W - occ
        const tkv_amq_segment& g = b.segments()[3];
        u32 blk = 0;
        for (; blk < g.n_blocks; ++blk) {
          const usize at = g.out_offset + 80 + 64 * usize{blk};
          const int zeros = 128 - __builtin_popcountll(rd64(host, at)) - __builtin_popcountll(rd64(host, at + 8));
          if (zeros > 1 && zeros < 48) break;
        }
        EXPECT(blk < g.n_blocks);
        std::vector<u8> flip = host;
        flip[g.out_offset + 80 + 64 * usize{blk} + 15] ^= 0x80;
        EXPECT(hipMemcpy(d_bad.get(), flip.data(), flip.size(), hipMemcpyHostToDevice) == hipSuccess);
        std::vector<tkv_amq_filter_stats> sf;
        EXPECT(scan_filters(kind, d_bad.get(), b.device_segments(), n_leaves, sf).ok());
        for (u32 l = 0; l < n_leaves; ++l) {
          EXPECT(same_stats(sf[l], host_stats(kind, flip, b.segments()[l])));
          EXPECT(sf[l].bad_blocks == (l == 3 ? 1u : 0u));
        }
      }
    }
  }
  std::printf("%s (%d failures)\n", failures ? "FAIL" : "OK", failures);
  return failures ? 1 : 0;
}
