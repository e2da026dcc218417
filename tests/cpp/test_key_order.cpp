// The order of two keys (turtle_kv_amd/csrc/tkv_amq_key_order.h) on the host, under
// AddressSanitizer and UBSan: key_compare against std::string_view's order, the 16- and 24-byte
// fast modes against the any-shape mode, bound() against std::lower_bound / std::upper_bound, the
// mode chooser, and leaf_key_range's clamping.  Every key (or fixed-stride key array) is a heap
// allocation of exactly its length, so a read past a key's end is an error.  Exits non-zero on any
// failed expectation.
#include <tkv_amq_key_order.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <string_view>
#include <vector>

using namespace tkv;

static int failures = 0;
#define EXPECT(c)                                                   \
  do {                                                              \
    if (!(c)) {                                                     \
      std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
      ++failures;                                                   \
    }                                                               \
  } while (0)

// `s` at the end of an allocation of exactly align + size bytes: the key starts `align` bytes past
// malloc's 16-byte alignment and ends where the allocation ends
struct HeapKey {
  uint8_t* block;
  uint8_t* p;
  uint32_t len;
  HeapKey(const std::string& s, uint32_t align) : len((uint32_t)s.size())
  {
    block = static_cast<uint8_t*>(std::malloc(align + s.size() ? align + s.size() : 1));
    p = block + align;
    if (!s.empty()) std::memcpy(p, s.data(), s.size());
  }
  HeapKey(const HeapKey&) = delete;
  ~HeapKey() { std::free(block); }
};

static int sign(int x) { return x < 0 ? -1 : x > 0 ? 1 : 0; }

static int sv_order(const std::string& a, const std::string& b)
{
  return sign(std::string_view(a).compare(std::string_view(b)));
}

// about 200 keys of lengths 0..20: a common stem cut at every length 0..20, and for every length
// 1..20 the stem's prefix with its last byte replaced by each of the edge values
static std::vector<std::string> compare_keys()
{
  std::string stem;
  for (int i = 0; i < 20; ++i) stem.push_back((char)(0x41 + 7 * i));
  std::vector<std::string> keys;
  for (size_t n = 0; n <= 20; ++n) keys.push_back(stem.substr(0, n));
  const uint8_t last[] = {0x00, 0x01, 0x7f, 0x80, 0xfe, 0xff, 0x42, 0xc3, 0x10};
  for (size_t n = 1; n <= 20; ++n)
    for (uint8_t v : last) {
      std::string k = stem.substr(0, n);
      k[n - 1] = (char)v;
      keys.push_back(k);
    }
  return keys;
}

static void test_key_compare()
{
  const std::vector<std::string> keys = compare_keys();
  EXPECT(keys.size() >= 200);
  // (left alignment ak with right alignment (3 ak + 5) & 7: every alignment 0..7 occurs on both sides)
  for (uint32_t ak = 0; ak < 8; ++ak) {
    std::vector<std::unique_ptr<HeapKey>> left, right;
    const uint32_t aq = (ak * 3 + 5) & 7;
    for (const std::string& s : keys) {
      left.emplace_back(new HeapKey(s, ak));
      right.emplace_back(new HeapKey(s, aq));
    }
    for (size_t i = 0; i < keys.size(); ++i)
      for (size_t j = 0; j < keys.size(); ++j) {
        const int want = sv_order(keys[i], keys[j]);
        EXPECT(sign(key_compare(left[i]->p, left[i]->len, right[j]->p, right[j]->len)) == want);
        EXPECT(sign(key_compare(left[i]->p, left[i]->len, left[j]->p, left[j]->len)) == want);
      }
  }
}

// fixed-length keys that differ in the last (and the first) byte of each 8-byte word, and in nothing
static std::vector<std::string> fixed_keys(size_t len)
{
  std::string base;
  for (size_t i = 0; i < len; ++i) base.push_back((char)(0x60 + i));
  std::vector<std::string> keys{base};
  for (size_t w = 0; w < len / 8; ++w)
    for (size_t at : {8 * w, 8 * w + 7})
      for (uint8_t v : {0x00, 0x7f, 0x80, 0xff}) {
        std::string k = base;
        k[at] = (char)v;
        keys.push_back(k);
      }
  std::string lo(len, '\0'), hi(len, '\xff');
  keys.push_back(lo);
  keys.push_back(hi);
  return keys;
}

template <int MODE>
static void test_fast_mode(uint32_t len)
{
  const std::vector<std::string> keys = fixed_keys(len);
  std::vector<std::unique_ptr<HeapKey>> heap;
  for (const std::string& s : keys) heap.emplace_back(new HeapKey(s, 0));
  for (size_t qi = 0; qi < keys.size(); ++qi) {
    const KeyArray qs{heap[qi]->p, nullptr, len};
    const OrderedQuery<MODE> fast(qs, 0);
    const OrderedQuery<kOrderAny> any(qs, 0);
    for (size_t ki = 0; ki < keys.size(); ++ki) {
      const KeyArray ks{heap[ki]->p, nullptr, len};
      const int want = sv_order(keys[ki], keys[qi]);
      EXPECT(any.less(ks, 0) == (want < 0) && any.less_equal(ks, 0) == (want <= 0) && any.equal(ks, 0) == (want == 0));
      EXPECT(fast.less(ks, 0) == any.less(ks, 0));
      EXPECT(fast.less_equal(ks, 0) == any.less_equal(ks, 0));
      EXPECT(fast.equal(ks, 0) == any.equal(ks, 0));
    }
  }
}

// bound() over sorted arrays of every length 0..70 with duplicates, in one allocation of exactly
// the array's bytes: stride form for all three modes, offsets form for kOrderAny
template <int MODE>
static void test_bound(uint32_t len, bool offsets_form)
{
  for (uint32_t n = 0; n <= 70; ++n) {
    // element j has value j / 3 * 2 + 1 (runs of three equal keys, odd values), big-endian in its last bytes
    std::vector<std::string> sorted;
    for (uint32_t j = 0; j < n; ++j) {
      std::string k(len, '\x55');
      const uint32_t v = j / 3 * 2 + 1;
      k[len - 1] = (char)(v & 0xff);
      k[len - 9] = (char)(v >> 1);  // the word before changes too
      sorted.push_back(k);
    }
    EXPECT(std::is_sorted(sorted.begin(), sorted.end()));
    uint8_t* arr = static_cast<uint8_t*>(std::malloc(n * len ? n * len : 1));
    std::vector<uint64_t> offs(n + 1);
    for (uint32_t j = 0; j < n; ++j) std::memcpy(arr + j * len, sorted[j].data(), len);
    for (uint32_t j = 0; j <= n; ++j) offs[j] = (uint64_t)j * len;
    const KeyArray ks{arr, offsets_form ? offs.data() : nullptr, offsets_form ? 0u : len};
    // queries: below all, above all, every element, and the even values between the runs
    std::vector<std::string> queries{std::string(len, '\0'), std::string(len, '\xff')};
    for (const std::string& s : sorted) queries.push_back(s);
    for (uint32_t v = 0; v <= n / 3 * 2 + 2; v += 2) {
      std::string k(len, '\x55');
      k[len - 1] = (char)(v & 0xff);
      k[len - 9] = (char)(v >> 1);
      queries.push_back(k);
    }
    for (const std::string& qk : queries) {
      const HeapKey hq(qk, 0);
      const OrderedQuery<MODE> q(KeyArray{hq.p, nullptr, len}, 0);
      const uint64_t lb = std::lower_bound(sorted.begin(), sorted.end(), qk) - sorted.begin();
      const uint64_t ub = std::upper_bound(sorted.begin(), sorted.end(), qk) - sorted.begin();
      // from a first index that is not 0, with the 64-bit and the 32-bit length of the two call sites
      for (uint64_t first : {(uint64_t)0, (uint64_t)(n / 2)}) {
        const uint64_t want_lb = std::max(lb, first), want_ub = std::max(ub, first);
        EXPECT(bound(first, (uint64_t)(n - first), [&](uint64_t k) { return q.less(ks, k); }) == want_lb);
        EXPECT(bound(first, (uint32_t)(n - first), [&](uint64_t k) { return q.less_equal(ks, k); }) == want_ub);
      }
    }
    std::free(arr);
  }
}

static void test_mode_chooser()
{
  alignas(16) static uint8_t qbuf[256], kbuf[256];
  const uint64_t offs[2] = {0, 16};
  auto mode = [&](uint32_t qoff, bool q_offsets, uint32_t qstride, uint32_t koff, bool k_offsets, uint32_t kstride) {
    return key_order_mode(KeyArray{qbuf + qoff, q_offsets ? offs : nullptr, qstride},
                          KeyArray{kbuf + koff, k_offsets ? offs : nullptr, kstride});
  };
  EXPECT(mode(0, false, 16, 0, false, 16) == kOrder16);
  EXPECT(mode(32, false, 16, 16, false, 16) == kOrder16);
  EXPECT(mode(8, false, 16, 0, false, 16) == kOrderAny);  // one side at +8
  EXPECT(mode(0, false, 16, 8, false, 16) == kOrderAny);
  EXPECT(mode(0, false, 24, 0, false, 24) == kOrder24);
  EXPECT(mode(8, false, 24, 24, false, 24) == kOrder24);  // 8-aligned
  EXPECT(mode(4, false, 24, 0, false, 24) == kOrderAny);  // 4-aligned
  EXPECT(mode(0, false, 24, 4, false, 24) == kOrderAny);
  EXPECT(mode(0, false, 20, 0, false, 20) == kOrderAny);
  EXPECT(mode(0, false, 16, 0, false, 24) == kOrderAny);  // the strides differ
  EXPECT(mode(0, true, 16, 0, false, 16) == kOrderAny);   // either side in offsets form
  EXPECT(mode(0, false, 16, 0, true, 16) == kOrderAny);
  EXPECT(mode(0, true, 0, 0, true, 0) == kOrderAny);
  EXPECT(mode(0, true, 24, 0, false, 24) == kOrderAny);
  EXPECT(mode(0, false, 24, 0, true, 24) == kOrderAny);
}

// both forms of the rule: the leaf's segment in its array, and a loaded copy of it
static void expect_range(const uint64_t* csr, const std::vector<tkv_amq_segment>& segs, uint32_t leaf,
                         uint64_t n_keys, uint64_t want_b, uint64_t want_e)
{
  uint64_t b = 77, e = 77;
  leaf_key_range(csr, segs.data(), leaf, n_keys, b, e);
  EXPECT(b == want_b && e == want_e);
  const tkv_amq_segment g = segs[leaf];
  b = e = 77;
  segment_key_range(csr, &g, leaf, n_keys, b, e);
  EXPECT(b == want_b && e == want_e);
}

static void test_leaf_key_range()
{
  const uint64_t n_keys = 30;
  std::vector<tkv_amq_segment> segs(7);
  std::memset(segs.data(), 0, segs.size() * sizeof(tkv_amq_segment));
  auto set = [&](uint32_t s, uint64_t kb, uint32_t nk) {
    segs[s].key_begin = kb;
    segs[s].n_keys = nk;
  };
  set(0, 3, 4);
  set(1, 25, 10);         // the end past n_keys
  set(2, 30, 1);          // the begin at n_keys
  set(3, 31, 0);          // the begin past n_keys
  set(4, ~0ull - 3, 10);  // key_begin + n_keys wraps past 2^64: the end reads as the largest
  set(5, ~0ull, 2);
  set(6, 29, 1);
  // CSR form, [n + 1] offsets: the segments' own ranges are not looked at
  const uint64_t csr[] = {0, 5, 5, 12, 9, 40, 100, 7};
  expect_range(csr, segs, 0, n_keys, 0, 5);
  expect_range(csr, segs, 1, n_keys, 5, 5);
  expect_range(csr, segs, 2, n_keys, 5, 12);
  expect_range(csr, segs, 3, n_keys, 12, 12);  // an end below its begin: empty at the begin
  expect_range(csr, segs, 4, n_keys, 9, 30);   // an end past n_keys
  expect_range(csr, segs, 5, n_keys, 30, 30);  // a begin past n_keys
  expect_range(csr, segs, 6, n_keys, 30, 30);  // a begin past n_keys, an end below it
  const uint64_t wrap[] = {~0ull - 1, 2};      // an end that wrapped: below its begin
  expect_range(wrap, segs, 0, n_keys, 30, 30);
  expect_range(wrap, segs, 0, ~0ull, ~0ull - 1, ~0ull - 1);
  // segment form
  expect_range(nullptr, segs, 0, n_keys, 3, 7);
  expect_range(nullptr, segs, 1, n_keys, 25, 30);
  expect_range(nullptr, segs, 2, n_keys, 30, 30);
  expect_range(nullptr, segs, 3, n_keys, 30, 30);
  expect_range(nullptr, segs, 4, n_keys, 30, 30);
  expect_range(nullptr, segs, 5, n_keys, 30, 30);
  expect_range(nullptr, segs, 6, n_keys, 29, 30);
  // (with every index a valid key the wrapped end is seen: it is the largest index, not a small one)
  expect_range(nullptr, segs, 4, ~0ull, ~0ull - 3, ~0ull);
  expect_range(nullptr, segs, 5, ~0ull, ~0ull, ~0ull);
  expect_range(nullptr, segs, 1, ~0ull, 25, 35);
  expect_range(nullptr, segs, 0, 0, 0, 0);  // no keys at all
}

static void test_key_array()
{
  const HeapKey h(std::string("abcdefghijkl"), 0);
  const uint64_t offs[] = {0, 0, 5, 12};
  const uint8_t* p;
  uint32_t len;
  const KeyArray o{h.p, offs, 0};
  o.at(0, p, len);
  EXPECT(p == h.p && len == 0);
  o.at(1, p, len);
  EXPECT(p == h.p && len == 5);
  o.at(2, p, len);
  EXPECT(p == h.p + 5 && len == 7);
  const KeyArray s{h.p, nullptr, 4};
  s.at(2, p, len);
  EXPECT(p == h.p + 8 && len == 4);
}

int main()
{
  test_key_compare();
  test_fast_mode<kOrder16>(16);
  test_fast_mode<kOrder24>(24);
  test_bound<kOrder16>(16, false);
  test_bound<kOrder24>(24, false);
  test_bound<kOrderAny>(16, false);
  test_bound<kOrderAny>(13, false);
  test_bound<kOrderAny>(24, true);
  test_mode_chooser();
  test_leaf_key_range();
  test_key_array();
  std::printf("%s (%d failures)\n", failures ? "FAIL" : "OK", failures);
  return failures ? 1 : 0;
}
