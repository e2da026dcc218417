// The strided LDS image of the Bloom leaf builds (turtle_kv_amd/csrc/tkv_amq_lds_stride.h), on the
// host: for images of 1..65 blocks, (block, word) -> address is injective, stays inside
// ceil(nb / 8) * 512 bytes and 4-byte aligned, carries the word in address bits 5..8, and the
// write-out's quad addresses return every (block, word) exactly once, in canonical order.  A bit's
// address, as the kernels form it (a bit-field insert of the bit index into the per-key base with
// don't-care bits 5..8), is the address of the bit's word.  Exits non-zero on any failed
// expectation.
#include <tkv_amq_lds_stride.h>

#include <cstdio>
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

// compile-time: the flagship's 320 blocks keep their 20,480 bytes; a part of a region takes a whole one
static_assert(lds_stride_bytes(320) == 320 * 64, "a multiple of 8 blocks takes the canonical image's bytes");
static_assert(lds_stride_bytes(1) == 512 && lds_stride_bytes(8) == 512 && lds_stride_bytes(9) == 1024, "whole regions");
static_assert(lds_stride_bytes64(2560) == 160 * 1024, "the LDS budget is a whole number of regions");
static_assert(lds_stride_addr(9, 3) == 512 + 3 * 32 + 4, "(b >> 3) * 512 + w * 32 + (b & 7) * 4");

int main()
{
  for (uint32_t nb = 1; nb <= 65; ++nb) {
    const uint32_t bytes = lds_stride_bytes(nb);
    EXPECT(bytes == (nb + 7) / 8 * 512);
    EXPECT(lds_stride_words(nb) * 4 == bytes);
    EXPECT(lds_stride_bytes64(nb) == bytes);
    if (nb % 8 == 0) EXPECT(bytes == nb * 64);
    std::vector<int> hit(bytes / 4, 0);
    for (uint32_t b = 0; b < nb; ++b) {
      for (uint32_t w = 0; w < 16; ++w) {
        const uint32_t a = lds_stride_addr(b, w);
        EXPECT(a == (b >> 3) * 512 + w * 32 + (b & 7) * 4);
        EXPECT(a < bytes && a % 4 == 0);
        if (a < bytes) EXPECT(hit[a / 4]++ == 0);  // injective
        EXPECT(((a >> 5) & 15) == w);              // the word at address bits 5..8
        EXPECT(lds_stride_block_of(a) == b && lds_stride_word_of(a) == w);
        // a bit of this word, with junk above its 9 bits, into a base whose bits 5..8 are junk
        // too, and the image at a region-aligned base
        for (uint32_t bit = 32 * w; bit < 32 * w + 32; bit += 31) {
          EXPECT(lds_stride_bit_addr(b, bit | 0xabcdee00u) == a);
          const uint32_t base = 17 * kStrideRegionBytes, junk = (b * 7 + w) & 15;
          const uint32_t x = base + (lds_stride_block(b) | (junk << 5));
          EXPECT(((x & ~kStrideWordMask) | (bit & kStrideWordMask)) == base + a);
        }
      }
      EXPECT((lds_stride_block(b) & kStrideWordMask) == 0);
      // the kernels' per-key base, from the block times four with anything in its low two bits:
      // the block at bit 6, the slot inserted at bits 2..4
      for (uint32_t frac = 0; frac < 4; ++frac) {
        const uint32_t b4 = 4 * b + frac, t = b4 << 4;
        const uint32_t x = (b4 & kStrideSlotMask) | (t & ~kStrideSlotMask);
        EXPECT((x & ~kStrideWordMask) == lds_stride_block(b));
      }
    }
    // the block times four straight from the hash: hi64(h0 * 4 nb) >> 2 == hi64(h0 * nb)
    uint64_t h0 = 0x9e3779b97f4a7c15ull * nb;
    for (int i = 0; i < 64; ++i, h0 = h0 * 6364136223846793005ull + 1442695040888963407ull) {
      const uint64_t hs[] = {h0, 0, ~0ull, ~0ull / nb, ~0ull / nb + 1, ~0ull / (4ull * nb) * 3 + 1};
      for (uint64_t h : hs) {
        const uint64_t blk = (uint64_t)(((unsigned __int128)h * nb) >> 64);
        const uint64_t b4 = (uint64_t)(((unsigned __int128)h * (4ull * nb)) >> 64);
        EXPECT((b4 >> 2) == blk && blk < nb);
      }
    }
    // the write-out: quad q is words 4 * (q & 3) .. + 3 of block q >> 2, 32 bytes apart
    std::vector<int> out(nb * 16, 0);
    for (uint32_t q = 0; q < nb * 4; ++q) {
      for (uint32_t i = 0; i < 4; ++i) {
        const uint32_t a = lds_stride_quad(q) + i * kStrideWordBytes;
        EXPECT(a < bytes);
        const uint32_t canon = 4 * q + i;  // word index of the canonical image
        EXPECT(lds_stride_block_of(a) == canon / 16 && lds_stride_word_of(a) == canon % 16);
        if (lds_stride_block_of(a) * 16 + lds_stride_word_of(a) < out.size())
          ++out[lds_stride_block_of(a) * 16 + lds_stride_word_of(a)];
      }
      // a lane's next quad, 256 / 512 / 1024 quads on, is that many * 16 bytes on
      for (uint32_t nt : {256u, 512u, 1024u}) EXPECT(lds_stride_quad(q + nt) == lds_stride_quad(q) + nt * 16);
    }
    for (int c : out) EXPECT(c == 1);
  }
  std::printf("%s (%d failures)\n", failures ? "FAIL" : "OK", failures);
  return failures ? 1 : 0;
}
