// tkv_amq_lds_stride.h -- the strided LDS image of the Bloom leaf builds.
//
// A Bloom block is 16 words; a bit index (0..511) has its word in bits 5..8 and the bit of that
// word in bits 0..4.  In the canonical image word w of block b is at byte 64 * b + 4 * w, so the
// word number has to be extracted and scaled (bits 5..8 -> address bits 2..5).  In the strided
// image the words of a block are 32 bytes apart, so the word number sits at address bits 5..8,
// where the bit index already has it: a bit's address is one bit-field insert of the bit index
// into a per-key base.  Blocks are grouped 8 to a 512-byte region, the 8 blocks' words w side by
// side (4 bytes each) in the region's 32-byte row w:
//
//   byte of (block b, word w) = (b >> 3) * 512 + w * 32 + (b & 7) * 4
//
// An image of nb blocks takes ceil(nb / 8) regions: for nb a multiple of 8 exactly the canonical
// image's bytes.  The layout is private to a kernel: what leaves LDS is canonical.
// Plain constexpr functions, shared by the kernels, the host's LDS sizing and tests/cpp.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TKV_STRIDE_FN __host__ __device__ constexpr
#else
#define TKV_STRIDE_FN constexpr
#endif

namespace tkv {

constexpr uint32_t kStrideRegionBlocks = 8;    // blocks per region
constexpr uint32_t kStrideRegionBytes = 512;   // 8 blocks x 64 bytes; the image base's alignment
constexpr uint32_t kStrideWordBytes = 32;      // between two words of one block
constexpr uint32_t kStrideWordMask = 0x1e0;    // address bits 5..8: the word (= a bit index's bits 5..8)
constexpr uint32_t kStrideSlotMask = 0x1c;     // address bits 2..4: the block's slot in its region

// bytes (and 4-byte words) of the strided image of nb blocks
TKV_STRIDE_FN uint32_t lds_stride_bytes(uint32_t nb) { return ((nb + 7u) >> 3) * kStrideRegionBytes; }
TKV_STRIDE_FN uint32_t lds_stride_words(uint32_t nb) { return lds_stride_bytes(nb) / 4u; }
// the same for a launch's dynamic LDS, from a block count of any width
TKV_STRIDE_FN uint64_t lds_stride_bytes64(uint64_t nb) { return ((nb + 7u) >> 3) * kStrideRegionBytes; }

// byte offset of word 0 of local block b; bits 5..8 are zero
TKV_STRIDE_FN uint32_t lds_stride_block(uint32_t b) { return ((b >> 3) << 9) | ((b & 7u) << 2); }
// byte offset of word w (0..15) of local block b
TKV_STRIDE_FN uint32_t lds_stride_addr(uint32_t b, uint32_t w) { return lds_stride_block(b) | (w << 5); }
// byte offset of bit index `bit` of local block b (bits above 8 of `bit` are ignored)
TKV_STRIDE_FN uint32_t lds_stride_bit_addr(uint32_t b, uint32_t bit)
{
  return (lds_stride_block(b) & ~kStrideWordMask) | (bit & kStrideWordMask);
}

// the inverse: the block and the word at byte offset a
TKV_STRIDE_FN uint32_t lds_stride_block_of(uint32_t a) { return ((a >> 9) << 3) | ((a >> 2) & 7u); }
TKV_STRIDE_FN uint32_t lds_stride_word_of(uint32_t a) { return (a >> 5) & 15u; }

// The write-out: quad q of the canonical image (16 bytes: words 4 * (q & 3) .. + 3 of block
// q >> 2) is the four words at lds_stride_quad(q) + i * kStrideWordBytes, i = 0..3.
TKV_STRIDE_FN uint32_t lds_stride_quad(uint32_t q) { return lds_stride_addr(q >> 2, 4u * (q & 3u)); }

}  // namespace tkv
