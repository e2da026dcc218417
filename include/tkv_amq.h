/*
 * tkv_amq.h -- C ABI of the MI355X-native AMQ filter engine for TurtleKV (libtkv_amq.so).
 *
 * This is the drop-in boundary for TurtleKV's per-leaf filter build/probe path.  Each
 * entry point names the reference interface it replaces (paths relative to the
 * mathworks/turtle_kv source tree):
 *
 *   tkv_amq_plan            build_{bloom,quotient}_filter_for_leaf sizing
 *                           (src/turtle_kv/tree/filter_builder.hpp:121-135, 241-290) and
 *                           TreeOptions::filter_bits_per_key (tree/tree_options.hpp:155-164)
 *   tkv_amq_build           build_filter_for_leaf_in_job (tree/filter_builder.hpp:307-331),
 *                           batched over every leaf of one TreeSerializeContext::build_all_pages
 *                           queue (tree/tree_serialize_context.cpp:62-115); per leaf it does what
 *                           build_bloom_filter_for_leaf (:109-152) or build_vqf_filter<T> (:176-217)
 *                           writes into the filter page payload
 *   tkv_amq_probe           KeyQuery::reject_page filter test (tree/key_query.hpp:149-247):
 *                           PackedBloomFilter::query (:216-219) / PackedVqfFilter::is_present
 *                           (vqf_filter_page_view.hpp:113-125); result 0 == "reject" (kTrue)
 *   tkv_amq_vqf_hash        vqf_hash_val (vqf_filter_page_view.hpp:32-35), hash-once per query
 *                           (tree/key_query.hpp:82)
 *   tkv_amq_vqf_probe_hashed PackedVqfFilter::is_present(hash_val) for pre-hashed queries
 *   tkv_amq_bloom_hash /    BloomFilterQuery<KeyView> hash cache (tree/key_query.hpp:78,97)
 *   tkv_amq_bloom_probe_hashed   and PackedBloomFilter::query on it (:219)
 *   tkv_amq_vqf_*sizing     vqf_filter_load_factor<T> (vqf_filter_page_view.hpp:39-59),
 *                           vqf_required_size<T> / vqf_nslots_for_size (vqf 0.2.4, used at
 *                           tree/filter_builder.hpp:243-244,270,274)
 *   tkv_amq_filter_page_size_log2, tkv_amq_expected_items_per_leaf, tkv_amq_leaf_data_size
 *                           TreeOptions::filter_page_size_log2 / expected_items_per_leaf /
 *                           leaf_data_size (tree/tree_options.hpp:177-258, tree_options.cpp:57-60,
 *                           tree/packed_leaf_page.hpp:307-311, core/packed_sizeof_edit.hpp:13-15)
 *   tkv_amq_bloom_route / tkv_amq_bloom_build_range (and their _records forms)
 *   tkv_amq_bloom_route_plan / _route_blocks / _build_part_blocks (the pipelined form)
 *                           one monolithic Bloom filter sharded by hash range over GPUs
 *                           (BASELINE config 5; the llfs build_bloom_filter_page it replaces is
 *                           called at tree/filter_builder.hpp:126-135)
 *   tkv_amq_plan_pages      FilterPageAlloc + the page header fields the builders set:
 *                           layout_id (filter_builder.hpp:237), unused_begin / unused_end
 *                           (:293-296), in one page-sized slot per leaf
 *   tkv_amq_probe_ex / tkv_amq_*_probe_hashed_ex
 *                           the same probes with KeyQuery::reject_page's page-id check
 *                           (tree/key_query.hpp:205-212,227-232) and KeyQuery::Metrics counters
 *                           (:36-60, updated at :154,157,210,231,243 and key_query.cpp:41,77)
 *   tkv_amq_path_probe      a batch of point lookups' walks over their segments (tree/algo/
 *                           nodes.hpp:158-187, segmented_levels.hpp:358-369): each key hashed
 *                           once, reject_page asked of every filter on its path, the leaves
 *                           still to search returned per query, in order
 *   tkv_amq_find_keys       the leaf search behind the filters (find_key_in_leaf_impl, tree/
 *                           key_query.cpp:27-80,299-327): a lower bound over each surviving
 *                           leaf's sorted keys, the walk ended at the first leaf that holds the
 *                           key (tree/algo/nodes.hpp:165-187), filter_false_positive_count (:76-78)
 *   tkv_amq_walk_paths      the tree descent in front of both (find_pivot_containing, tree/algo/
 *                           nodes.hpp:48-71; find_key, :158-187; for_each_active_segment_in,
 *                           tree/algo/segmented_levels.hpp:340-369): each lookup's ordered list of
 *                           leaves, with page ids, flushed item upper bounds (packed_node_page.cpp:
 *                           231-248) and (depth, level) per entry
 *   tkv_amq_get_keys        the three above in one call and in the reference's order: the point
 *                           lookup (NodeAlgorithms::find_key, tree/algo/nodes.hpp:158-187) for values
 *                           that need no combining, with two of its stopping rules -- the first
 *                           level that yields the key ends it, and an item found below a segment's
 *                           flushed item upper bound (SegmentAlgorithms::find_key, tree/algo/
 *                           segments.hpp:166-206) leaves the level -- and KeyQuery::Metrics over the
 *                           filters the reference asks
 *   tkv_amq_get_values      the same lookup with find_key's third rule, the value rule: each found
 *                           item's packed value (unpack_value_view, core/packed_key_value.hpp:18-23:
 *                           an op byte, then the data) is folded into the lookup's value as
 *                           combine_in_place folds it (core/value_view.hpp:316-361), and the lookup
 *                           goes on through older levels and the child while the value
 *                           needs_combine() (:279-285) -- OP_ADD_I32 deltas are summed until an
 *                           OP_WRITE or an OP_DELETE resolves them
 *   tkv_amq_gather_values   the resolved values' bytes, one fixed slot per lookup
 *   tkv_amq_merge_leaves    the leaf update, {BatchUpdate} + {PackedLeafPage} => leaf (tree/
 *                           subtree.cpp:170-191, 211-231): merge_compact_edits over the update's
 *                           edits (newer) and the leaf's items (older) -- the stable merge
 *                           (core/algo/merge_compact_edits.hpp:84-94), run_compact (core/algo/
 *                           parallel_compact.hpp:80-116) and keep_item (core/algo/decay_to_item.hpp:
 *                           14-46) -- batched over the leaves of one update, as 16-byte records
 *   tkv_amq_gather_merged   those records' keys and packed values, as the arrays tkv_amq_build and
 *                           tkv_amq_get_values take
 *   tkv_amq_merge_levels    merge_compact_edits over K levels (core/algo/merge_compact_edits.hpp:
 *                           26-148, one MergeCompactor::push_level per level): the node path's
 *                           merge, the incoming batch and every update-buffer level it collapses
 *                           (InMemoryNode::push_levels_to_merge, tree/in_memory_node.cpp:827-866),
 *                           up to 8 runs in one call, batched over key ranges, as the same records
 *   tkv_amq_gather_levels   tkv_amq_gather_merged over that table of runs
 *   tkv_amq_open_filters    what KeyQuery::reject_page reads from a loaded filter page instead
 *                           of a plan (tree/key_query.hpp:149-247): check_magic()
 *                           (vqf_filter_page_view.hpp:96-100), src_page_id, block_count,
 *                           hash_count, the VQF hash_mask and vqf_metadata -- for a batch of
 *                           stored payloads or page images, validated, as probe segments
 *   tkv_amq_scan_filters    no reference counterpart: a read-only scrub of the filter bytes
 *                           (set bits per Bloom filter, occupied slots and the block invariants
 *                           of vqf_init_in_place / vqf_insert per VQF)
 *   tkv_amq_verify_members  no reference counterpart: the property the reference's own test pins
 *                           (tree/in_memory_node.test.cpp:101-131, every key of a leaf passes
 *                           its filter), audited for a whole batch in one leaf-major pass
 *   tkv_amq_stage_keys      the EditView key range build_filter_for_leaf_in_job iterates
 *                           (core/merge_compactor.hpp:107-139) gathered into one contiguous
 *                           host key buffer for the H2D copy (host only)
 *
 * Conventions
 *  - Plain pointers and sizes only.  Pointers documented "device" are HIP device pointers
 *    (hipMalloc / framework-owned HBM); `stream` is a hipStream_t passed as void* (NULL =
 *    the default stream).  Launch functions never allocate, copy synchronously or
 *    synchronise, so they can be captured into a hipGraph.
 *  - The caller owns every buffer (the reference writes into a PageCache page buffer it
 *    does not own, tree/filter_builder.hpp:76-84,189-193).
 *  - Return values are status codes numbered like batt::StatusCode / absl::StatusCode.
 *    On error the output is undefined and must not be committed (reference: a failed build
 *    leaves the leaf without a filter, tree/filter_builder.hpp:323-325).
 *  - Thread-safe: no global mutable state; concurrent calls on different streams are fine.
 *  - Filter bit layouts follow the frozen "tkv-amq v1" spec.
 */
#ifndef TKV_AMQ_H
#define TKV_AMQ_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TKV_AMQ_ABI_VERSION 3

/* status codes (batt::StatusCode values) */
#define TKV_AMQ_OK 0
#define TKV_AMQ_INVALID_ARGUMENT 3
#define TKV_AMQ_RESOURCE_EXHAUSTED 8
#define TKV_AMQ_INTERNAL 13
#define TKV_AMQ_UNAVAILABLE 14

/* filter kinds (config.hpp:20-24 compile-time switch, made a runtime argument) */
#define TKV_AMQ_BLOOM 0
#define TKV_AMQ_VQF 1

/* One leaf's filter ("segment"), produced on the host by tkv_amq_plan and read by the
 * device kernels.  64 bytes, little-endian, no padding.  The first 32 bytes are what a
 * probe needs (two 16-byte loads). */
typedef struct tkv_amq_segment {
  uint64_t out_offset;    /* byte offset of the filter page payload in the output array */
  uint32_t n_blocks;      /* Bloom: 512-bit blocks; VQF: 64-byte vqf blocks */
  uint16_t hash_count;    /* Bloom k; VQF 0 */
  uint8_t tag_bits;       /* VQF 8 | 16; Bloom 0 */
  uint8_t hash_val_shift; /* VQF hash truncation (filter_builder.hpp:280-283) */
  uint64_t mod_magic;     /* VQF: floor((2^64-1) / (n_blocks * buckets_per_block)); Bloom: 0 */
  uint64_t key_begin;     /* first key index of this leaf's (sorted) item range */
  uint64_t src_page_id;   /* leaf PageId stored in the filter header (reject_page check) */
  uint64_t block_base;    /* prefix sum of n_blocks (VQF workspace addressing) */
  uint32_t n_keys;        /* items in the leaf (tombstones included) */
  uint32_t payload_bytes; /* bytes of payload the build writes (header + filter) */
  uint32_t bits_per_key;  /* effective bits/key after the TreeOptions clamp */
  uint32_t page_flags;    /* TKV_AMQ_PAGE_IMAGE | page_size_log2 << 8 (tkv_amq_plan_pages); 0 */
} tkv_amq_segment;

/* page_flags bit: the build also writes the 64-byte llfs PackedPageHeader fields the filter
 * builders set, at out_offset - 64 (the page starts there) */
#define TKV_AMQ_PAGE_IMAGE 0x1u

const char* tkv_amq_version(void);
const char* tkv_amq_status_string(int status);
/* number of visible HIP devices; 0 => every device entry point returns TKV_AMQ_UNAVAILABLE */
int tkv_amq_device_count(void);

/* TreeOptions::filter_bits_per_key(): VQF clamps any nonzero bpk to >= 12 */
uint64_t tkv_amq_filter_bits_per_key(int kind, uint64_t requested_bits_per_key);

double tkv_amq_vqf_load_factor(int tag_bits, uint64_t bits_per_key);
uint64_t tkv_amq_vqf_required_size(int tag_bits, uint64_t nslots);
uint64_t tkv_amq_vqf_nslots_for_size(int tag_bits, uint64_t bytes);

/* TreeOptions filter page sizing (tree/tree_options.hpp:177-258).
 *  leaf_size              TreeOptions::leaf_size() (default 2 MiB)
 *  key/value_size_hint    defaults 24 / 100 (tree_options.hpp:58-59)
 *  bits_per_key           as set (the VQF clamp of filter_bits_per_key() is applied here)
 * tkv_amq_filter_page_size_log2 returns the derived log2 page size (0 for VQF with bpk 0, where
 * the reference would divide by a zero load factor).  The filter page payload capacity the
 * builders see is (1 << log2) - 64 (the llfs PackedPageHeader). */
uint64_t tkv_amq_leaf_data_size(uint64_t leaf_size);
uint64_t tkv_amq_expected_items_per_leaf(uint64_t leaf_size, uint32_t key_size_hint,
                                         uint32_t value_size_hint);
uint32_t tkv_amq_filter_page_size_log2(int kind, uint64_t leaf_size, uint32_t key_size_hint,
                                       uint32_t value_size_hint, uint64_t bits_per_key);

/* Host-side plan for a batch of n_segs leaves.
 *  seg_key_counts[n_segs]  items per leaf (keys are laid out leaf after leaf)
 *  src_page_ids[n_segs]    leaf page ids (NULL => segment index)
 *  bits_per_key            as passed to build_filter_for_leaf_in_job (0 => no filters)
 *  payload_capacity        filter page payload bytes (page size - page header); 0 => unlimited
 *                          (VQF needs a capacity: it drives vqf_nslots_for_size)
 *  out_stride              0 => payloads packed back to back (64-byte aligned); otherwise each
 *                          segment s starts at s * out_stride (e.g. the filter page size)
 *  segs[n_segs]            (out) plan; upload it to the device before tkv_amq_build
 *  total_out_bytes         (out) size of the output array
 *  workspace_bytes         (out) device workspace tkv_amq_build needs (0 for Bloom)
 *  max_seg_blocks          (out) largest n_blocks of any segment (launch geometry) */
int tkv_amq_plan(int kind, const uint64_t* seg_key_counts, const uint64_t* src_page_ids,
                 uint32_t n_segs, uint32_t bits_per_key, uint64_t payload_capacity,
                 uint64_t out_stride, tkv_amq_segment* segs, uint64_t* total_out_bytes,
                 uint64_t* workspace_bytes, uint32_t* max_seg_blocks);

/* Plan whole filter pages: leaf s owns bytes [s << page_size_log2, (s+1) << page_size_log2) of
 * the output array, laid out as the page buffer FilterPageAlloc hands the builder
 * (filter_builder.hpp:70-88): a 64-byte PackedPageHeader, then the payload (capacity =
 * page size - 64, which drives the VQF sizing).  tkv_amq_build then also writes the header
 * fields the filter builders set -- layout_id ("vqf_filt", :237 / vqf_filter_page_view.hpp:142;
 * Bloom "bloomflt"), unused_begin = 64 + payload bytes, unused_end = page size (:293-296) --
 * and the page size.  Magic, page id and crc are the PageCache's (llfs) and are written as 0.
 * Header field offsets follow llfs 0.42's PackedPageHeader and are UNPINNED (llfs is absent).
 * Bytes between unused_begin and unused_end are not written. */
int tkv_amq_plan_pages(int kind, const uint64_t* seg_key_counts, const uint64_t* src_page_ids,
                       uint32_t n_segs, uint32_t bits_per_key, uint32_t page_size_log2,
                       tkv_amq_segment* segs, uint64_t* total_out_bytes, uint64_t* workspace_bytes,
                       uint32_t* max_seg_blocks);

/* Device build of every planned filter.
 *  keys         device; fixed-length keys (key_offsets == NULL: key i at keys + i*key_stride,
 *               length key_stride) or variable-length (key_offsets[n_keys+1], device)
 *  d_segs       device copy of the plan; max_seg_blocks as returned by tkv_amq_plan
 *  d_out        device output array (total_out_bytes)
 *  d_workspace  device workspace (workspace_bytes, 16-byte aligned)
 * Asynchronous on `stream`.  VQF insert failures (the reference BATT_CHECKs,
 * filter_builder.hpp:211) are recorded in the workspace; read them with
 * tkv_amq_build_check after the stream completes.  VQF workspace header (written by every
 * build, so no clearing is needed between builds): bytes [4, 8) = the build's n_segs; bytes
 * [64 + 4*s, 68 + 4*s) = leaf s's element count, with TKV_AMQ_VQF_FLAG_OVERFLOW set if one of
 * its inserts failed and TKV_AMQ_VQF_FLAG_WORKSPACE if the workspace was short (a caller may
 * copy these words back with its own results instead of calling tkv_amq_build_check). */
#define TKV_AMQ_VQF_NELTS_OFFSET 64u
#define TKV_AMQ_VQF_FLAG_OVERFLOW 0x80000000u
#define TKV_AMQ_VQF_FLAG_WORKSPACE 0x40000000u
int tkv_amq_build(int kind, const uint8_t* keys, const uint64_t* key_offsets,
                  uint32_t key_stride, uint64_t n_keys, const tkv_amq_segment* d_segs,
                  uint32_t n_segs, uint32_t max_seg_blocks, uint8_t* d_out,
                  void* d_workspace, uint64_t workspace_bytes, void* stream);

/* tkv_amq_build with the host copy of the plan's segments (h_segs: the n_segs entries
 * tkv_amq_plan filled; d_segs is their device copy).  With it a Bloom batch of 16- or 24-byte
 * keys builds its leaves of more than 5 LDS windows (images past 800 KB; tree/tree_options.hpp:
 * 177-215 sizes any leaf) through the tiled build, up to 40 of them per launch, and the other
 * leaves through the batch kernels; with other key shapes (variable-length, other strides) only
 * the leaves past 16 windows (2.5 MB) leave the batch kernels, each hashed into bit records by
 * a pass of its own and built by the tiled build (k <= 16, i.e. up to 23 bits/key, two records
 * per key above k = 8: the wide record below; from k = 17, device atomics); tkv_amq_build
 * of such a batch sets those leaves' bits with device atomics.  The workspace tkv_amq_plan
 * sizes covers either key shape.
 * h_segs == NULL, a single leaf, or a batch without such leaves: exactly tkv_amq_build. */
int tkv_amq_build_ex(int kind, const uint8_t* keys, const uint64_t* key_offsets, uint32_t key_stride,
                     uint64_t n_keys, const tkv_amq_segment* d_segs, const tkv_amq_segment* h_segs,
                     uint32_t n_segs, uint32_t max_blocks, uint8_t* d_out, void* d_workspace,
                     uint64_t workspace_bytes, void* stream);

/* The route a build takes ("Build routes").  Bloom: `route` is the batch's route.
 * VQF: `route` is the decide stage and `place` the place stage. */
#define TKV_AMQ_ROUTE_SPLIT 0u         /* Bloom: each leaf's keys over `parts` workgroups, merged */
#define TKV_AMQ_ROUTE_WINDOW 1u        /* Bloom: `windows` LDS windows per leaf, `parts` per window */
#define TKV_AMQ_ROUTE_LDS 2u           /* Bloom: one workgroup of `threads` per leaf */
#define TKV_AMQ_ROUTE_TILED_KEYS 3u    /* Bloom: one filter, tiled, from its 16- or 24-byte keys */
#define TKV_AMQ_ROUTE_TILED_RECORDS 4u /* Bloom: one filter, tiled, from hashed bit records */
#define TKV_AMQ_ROUTE_ATOMICS 5u       /* Bloom: device atomics */
#define TKV_AMQ_ROUTE_VQF_BIG_U8 16u      /* vqf_decide_big, u8 counts in LDS */
#define TKV_AMQ_ROUTE_VQF_BIG_GLOBAL 17u  /* vqf_decide_big, counts in the workspace */
#define TKV_AMQ_ROUTE_VQF_RING_PLACE 18u  /* vqf_ring_place, one workgroup per CU */
#define TKV_AMQ_ROUTE_VQF_RING_PLACE2 19u /* vqf_ring_place, two workgroups per CU */
#define TKV_AMQ_ROUTE_VQF_RING 20u        /* vqf_decide_ring */
#define TKV_AMQ_ROUTE_VQF_DECIDE 21u      /* vqf_decide */
#define TKV_AMQ_PLACE_NONE 0u      /* Bloom, or placed by the decide stage (vqf_ring_place) */
#define TKV_AMQ_PLACE_FUSED512 1u  /* vqf_place_fused, 512 threads */
#define TKV_AMQ_PLACE_FUSED256 2u  /* vqf_place_fused, 256 threads */
#define TKV_AMQ_PLACE_SCATTER 3u   /* vqf_scatter, then vqf_place */
/* tkv_amq_build_ex's leaves (leaf_route) */
#define TKV_AMQ_LEAF_BATCH 0u         /* in the compacted batch `out` describes */
#define TKV_AMQ_LEAF_MULTI 1u         /* tiled, in a multi-leaf launch */
#define TKV_AMQ_LEAF_TILED_KEYS 2u    /* tiled alone, from its keys */
#define TKV_AMQ_LEAF_TILED_RECORDS 3u /* tiled alone, from bit records */
#define TKV_AMQ_LEAF_ATOMICS 4u       /* device atomics */
#define TKV_AMQ_LEAF_NONE 5u          /* no filter (bits_per_key 0) */

struct tkv_amq_build_route { /* 40 bytes */
  uint32_t route;         /* TKV_AMQ_ROUTE_* */
  uint32_t place;         /* TKV_AMQ_PLACE_* */
  uint32_t parts;         /* workgroups per leaf (split), per window (window) or per leaf (place) */
  uint32_t windows;       /* LDS windows per leaf (window route), else 0 */
  uint32_t threads;       /* the build kernel's workgroup size (VQF: the decide stage's) */
  uint32_t located;       /* VQF: vqf_locate_keys runs ahead of vqf_ring_place */
  uint64_t ws_bytes;      /* the workspace the route needs */
  uint32_t lds_bytes;     /* Bloom: a workgroup's LDS image, 64 bytes a block (0: tiled, atomics; the
                             launch takes whole 512-byte regions of 8 blocks); VQF: the decide
                             stage's dynamic LDS */
  uint32_t reserved;
};

/* The route tkv_amq_build / tkv_amq_build_ex would take.  Pure host: no device needed.
 * keys_aligned8: the key pointer is 8-byte aligned (24-byte keys then load as three u64).
 * h_segs == NULL: tkv_amq_build of n_segs leaves holding n_keys keys.  With h_segs (the plan's
 * segments): tkv_amq_build_ex; leaf_route[i] (may be NULL) is leaf i's TKV_AMQ_LEAF_*, `out`
 * describes the compacted batch of the TKV_AMQ_LEAF_BATCH leaves (ws_bytes: after the leaf
 * list), and is zeroed when there is none.  have_workspace 0: no workspace pointer. */
int tkv_amq_build_route(int kind, uint32_t key_stride, int has_offsets, int keys_aligned8,
                        uint32_t n_segs, uint64_t n_keys, uint32_t max_blocks,
                        const tkv_amq_segment* h_segs, int have_workspace, uint64_t workspace_bytes,
                        struct tkv_amq_build_route* out, uint8_t* leaf_route);

/* Synchronises `stream`; returns TKV_AMQ_OK, TKV_AMQ_INTERNAL (a VQF block overflowed) or
 * TKV_AMQ_INVALID_ARGUMENT (the workspace was smaller than the plan).  Bloom builds cannot
 * fail on the device. */
int tkv_amq_build_check(int kind, const void* d_workspace, uint64_t workspace_bytes,
                        void* stream);

/* Hash-range sharding of ONE monolithic Bloom filter over several GPUs (BASELINE config 5,
 * SURVEY.md 8(e); no reference counterpart: the reference builds each filter on one CPU
 * thread, filter_builder.hpp:126-135).  The filter planned by tkv_amq_plan for the whole key
 * set (one segment of n_blocks blocks) is cut into T = ceil(n_blocks / tile_blocks) tiles of
 * tkv_amq_bloom_tile_blocks() blocks (2048: one 128 KiB LDS image); part p of n_parts owns
 * tiles [p*q, min((p+1)*q, T)), q = ceil(T / n_parts), i.e. a contiguous byte range of the
 * bitmap.  A key belongs to the tile of its block (h0).  A rank may own several consecutive
 * parts (its range is then their union, built part by part).
 *
 * tkv_amq_bloom_route: rank-local step 1.  Reorders this rank's n_keys 16-byte keys by owning
 * part into d_routed16 (part 0's keys first) and writes the per-part counts
 * (d_part_counts[n_parts], u32, device) -- the send counts of the all-to-all that follows.
 * d_seg is the whole filter's segment (device), n_blocks its n_blocks (host copy). */
uint32_t tkv_amq_bloom_tile_blocks(void);
/* the most tiles one range build takes, from records (records != 0) or from 16-byte keys: the
 * partition's LDS tile table (6,400 tiles) */
uint32_t tkv_amq_bloom_range_max_tiles(int records);
uint64_t tkv_amq_bloom_route_ws_bytes(uint64_t n_keys, uint32_t n_parts);
int tkv_amq_bloom_route(const uint8_t* d_keys16, uint64_t n_keys, const tkv_amq_segment* d_seg,
                        uint32_t n_blocks, uint32_t n_parts, uint8_t* d_routed16,
                        uint32_t* d_part_counts, void* d_workspace, uint64_t workspace_bytes,
                        void* stream);

/* tkv_amq_bloom_build_range: rank-local step 2, after the all-to-all.  Builds tiles
 * [tile_begin, tile_end) of the filter from the keys this rank received (all of whose tiles
 * must fall in the range; others are ignored) into d_out at the segment's out_offset, exactly
 * where tkv_amq_build puts them, and writes the filter header too.  Bytes of other tiles are
 * not touched, so the ranks' ranges are disjoint and one all-gather of them is the filter.
 * An empty range (tile_begin == tile_end: a rank past the last tile when ceil(T/q) < ranks)
 * writes the header only.  Keys are 16 bytes (route and range build alike); a range holds at
 * most tkv_amq_bloom_range_max_tiles(0) tiles. */
uint64_t tkv_amq_bloom_build_range_ws_bytes(uint64_t n_keys, uint32_t tile_begin, uint32_t tile_end);
int tkv_amq_bloom_build_range(const uint8_t* d_keys16, uint64_t n_keys, const tkv_amq_segment* d_seg,
                              uint32_t n_blocks, uint32_t tile_begin, uint32_t tile_end,
                              uint8_t* d_out, void* d_workspace, uint64_t workspace_bytes,
                              void* stream);

/* The same two steps with 12-byte bit records in place of the keys (the routes of 16- and
 * 24-byte keys: hash_count <= 8, i.e.
 * bits_per_key <= 12; InvalidArgument otherwise): tkv_amq_bloom_route_records hashes each key
 * once and writes its record (block in tile, the k bit indices, the tile relative to its
 * owner's first tile) into d_recs12 ordered by owner, so the all-to-all carries 12 bytes per key
 * instead of 16 and the owner does not hash again; tkv_amq_bloom_build_range_records builds the
 * owner's tiles from the records it received.  The record carries its tile relative to its
 * part, so a part -- and a range built from records -- holds at most
 * tkv_amq_bloom_range_max_tiles(1) tiles (6,400: 800 MiB of filter); a route with larger parts
 * is refused (InvalidArgument). */
uint64_t tkv_amq_bloom_route_records_ws_bytes(uint64_t n_keys, uint32_t n_parts);
int tkv_amq_bloom_route_records(const uint8_t* d_keys16, uint64_t n_keys, const tkv_amq_segment* d_seg,
                                uint32_t n_blocks, uint32_t hash_count, uint32_t n_parts,
                                uint8_t* d_recs12, uint32_t* d_part_counts, void* d_workspace,
                                uint64_t workspace_bytes, void* stream);
/* tkv_amq_bloom_route_records_ex: the same with key_bytes 16 or 24 (24-byte keys 8-byte
 * aligned: TurtleKV's default key size, tree/tree_options.hpp:58); the records, and so the
 * exchange and tkv_amq_bloom_build_range_records, do not depend on the key size.  Same
 * workspace as tkv_amq_bloom_route_records_ws_bytes. */
int tkv_amq_bloom_route_records_ex(const uint8_t* d_keys, uint32_t key_bytes, uint64_t n_keys,
                                   const tkv_amq_segment* d_seg, uint32_t n_blocks,
                                   uint32_t hash_count, uint32_t n_parts, uint8_t* d_recs12,
                                   uint32_t* d_part_counts, void* d_workspace,
                                   uint64_t workspace_bytes, void* stream);
/* tkv_amq_bloom_build_range_records takes hash_count up to 16: n_recs counts records, and
 * every record of a hash_count > 8 build sets its eight indices (wide records, below). */
uint64_t tkv_amq_bloom_build_range_records_ws_bytes(uint64_t n_recs, uint32_t tile_begin,
                                                    uint32_t tile_end);
int tkv_amq_bloom_build_range_records(const uint8_t* d_recs12, uint64_t n_recs,
                                      const tkv_amq_segment* d_seg, uint32_t n_blocks,
                                      uint32_t hash_count, uint32_t tile_begin, uint32_t tile_end,
                                      uint8_t* d_out, void* d_workspace, uint64_t workspace_bytes,
                                      void* stream);

/* The wide record, and the route for keys of any shape.  A record holds eight bit indices; a
 * key with 9 <= hash_count <= 16 (13 to 23 bits/key) leaves as TWO 12-byte records with the
 * same block and tile, the first holding bits 0..7, the second bits 8..k-1 padded by repeating
 * bit 8 (OR is idempotent: the padding sets no new bit).  So the exchange still carries
 * 12-byte units, the 6,400-tile limit per part is unchanged, and a record consumer sets all
 * eight indices of every record without knowing k.
 * tkv_amq_bloom_route_records_any routes keys of any shape -- key_offsets == NULL: a fixed
 * key_stride (> 0, 16 and 24 included); else key_offsets[n_keys + 1] on the device, as
 * tkv_amq_build takes them -- for 1 <= hash_count <= 16.  The rank's keys are keys [0, n_keys)
 * of its own buffer (the segment's key_begin and n_keys describe the whole filter and are not
 * applied).  Each key becomes rpk = tkv_amq_bloom_records_per_key(hash_count) records, written
 * to d_recs12 (rpk * n_keys * 12 bytes, 4-byte aligned) grouped by part, part 0 first;
 * d_part_counts[n_parts] counts RECORDS.  A key's records land in the same part.  Asynchronous,
 * allocates nothing, capturable.  InvalidArgument: hash_count 0 or > 16, n_parts 0 or > 2048,
 * parts of more than tkv_amq_bloom_range_max_tiles(1) tiles, rpk * n_keys > 0xffffffff, fixed
 * keys with stride 0, null or misaligned buffers, a short workspace. */
/* 12-byte bit records per key: 1 for hash_count 1..8, 2 for 9..16, 0 otherwise (host only) */
uint32_t tkv_amq_bloom_records_per_key(uint32_t hash_count);
uint64_t tkv_amq_bloom_route_records_any_ws_bytes(uint64_t n_keys, uint32_t n_parts, uint32_t hash_count);
int tkv_amq_bloom_route_records_any(const uint8_t* keys, const uint64_t* key_offsets, uint32_t key_stride,
                                    uint64_t n_keys, const tkv_amq_segment* d_seg, uint32_t n_blocks,
                                    uint32_t hash_count, uint32_t n_parts, uint8_t* d_recs12,
                                    uint32_t* d_part_counts, void* d_workspace, uint64_t workspace_bytes,
                                    void* stream);

/* The pipelined hash-range build (hash_count <= 8): the route writes fixed-capacity part
 * blocks, so the exchange needs no counts first.  Parts of q tiles are owned round-robin: part p
 * belongs to rank p % world as its part j = p / world, so round j (parts [j*world, (j+1)*world))
 * is one contiguous byte range of the bitmap and can be all-gathered in place as soon as every
 * rank has built its part of it.  Per step, each rank:
 *   1. routes its keys in n_chunks chunks (tkv_amq_bloom_route_blocks): every key hashed once
 *      into its 12-byte bit record, counting-sorted by part on chip, and appended to its route
 *      workgroup's region of that part's block.  Chunk c's send buffer holds n_parts blocks in
 *      global part order (part p at p * block_bytes), so round j's blocks -- one per
 *      destination -- are one slice;
 *   2. exchanges round j of chunk c with one all-to-all of equal splits (block_bytes per peer):
 *      the chunks' rounds as their routes finish, the last chunk round by round;
 *   3. builds its part j from the n_chunks * world blocks of round j it received, laid out
 *      contiguously (tkv_amq_bloom_build_part_blocks), as soon as they have landed, writing the
 *      part's tiles where tkv_amq_build puts them (and the header);
 *   4. all-gathers round j as soon as its part of round j is built, while the next rounds
 *      are exchanged and built.
 * Records beyond a region's capacity travel as (record, part) entries in its block's overflow area, at
 * most ovf_cap per block; tkv_amq_bloom_blocks_lost reports a block that needed more (keys far
 * from uniform, e.g. one key repeated), after which the caller must build through the exact
 * exchange (tkv_amq_bloom_route_records + tkv_amq_bloom_build_range_records) instead. */
typedef struct tkv_amq_route_plan {
  uint32_t n_tiles;          /* T = ceil(n_blocks / tile_blocks) */
  uint32_t n_parts;          /* world * parts_per_rank */
  uint32_t parts_per_rank;   /* g */
  uint32_t part_tiles;       /* q: part p owns tiles [p*q, min((p+1)*q, T)) */
  uint32_t world;
  uint32_t n_chunks;
  uint32_t route_wgs;        /* P: route workgroups per chunk (= a part build's workgroups) */
  uint32_t region_cap;       /* records per (part block, route workgroup) region */
  uint32_t ovf_cap;          /* overflow entries per part block */
  uint32_t hash_count;
  uint64_t chunk_keys;       /* keys per chunk the capacities are sized for (fewer is fine) */
  uint64_t block_bytes;      /* one (chunk, sender, part) block */
  uint64_t counts_off, ovf_n_off, regions_off, ovf_off;  /* block layout */
  uint64_t route_ws_bytes;   /* workspace of one tkv_amq_bloom_route_blocks call */
  uint64_t part_ws_bytes;    /* workspace of one tkv_amq_bloom_build_part_blocks call */
  uint64_t part_bytes;       /* bitmap bytes per part (q tiles; parts past the last tile pad) */
  uint64_t n_blocks;         /* the filter's blocks */
} tkv_amq_route_plan;

/* chunk_keys: the most keys a rank routes per chunk (the capacities assume a uniform hash) */
int tkv_amq_bloom_route_plan(uint64_t chunk_keys, uint32_t n_chunks, uint32_t n_blocks,
                             uint32_t hash_count, uint32_t world, tkv_amq_route_plan* plan);
/* d_keys: n_keys keys of key_bytes 16 (16-byte aligned) or 24 (8-byte aligned), n_keys <=
 * plan->chunk_keys.  Part p's block goes to d_dst + (p / world) * round_stride + (p % world) *
 * block_bytes; round_stride 0 means world * block_bytes (a send buffer: n_parts * block_bytes,
 * part p at p * block_bytes).  A rank that exchanges nothing (world 1) routes chunk c straight
 * into its receive layout with d_dst = recv + c * block_bytes, round_stride = n_chunks *
 * block_bytes. */
int tkv_amq_bloom_route_blocks(const uint8_t* d_keys, uint32_t key_bytes, uint64_t n_keys,
                               const tkv_amq_segment* d_seg, const tkv_amq_route_plan* plan,
                               uint8_t* d_dst, uint64_t round_stride, void* d_workspace,
                               uint64_t workspace_bytes, void* stream);
/* part: the global part index (this rank's part j is j * world + rank); d_recv: the part's
 * n_recv blocks, block_bytes apart (n_chunks * world after the exchange of its round); d_out:
 * the whole filter payload (header + bitmap, padded to 64 + n_parts * part_bytes) */
int tkv_amq_bloom_build_part_blocks(const uint8_t* d_recv, uint32_t n_recv,
                                    const tkv_amq_segment* d_seg, const tkv_amq_route_plan* plan,
                                    uint32_t part, uint8_t* d_out, void* d_workspace,
                                    uint64_t workspace_bytes, void* stream);
/* synchronises `stream`; returns 1 if any of the n_recv blocks lost overflow entries (the
 * exact exchange must be used), 0 if none, < 0 on error */
int tkv_amq_bloom_blocks_lost(const uint8_t* d_recv, uint32_t n_recv, const tkv_amq_route_plan* plan,
                              void* stream);

/* Batched probe: query i tests the filter of segment d_query_seg[i].  d_result[i] = 1 if
 * the key may be present, 0 if the filter rejects it (reject_page == kTrue).  A segment index
 * >= n_segs, like a segment without a filter, answers 1 (kUnknown: cannot reject). */
int tkv_amq_probe(int kind, const uint8_t* d_filters, const tkv_amq_segment* d_segs,
                  uint32_t n_segs, const uint8_t* queries, const uint64_t* query_offsets,
                  uint32_t query_stride, uint64_t n_queries, const uint32_t* d_query_seg,
                  uint8_t* d_result, void* stream);

/* KeyQuery::Metrics counters (tree/key_query.hpp:36-60) a probe launch adds to (device
 * memory, u64 each, accumulated with atomics across launches; zero them to reset). */
typedef struct tkv_amq_probe_metrics {
  uint64_t total_filter_query_count;    /* every (query, leaf) test (:154) */
  uint64_t no_filter_page_count;        /* leaf without a filter / outside the plan (:157) */
  uint64_t page_id_mismatch_count;      /* filter's src_page_id != the leaf asked about (:210,231) */
  uint64_t filter_reject_count;         /* definitely absent, kTrue (:243) */
  uint64_t filter_positive_count;       /* filter says maybe, kFalse (key_query.cpp:41) */
  uint64_t filter_false_positive_count; /* positive, but ground truth says absent (:77) */
} tkv_amq_probe_metrics;

/* Optional per-query inputs and outputs of the _ex probes (any field may be NULL):
 *  d_query_page_id[i]  the leaf page id query i asks about (reject_page's page_id_to_reject);
 *                      if it differs from the filter's src_page_id the answer is 1 (kUnknown)
 *  d_truth[i]          1 if the key is in the leaf (the leaf search's answer), for the
 *                      false-positive count; NULL => filter_false_positive_count untouched
 *  d_metrics           counters to add to */
typedef struct tkv_amq_probe_opts {
  const uint64_t* d_query_page_id;
  const uint8_t* d_truth;
  tkv_amq_probe_metrics* d_metrics;
} tkv_amq_probe_opts;

int tkv_amq_probe_ex(int kind, const uint8_t* d_filters, const tkv_amq_segment* d_segs,
                     uint32_t n_segs, const uint8_t* queries, const uint64_t* query_offsets,
                     uint32_t query_stride, uint64_t n_queries, const uint32_t* d_query_seg,
                     uint8_t* d_result, const tkv_amq_probe_opts* opts, void* stream);

/* vqf_hash_val for n keys -> d_hash[n] (device) */
int tkv_amq_vqf_hash(const uint8_t* keys, const uint64_t* key_offsets, uint32_t key_stride,
                     uint64_t n_keys, uint64_t* d_hash, void* stream);

/* PackedVqfFilter::is_present(hash_val) for pre-hashed queries (hash once, probe many).
 * Pair i probes leaf d_pair_leaf[i] with hash d_hash[d_pair_query ? d_pair_query[i] : i]:
 * one query's hash serves every filter on its root-to-leaf path (tree/algo/nodes.hpp:165-178). */
int tkv_amq_vqf_probe_hashed(const uint8_t* d_filters, const tkv_amq_segment* d_segs,
                             uint32_t n_segs, const uint64_t* d_hash,
                             const uint32_t* d_pair_query, uint64_t n_pairs,
                             const uint32_t* d_pair_leaf, uint8_t* d_result, void* stream);
/* opts fields are indexed by pair i */
int tkv_amq_vqf_probe_hashed_ex(const uint8_t* d_filters, const tkv_amq_segment* d_segs,
                                uint32_t n_segs, const uint64_t* d_hash,
                                const uint32_t* d_pair_query, uint64_t n_pairs,
                                const uint32_t* d_pair_leaf, uint8_t* d_result,
                                const tkv_amq_probe_opts* opts, void* stream);

/* BloomFilterQuery<KeyView> (tree/key_query.hpp:78,97,219): the hashes one query needs,
 * computed once and reused for every Bloom filter it is tested against.  Record i lives at
 * d_query + i * tkv_amq_bloom_query_stride(k_max): u64 h0 (block selector and bit 0), then
 * u16 bit index of hash j for j = 1 .. k_max-1.  k_max <= 32; a filter whose hash_count
 * exceeds k_max cannot be tested with the record, so it cannot reject (result 1).  The _ex
 * form counts such a pair as no_filter_page_count, like a leaf without a filter, and before
 * the page-id check: it is never a page_id_mismatch_count. */
uint32_t tkv_amq_bloom_query_stride(uint32_t k_max);
int tkv_amq_bloom_hash(const uint8_t* keys, const uint64_t* key_offsets, uint32_t key_stride,
                       uint64_t n_keys, uint32_t k_max, uint8_t* d_query, void* stream);
int tkv_amq_bloom_probe_hashed(const uint8_t* d_filters, const tkv_amq_segment* d_segs,
                               uint32_t n_segs, const uint8_t* d_query, uint32_t k_max,
                               const uint32_t* d_pair_query, uint64_t n_pairs,
                               const uint32_t* d_pair_leaf, uint8_t* d_result, void* stream);
int tkv_amq_bloom_probe_hashed_ex(const uint8_t* d_filters, const tkv_amq_segment* d_segs,
                                  uint32_t n_segs, const uint8_t* d_query, uint32_t k_max,
                                  const uint32_t* d_pair_query, uint64_t n_pairs,
                                  const uint32_t* d_pair_leaf, uint8_t* d_result,
                                  const tkv_amq_probe_opts* opts, void* stream);

/* Path probe: a batched multi-get's filter walk in one call (tree/algo/nodes.hpp:158-187,
 * tree/algo/segmented_levels.hpp:358-369, tree/key_query.cpp:27-80).  Query i carries the
 * ordered list of leaves its lookup would visit, in CSR form: entries
 * [d_path_begin[i], d_path_begin[i+1]) of d_path_leaf (segment indices, newest level first).
 * Each key is hashed once, in registers; every entry answers exactly as tkv_amq_probe /
 * tkv_amq_*_probe_hashed[_ex] answer the pair (query i, that leaf): 0 = the filter rejects,
 * 1 = maybe or cannot reject (leaf >= n_segs, a segment without a filter, a d_query_page_id
 * mismatch, a VQF hash dropped by hash_val_shift).  The entries that answered 1 are query i's
 * candidates -- the leaves still to search -- written in path order:
 *   d_cand_leaf[d_cand_begin[i] .. d_cand_begin[i+1])   the leaves
 *   d_cand_entry[same positions]                         their entry indices (if not NULL)
 * d_cand_begin[0] == 0 and d_cand_begin[n_queries] is the total; nothing past the total is
 * written (capacity n_entries).  The output is a function of the inputs only.
 *  queries / query_offsets / query_stride   the key forms of tkv_amq_probe
 *  d_entry_result   [n_entries] or NULL: the answer of every entry
 *  opts             NULL, or fields indexed by ENTRY (as the hashed _ex probes index by pair);
 *                   one count per entry, classified as there
 *  d_workspace      tkv_amq_path_probe_ws_bytes(n_queries, n_entries) bytes, 16-byte aligned
 * Both ends of a path are clamped to n_entries and end < begin reads as empty, so a malformed
 * list gives a defined answer and never an out-of-range access.  If the clamped paths of a
 * path_begin that is not monotone share entries, each query's candidates are still its own;
 * d_entry_result at a shared entry holds the answer of one of the queries that cover it, and
 * candidates that would not fit the capacity are dropped (the offsets stop at n_entries).
 * Asynchronous on `stream`; never allocates, copies synchronously or synchronises.
 * InvalidArgument: unknown kind, n_queries or n_entries above 0xffffffff, a null required
 * buffer with a non-zero count, fixed keys with stride 0, a short or misaligned workspace.
 * n_queries == 0 is OK and writes d_cand_begin[0] = 0.
 * tkv_amq_path_probe_ws_bytes is a host function (no device needed): at least 16, and 0 for
 * counts the probe refuses. */
uint64_t tkv_amq_path_probe_ws_bytes(uint64_t n_queries, uint64_t n_entries);
int tkv_amq_path_probe(int kind, const uint8_t* d_filters, const tkv_amq_segment* d_segs, uint32_t n_segs,
                       const uint8_t* queries, const uint64_t* query_offsets, uint32_t query_stride,
                       uint64_t n_queries, const uint32_t* d_path_begin, const uint32_t* d_path_leaf,
                       uint64_t n_entries, uint8_t* d_entry_result, uint32_t* d_cand_begin,
                       uint32_t* d_cand_leaf, uint32_t* d_cand_entry, const tkv_amq_probe_opts* opts,
                       void* d_workspace, uint64_t workspace_bytes, void* stream);

/* Leaf search: resolves a batch of lookups' candidates to found keys (find_key_in_leaf_impl,
 * tree/key_query.cpp:27-80: std::lower_bound over the leaf's sorted keys and an equality test,
 * :299-327; the item index reported, :196,327; the walk ended at the first leaf that holds the
 * key, tree/algo/nodes.hpp:165-187; a false positive counted when a filter that said "maybe"
 * guarded a leaf without the key, :76-78).  Behind tkv_amq_path_probe it completes a batched
 * multi-get over device-resident keys: (leaf, item index) per query, and KeyQuery::Metrics
 * without host truth.
 * Candidates.  Query i's candidates are positions [d_cand_begin[i], d_cand_begin[i+1]) of
 * d_cand_leaf, in path order: what tkv_amq_path_probe writes, or any CSR list.  Both ends are
 * clamped to n_cand and an end below its begin reads as empty.  d_cand_entry is
 * tkv_amq_path_probe's output of the same name, or NULL.
 * Leaf keys.  leaf_keys / leaf_key_offsets / leaf_key_stride / n_leaf_keys are the key forms of
 * tkv_amq_build (leaf_key_offsets[n_leaf_keys + 1] on the device, or a fixed stride).  Leaf s
 * owns keys [seg.key_begin, seg.key_begin + seg.n_keys), or with d_key_begin (device, n_segs + 1
 * entries) keys [d_key_begin[s], d_key_begin[s+1]): the form for opened segments, as
 * tkv_amq_verify_members defines it.  Ranges are clamped to n_leaf_keys.  Query keys and leaf
 * keys may be of different forms (fixed queries against offset-form leaves, say).
 * Precondition.  Each leaf's keys are in ascending byte order -- memcmp over the common length,
 * then the shorter key first: the order of std::string_view.  On an unsorted leaf the result is
 * whatever the lower-bound procedure yields: defined, never out of range, no membership answer.
 * Search.  The lower bound of the query key in the leaf's range; FOUND iff that position is
 * inside the range and the key there equals the query byte for byte and in length.  key_index
 * is that position as a global index (so the first of a run of equal keys).  An empty leaf is
 * ABSENT.
 * Walk.  Candidates are taken in order.  Without TKV_AMQ_FIND_ALL the walk ends at the first
 * FOUND (the reference: newest level first); later candidates are NOT_SEARCHED and count
 * nowhere.  With it every candidate is searched; d_result is still the first hit in path order.
 * False positives.  If opts && opts->d_metrics, a candidate that is searched and ABSENT adds 1
 * to filter_false_positive_count iff reject_page's class of it is "checked" -- the leaf is in
 * the plan, its segment has a filter and, when opts->d_query_page_id is given, the filter's
 * stored page id equals d_query_page_id[d_cand_entry[pos]] -- judged by the code the probes
 * judge it with.  No other field of tkv_amq_probe_metrics is touched (the path probe has
 * counted them); opts->d_truth is ignored.  d_filters is read only for the page-id check (8
 * bytes per such candidate) and may be NULL otherwise; d_cand_entry's values are the caller's
 * indices into d_query_page_id and are used as given.
 * Outputs.  d_result[i] is written for every query.  d_cand_state (may be NULL) is written at
 * every position inside a query's clamped range and nowhere else.  Integer atomics on the
 * counters only, none on an output position: the output is a function of the input.  (Where
 * the clamped ranges of a d_cand_begin that is not monotone share positions, d_cand_state there
 * holds the state one of the covering queries saw; every d_result is still its own query's.)
 * One lane per query: the workload has about one candidate per query that exists and about none
 * for one that does not, so the early exit needs no second pass and no atomics; a query with
 * hundreds of candidates is searched serially by its lane.  16-byte keys (both sides fixed,
 * 16-byte aligned) and 24-byte keys (both fixed, 8-byte aligned) are compared as big-endian
 * words; any other shape 8 bytes at a time where both keys have them, then the tail bytes, then
 * the lengths, never reading past a key's end.
 * Asynchronous on `stream`: one kernel launch, no workspace, no allocation, no synchronisation;
 * capturable as a linear chain behind tkv_amq_path_probe.  n_queries == 0 is OK.
 * InvalidArgument, judged before a device is looked for: unknown kind; unknown flag bits;
 * n_queries or n_cand above 0xffffffff; a null d_cand_begin, d_result or queries with
 * n_queries > 0; a null d_cand_leaf with n_cand > 0; a null d_segs with n_segs > 0; null
 * leaf_keys with n_leaf_keys > 0; a fixed form (no offsets) with stride 0, on either side;
 * opts->d_query_page_id without d_cand_entry or without d_filters; d_result not 16-byte
 * aligned; d_counts not 8-byte aligned.  A valid call on a machine without a device returns
 * Unavailable. */
typedef struct tkv_amq_find_result { /* 16 bytes */
  uint64_t key_index; /* global index (into leaf_keys) of the found key; ~0ull if not found */
  uint32_t leaf;      /* the segment that holds it; 0xffffffff if none */
  uint32_t cand;      /* position in d_cand_leaf of that candidate; 0xffffffff if none */
} tkv_amq_find_result;

typedef struct tkv_amq_find_counts { /* 32 bytes, u64 each, ADDED to with atomics (zero to reset) */
  uint64_t leaf_search_count;  /* candidates searched */
  uint64_t found_count;        /* queries that found their key */
  uint64_t absent_count;       /* candidates searched that did not hold the key */
  uint64_t unsearchable_count; /* candidates naming no leaf of the plan (leaf >= n_segs) */
} tkv_amq_find_counts;

#define TKV_AMQ_FIND_ALL 0x1u /* search every candidate, not only up to the first hit */

/* per-candidate state, d_cand_state (optional) */
#define TKV_AMQ_CAND_ABSENT 0u       /* searched, key not in the leaf */
#define TKV_AMQ_CAND_FOUND 1u        /* searched, key in the leaf */
#define TKV_AMQ_CAND_NOT_SEARCHED 2u /* the walk had already ended at an earlier candidate */
#define TKV_AMQ_CAND_UNSEARCHABLE 3u /* leaf >= n_segs */

int tkv_amq_find_keys(int kind, const uint8_t* d_filters, const tkv_amq_segment* d_segs, uint32_t n_segs,
                      const uint8_t* queries, const uint64_t* query_offsets, uint32_t query_stride,
                      uint64_t n_queries,
                      const uint32_t* d_cand_begin, const uint32_t* d_cand_leaf,
                      const uint32_t* d_cand_entry, uint64_t n_cand,
                      const uint8_t* leaf_keys, const uint64_t* leaf_key_offsets, uint32_t leaf_key_stride,
                      uint64_t n_leaf_keys, const uint64_t* d_key_begin,
                      uint32_t flags, tkv_amq_find_result* d_result, uint8_t* d_cand_state,
                      const tkv_amq_probe_opts* opts, tkv_amq_find_counts* d_counts, void* stream);

/* Tree walk: resolves a batch of lookups to the paths tkv_amq_path_probe and tkv_amq_find_keys
 * start from (find_pivot_containing, tree/algo/nodes.hpp:48-71; find_key, :158-187;
 * for_each_active_segment_in / find_key, tree/algo/segmented_levels.hpp:340-369; the shapes of
 * PackedNodePage, tree/packed_node_page.hpp:42-223; get_flushed_item_upper_bound,
 * packed_node_page.cpp:231-248).  Keys -> paths -> candidates -> found keys is then three calls on
 * one stream with no host work between them.
 * The tree is flat, caller-owned device memory; node 0 is the root.
 *  nodes[n_nodes]             a node owns pivot_count + 1 keys k0..kp of the pivot-key list from
 *                             pivot_key_begin, the segments of its update buffer from seg_begin
 *                             (level l: [seg_begin + level_start[l], seg_begin + level_start[l+1]),
 *                             as UpdateBuffer::level_start) and one child per pivot from child_begin
 *  segments[n_segments]       one update-buffer segment: the leaf it names, in the filter plan
 *                             (`leaf`, passed through as given: 0xffffffff or any leaf >= the probe's
 *                             n_segs is "cannot reject" there) and as a page id; active_pivots and
 *                             flushed_pivots, one bit per pivot
 *  children[n_children]       page id and index: a node index under a parent of height > 1, a leaf
 *                             index (as `leaf` above) under one of height 1 (or 0, read as 1)
 *  d_flushed_bounds[n_flushed_bounds]  u32; a segment's bound for pivot p is 0 if bit p of
 *                             flushed_pivots is clear, else d_flushed_bounds[flushed_begin + the
 *                             number of set bits of flushed_pivots below p] (bit_rank)
 *  pivot_keys / pivot_key_offsets / pivot_key_stride / n_pivot_keys   the key forms of
 *                             tkv_amq_build; queries likewise
 * Per query, from node 0 at depth 0:
 *  1. p = the number of the node's interior keys k1..k(pivot_count-1) that are <= the query: an
 *     upper_bound in std::string_view order (tkv_amq_find_keys' order).  k0 and kp are never read;
 *     pivot_count == 1 gives p = 0 and reads no key.
 *  2. for level 0 .. level_count-1, for each segment of the level in order: if bit p of its
 *     active_pivots is set, the entry (leaf, leaf_page_id, flushed bound for p, depth << 8 | level)
 *  3. child p: under height <= 1 the entry (index, page_id, 0, depth << 8 | 0xff) and the walk ends;
 *     otherwise the walk goes on in node `index` at depth + 1.
 * Output: a CSR list in that order.  d_path_begin[i] is the exact prefix sum clamped to
 * path_capacity (d_path_begin[n_queries] = min(total, path_capacity)); entries at positions below
 * path_capacity are written to d_path_leaf and to each of d_path_page_id / d_path_flushed /
 * d_path_where that is given; nothing is written at or past path_capacity; *d_needed (if given)
 * is the unclamped total, so a caller sees a short capacity and can retry.  The output is a
 * function of the input: no atomics.  d_path_flushed and d_path_where are for a search that knows
 * the reference's rule "found below the flushed bound: skip the rest of the level"
 * (tree/algo/segments.hpp:185-200); tkv_amq_find_keys does not read them: tkv_amq_get_keys is the
 * call that applies the rule (it takes the bounds from the tree itself).
 * Malformed trees get a defined answer and never an out-of-range read:
 *  - interior keys at or past n_pivot_keys do not exist (the search runs over those that do)
 *  - a level's segment range is clamped to n_segments; level_start[l+1] < level_start[l] reads as
 *    an empty level; level_count above 7 reads as 7
 *  - a flushed-bound index at or past n_flushed_bounds reads as 0
 *  - the walk ends, with what it has emitted, at a node index >= n_nodes (n_nodes == 0: every path
 *    is empty), at pivot_count 0 or > 64, at a child slot >= n_children, and after
 *    TKV_AMQ_WALK_MAX_DEPTH nodes (so a cycle terminates)
 * Chaining without a host read: give tkv_amq_path_probe n_entries = path_capacity and a workspace
 * sized for it (its paths then lie below the total), and d_path_page_id as opts->d_query_page_id.
 * Asynchronous on `stream`: three kernel launches (count, scan, write; an empty batch: one), no
 * allocation, no synchronisation; capturable as a linear chain in front of tkv_amq_path_probe.
 * n_queries == 0 is OK and writes d_path_begin[0] = 0 and *d_needed = 0 (each if given).
 *  d_workspace   tkv_amq_walk_paths_ws_bytes(n_queries) bytes (host function: >= 16, monotone, 0
 *                for counts the walk refuses), 16-byte aligned: 16 bytes per query (its pivot at
 *                each depth, 6 bits x 16) and 8 per 256 queries
 * InvalidArgument, judged before a device is looked for: any count above 0xffffffff; a null
 * nodes / segments / children / d_flushed_bounds / pivot_keys / queries with its count non-zero; a
 * null d_path_begin or d_workspace with n_queries > 0; a null d_path_leaf with path_capacity > 0;
 * a fixed key form (no offsets) with stride 0, on either side; nodes, segments or children not
 * 16-byte aligned; d_needed not 8-byte aligned; a short or misaligned workspace.  A valid call on
 * a machine without a device returns Unavailable. */
#define TKV_AMQ_WALK_MAX_DEPTH 16u
#define TKV_AMQ_WALK_LEAF_LEVEL 0xffu /* d_path_where's level byte of a child-leaf entry */

typedef struct tkv_amq_tree_node { /* 32 bytes */
  uint32_t pivot_key_begin; /* index of k0 in the pivot-key list */
  uint32_t seg_begin;       /* index of the node's first segment */
  uint32_t child_begin;     /* child of pivot i is children[child_begin + i] */
  uint32_t reserved0;
  uint8_t pivot_count;      /* 1..64 */
  uint8_t height;           /* 1: the children are leaves */
  uint8_t level_count;      /* 0..7 */
  uint8_t reserved1;
  uint8_t level_start[8];   /* level l: segments [level_start[l], level_start[l+1]) from seg_begin */
  uint32_t reserved2;
} tkv_amq_tree_node;

typedef struct tkv_amq_tree_segment { /* 32 bytes */
  uint64_t leaf_page_id;    /* the leaf's page id */
  uint64_t active_pivots;   /* bit p: the segment holds items of pivot p */
  uint64_t flushed_pivots;  /* bit p: pivot p has a flushed item upper bound */
  uint32_t leaf;            /* the leaf's segment index in the filter plan */
  uint32_t flushed_begin;   /* index of the segment's first bound in d_flushed_bounds */
} tkv_amq_tree_segment;

typedef struct tkv_amq_tree_child { /* 16 bytes */
  uint64_t page_id;         /* the child's page id */
  uint32_t index;           /* node index (parent height > 1) or leaf index (height 1) */
  uint32_t reserved;
} tkv_amq_tree_child;

uint64_t tkv_amq_walk_paths_ws_bytes(uint64_t n_queries);
int tkv_amq_walk_paths(const tkv_amq_tree_node* nodes, uint64_t n_nodes,
                       const tkv_amq_tree_segment* segments, uint64_t n_segments,
                       const tkv_amq_tree_child* children, uint64_t n_children,
                       const uint32_t* d_flushed_bounds, uint64_t n_flushed_bounds,
                       const uint8_t* pivot_keys, const uint64_t* pivot_key_offsets,
                       uint32_t pivot_key_stride, uint64_t n_pivot_keys,
                       const uint8_t* queries, const uint64_t* query_offsets, uint32_t query_stride,
                       uint64_t n_queries, uint32_t* d_path_begin, uint32_t* d_path_leaf,
                       uint64_t* d_path_page_id, uint32_t* d_path_flushed, uint16_t* d_path_where,
                       uint64_t path_capacity, uint64_t* d_needed, void* d_workspace,
                       uint64_t workspace_bytes, void* stream);

/* Fused point lookup: a batch of lookups from the root to the found key in one call
 * (NodeAlgorithms::find_key, tree/algo/nodes.hpp:158-187: levels newest first, then the child,
 * ended at the first level that yields the key; SegmentedLevelAlgorithms::find_key, tree/algo/
 * segmented_levels.hpp:340-369; SegmentAlgorithms::find_key, tree/algo/segments.hpp:166-206: an
 * item found below the segment's flushed item upper bound for the pivot "has been flushed from
 * this segment", kBreak; reject_page, tree/key_query.hpp:149-247; find_key_in_leaf_impl,
 * tree/key_query.cpp:27-80,299-327).  It computes what tkv_amq_walk_paths ->
 * tkv_amq_path_probe -> tkv_amq_find_keys compute for a tree without flushed bounds, and the
 * reference's answer for one with them; it writes no path, asks no filter below a hit and
 * counts KeyQuery::Metrics over the filters the reference would have asked.
 * Arguments: kind / d_filters / d_segs / n_segs as the probes take them; the flat tree, the pivot
 * keys and the queries exactly as tkv_amq_walk_paths takes them; leaf_keys .. d_key_begin exactly
 * as tkv_amq_find_keys takes them (the precondition on the leaves' order included).
 * Per query, from node 0 at depth 0:
 *  1. p = the pivot, as tkv_amq_walk_paths step 1 defines it.  Every clamp and stop for malformed
 *     trees listed there applies unchanged: the lookup ends with what it has so far.
 *  2. for level 0 .. level_count-1, for each segment of the level in order whose active_pivots bit
 *     p is set: VISIT (seg.leaf, seg.leaf_page_id) with bound = the segment's flushed bound for p
 *     (tkv_amq_walk_paths' definition: bit_rank, an index at or past n_flushed_bounds reads 0)
 *  3. child p: under height <= 1 VISIT (index, page_id) with bound 0 and end; otherwise go on in
 *     node `index` at depth + 1.
 * A VISIT of (leaf, page id) with a bound:
 *  - the filter is asked exactly as tkv_amq_path_probe asks an entry: the key is hashed once per
 *    query, before its first test; answer 0 = the filter rejects, 1 = maybe or cannot reject
 *    (leaf >= n_segs, a segment without a filter, a page id mismatch, a VQF hash dropped by
 *    hash_val_shift), from the same code.  With TKV_AMQ_GET_CHECK_PAGE_ID the id compared with the
 *    filter's stored one is the tree's own (leaf_page_id / page_id); without it no id is read and
 *    d_filters is read only for filter bytes.  One count per visit goes into d_metrics,
 *    classified as tkv_amq_probe_ex classifies a pair.
 *  - answer 0: the next entry.
 *  - answer 1, leaf >= n_segs: UNSEARCHABLE; the next entry.
 *  - answer 1 otherwise: the lower bound of the query in the leaf's range (range, clamp and order
 *    are tkv_amq_find_keys'; the first of equal keys).  Key not there: ABSENT, and if the visit's
 *    class was "checked", filter_false_positive_count + 1; the next entry.  Key there at global
 *    index b, index_in_leaf = b - the leaf's clamped range begin:
 *      index_in_leaf < bound   FLUSHED: the level is left -- its remaining segments are not
 *                              visited, asked or counted -- and the lookup goes on with the next
 *                              level or the child
 *      otherwise               FOUND: the result is written and the lookup ends
 *  d_result[n_queries]        (device, 16-byte aligned) written for every query
 *  d_query_visits[n_queries]  (device, or NULL) the number of visits of each query
 *  d_metrics, d_counts        (device, 8-byte aligned, or NULL) ADDED to with atomics, one per
 *                             non-zero counter per wave; zero them to reset
 * A wave sums its lanes' tallies in 32 bits before its one add per counter at the end of the launch:
 * the counters are exact while no wave visits 2^32 entries in one call (a wave takes 64 queries of
 * every 524,288; 25M lookups of 24.5 visits: 75 thousand per wave).
 * Integer atomics on the counters only: the output is a function of the input.  n_nodes == 0:
 * every result is "none" and every visit count 0.  One lane per query; 16-byte keys (all three key
 * sides fixed, 16-byte aligned) and 24-byte keys (all fixed, 8-byte aligned) are compared as
 * big-endian words, any other combination from memory; the hash takes the query side's shape as
 * tkv_amq_path_probe does.
 * Asynchronous on `stream`: one kernel launch, no workspace, no allocation, no synchronisation;
 * capturable.  n_queries == 0 is OK.
 * InvalidArgument, judged before a device is looked for: unknown kind; unknown flag bits; n_nodes,
 * n_segments, n_children, n_flushed_bounds, n_pivot_keys or n_queries above 0xffffffff; a null
 * nodes / segments / children / d_flushed_bounds / pivot_keys / leaf_keys with its count non-zero;
 * a null d_segs or d_filters with n_segs > 0; a null queries or d_result with n_queries > 0; a
 * fixed key form (no offsets) with stride 0, on any of the three key sides; nodes, segments,
 * children or d_result not 16-byte aligned; d_metrics or d_counts not 8-byte aligned;
 * d_query_visits not 4-byte aligned; fixed 16-byte queries that are not 16-byte aligned
 * (tkv_amq_path_probe's rule).  A valid call on a machine without a device returns Unavailable. */
typedef struct tkv_amq_get_result { /* 16 bytes */
  uint64_t key_index; /* global index (into leaf_keys) of the found key; ~0ull if not found */
  uint32_t leaf;      /* the segment that holds it; 0xffffffff if none */
  uint32_t where;     /* depth << 8 | level of the entry that held it (level 0xff: the child leaf,
                         as d_path_where); 0xffffffff if none */
} tkv_amq_get_result;

typedef struct tkv_amq_get_counts { /* 48 bytes, u64 each, ADDED to with atomics (zero to reset) */
  uint64_t visit_count;        /* entries visited (== total_filter_query_count) */
  uint64_t leaf_search_count;  /* visits that searched their leaf */
  uint64_t found_count;        /* queries that found their key */
  uint64_t absent_count;       /* searches that did not find the key */
  uint64_t unsearchable_count; /* visits that answered 1 and name no leaf of the plan */
  uint64_t flushed_count;      /* searches that found the key below the flushed bound */
} tkv_amq_get_counts;

#define TKV_AMQ_GET_CHECK_PAGE_ID 0x1u /* compare each filter's stored page id with the tree's */

int tkv_amq_get_keys(int kind, const uint8_t* d_filters, const tkv_amq_segment* d_segs, uint32_t n_segs,
                     const tkv_amq_tree_node* nodes, uint64_t n_nodes,
                     const tkv_amq_tree_segment* segments, uint64_t n_segments,
                     const tkv_amq_tree_child* children, uint64_t n_children,
                     const uint32_t* d_flushed_bounds, uint64_t n_flushed_bounds,
                     const uint8_t* pivot_keys, const uint64_t* pivot_key_offsets,
                     uint32_t pivot_key_stride, uint64_t n_pivot_keys,
                     const uint8_t* queries, const uint64_t* query_offsets, uint32_t query_stride,
                     uint64_t n_queries,
                     const uint8_t* leaf_keys, const uint64_t* leaf_key_offsets, uint32_t leaf_key_stride,
                     uint64_t n_leaf_keys, const uint64_t* d_key_begin,
                     uint32_t flags, tkv_amq_get_result* d_result, uint32_t* d_query_visits,
                     tkv_amq_probe_metrics* d_metrics, tkv_amq_get_counts* d_counts, void* stream);

/* Point lookup with values: tkv_amq_get_keys with the value rule of the reference's find_key
 * (tree/algo/nodes.hpp:158-187) in place of "the first level that holds the key ends the lookup".
 * The reference folds each level's answer into a running ValueView with combine_in_place
 * (core/value_view.hpp:316-361) and stops when the folded value no longer needs_combine()
 * (:279-285): a found OP_ADD_I32 is a delta and the lookup goes on through the older levels and the
 * child, summing, until it meets an OP_WRITE or an OP_DELETE or runs out of tree.
 * Arguments: everything tkv_amq_get_keys takes, with the same meaning, clamps and checks, and the
 * leaves' values, parallel to leaf_keys (the value of item i belongs to leaf key i):
 *  leaf_values          (device) the value bytes, leaf_values_bytes of them
 *  leaf_value_offsets   (device, n_leaf_keys + 1 entries) item i owns [offsets[i], offsets[i+1]), both
 *                       ends clamped to leaf_values_bytes, an end below its begin read as empty; or
 *  leaf_value_stride    (offsets NULL) item i owns [i * stride, (i+1) * stride), clamped likewise
 * No input causes a read outside [leaf_values, leaf_values + leaf_values_bytes).
 * A value is the packed form the reference stores (unpack_value_view, core/packed_key_value.hpp:
 * 18-23): byte 0 is the op (TKV_AMQ_OP_*, core/value_view.hpp:27-33), the data follows.  A value of
 * length 0 reads as NOOP with no data.  The integer of a value is as_i32() (:248-262) by data
 * length: 0 bytes: 0; 1, 2 or 3 bytes: the sign-extended little-endian integer; 4 or more: the
 * first four bytes, little-endian.
 * Per query the descent and the VISIT are exactly tkv_amq_get_keys' (pivot, levels, the filter asked
 * as the path probe asks it, the leaf searched, ABSENT, UNSEARCHABLE, FLUSHED with its "leave the
 * level") up to the point where it says FOUND.  There the item is TAKEN instead: its value is read
 * and folded into the lookup's value.
 *  - no value yet: the value becomes the item; key_index, leaf and where are the item's and stay
 *    so; an ADD_I32 starts the accumulator at its integer
 *  - the value is a pending ADD and the item's op is
 *      WRITE     the value becomes WRITE of (accumulator + the item's integer)
 *      DELETE    the value becomes WRITE of the accumulator
 *      ADD_I32   the accumulator adds the item's integer and stays pending
 *    (sums wrap modulo 2^32).  After the first of these folds the result carries
 *    TKV_AMQ_VALUE_COMBINED: its value is the 4-byte integer i32, not an item's bytes.
 *      any other op   the reference's "Bad combination of opcodes" (:331-333): the value is
 *                unchanged, the result carries TKV_AMQ_VALUE_BAD_COMBINE, bad_combine_count + 1
 * After the fold a value whose op is not ADD_I32 ends the lookup; a pending ADD leaves the level (the
 * segment search answers kBreak on a found key, tree/algo/segments.hpp:202-205, and keys are unique
 * in a level) and the lookup goes on with the next level or the child.  The reference nests -- each
 * node's find_key starts from an empty value and hands its result up to be combined
 * (nodes.hpp:176-180) -- which for the three combining ops equals this flat fold; for a bad
 * combination it does not: one on the FIRST item taken at its depth (the child leaf is a depth of
 * its own) is that node's whole result, which the parent's combine rejects, so it ends the lookup
 * with the value unchanged; one after another item taken at the same depth goes on as after an ADD.
 * A lookup that runs out of tree with the ADD pending reports op ADD_I32 and the accumulator, as
 * the reference returns it to KVStore::get (kv_store.cpp:709-719).
 *  d_result[n_queries]   (device, 16-byte aligned) one 32-byte record per query
 *  d_query_visits, d_metrics, d_counts   as tkv_amq_get_keys'; d_counts is a tkv_amq_value_counts
 * On any input in which no taken item is an ADD_I32, key_index, leaf, where, d_query_visits, all of
 * d_metrics and the six shared counts equal tkv_amq_get_keys' exactly.
 * One kernel launch, no workspace, no allocation, no synchronisation; capturable; the output is a
 * function of the input.
 * InvalidArgument, judged before a device is looked for: everything tkv_amq_get_keys refuses; a null
 * leaf_values with n_leaf_keys > 0 and leaf_values_bytes > 0; the fixed form (no offsets) with
 * stride 0 while n_leaf_keys > 0; d_result not 16-byte aligned.  A valid call on a machine without
 * a device returns Unavailable. */
#define TKV_AMQ_OP_DELETE 0u
#define TKV_AMQ_OP_NOOP 1u
#define TKV_AMQ_OP_WRITE 2u
#define TKV_AMQ_OP_ADD_I32 3u
#define TKV_AMQ_OP_PAGE_SLICE 4u
#define TKV_AMQ_OP_NONE 0xffu /* `op` of a lookup that took no item */

#define TKV_AMQ_VALUE_COMBINED 0x1u    /* the value is the record's i32, folded from several items */
#define TKV_AMQ_VALUE_BAD_COMBINE 0x2u /* an item that cannot be combined with a pending ADD was met */

typedef struct tkv_amq_value_result { /* 32 bytes */
  uint64_t key_index;  /* the newest item taken (global index into leaf_keys); ~0ull if none */
  uint64_t last_index; /* the last (oldest) item taken; == key_index when one was taken; ~0ull if none */
  uint32_t leaf;       /* the key_index item's segment and ... */
  uint32_t where;      /* ... depth << 8 | level, as in tkv_amq_get_result; 0xffffffff if none */
  int32_t i32;         /* the accumulator if the newest item was an ADD_I32, else 0 */
  uint8_t op;          /* the resolved op (TKV_AMQ_OP_*); TKV_AMQ_OP_NONE if no item was taken */
  uint8_t flags;       /* TKV_AMQ_VALUE_* */
  uint16_t n_items;    /* items taken, saturating */
} tkv_amq_value_result;

typedef struct tkv_amq_value_counts { /* 64 bytes, u64 each, ADDED to with atomics (zero to reset) */
  uint64_t visit_count;        /* the first six as tkv_amq_get_counts, ... */
  uint64_t leaf_search_count;
  uint64_t found_count;        /* ... found_count: queries that ended with a value */
  uint64_t absent_count;
  uint64_t unsearchable_count;
  uint64_t flushed_count;
  uint64_t item_count;         /* items taken */
  uint64_t bad_combine_count;  /* items met that could not be combined with a pending ADD */
} tkv_amq_value_counts;

int tkv_amq_get_values(int kind, const uint8_t* d_filters, const tkv_amq_segment* d_segs, uint32_t n_segs,
                       const tkv_amq_tree_node* nodes, uint64_t n_nodes,
                       const tkv_amq_tree_segment* segments, uint64_t n_segments,
                       const tkv_amq_tree_child* children, uint64_t n_children,
                       const uint32_t* d_flushed_bounds, uint64_t n_flushed_bounds,
                       const uint8_t* pivot_keys, const uint64_t* pivot_key_offsets,
                       uint32_t pivot_key_stride, uint64_t n_pivot_keys,
                       const uint8_t* queries, const uint64_t* query_offsets, uint32_t query_stride,
                       uint64_t n_queries,
                       const uint8_t* leaf_keys, const uint64_t* leaf_key_offsets, uint32_t leaf_key_stride,
                       uint64_t n_leaf_keys, const uint64_t* d_key_begin,
                       const uint8_t* leaf_values, const uint64_t* leaf_value_offsets,
                       uint32_t leaf_value_stride, uint64_t leaf_values_bytes,
                       uint32_t flags, tkv_amq_value_result* d_result, uint32_t* d_query_visits,
                       tkv_amq_probe_metrics* d_metrics, tkv_amq_value_counts* d_counts, void* stream);

/* The value bytes of a batch of tkv_amq_get_values results, one fixed slot per query: d_out +
 * i * out_stride receives the first min(len, out_stride) bytes of query i's value and nothing else
 * in the slot is written; d_value_len[i] receives len, the full data length, so a truncation shows:
 *  - a record whose key_index is at or past n_leaf_keys (so "none", ~0): 0 -- the records are caller
 *    memory and are trusted no further
 *  - TKV_AMQ_VALUE_COMBINED: 4, the record's i32 little-endian
 *  - op DELETE, or an empty value: 0
 *  - otherwise the data bytes of item key_index (the op byte excluded), from the value arrays as
 *    tkv_amq_get_values takes and clamps them
 * Sixteen lanes copy one value, eight bytes per lane and step: values start at
 * any byte address.  Asynchronous on `stream`, one kernel launch, no allocation; capturable behind
 * tkv_amq_get_values.  n_queries == 0 is OK.
 * InvalidArgument, judged before a device is looked for: n_queries above 0xffffffff; a null d_result
 * or d_value_len with n_queries > 0, or a null d_out with n_queries > 0 and out_stride > 0; d_result
 * not 16-byte aligned; d_value_len not 4-byte aligned; a null leaf_values with n_leaf_keys > 0 and
 * leaf_values_bytes > 0; the fixed form with stride 0 while n_leaf_keys > 0. */
int tkv_amq_gather_values(const tkv_amq_value_result* d_result, uint64_t n_queries,
                          const uint8_t* leaf_values, const uint64_t* leaf_value_offsets,
                          uint32_t leaf_value_stride, uint64_t leaf_values_bytes, uint64_t n_leaf_keys,
                          uint8_t* d_out, uint32_t out_stride, uint32_t* d_value_len, void* stream);

/* Leaf update on the device: a batch of n_jobs independent two-run merges, one per leaf being
 * updated -- the reference's {BatchUpdate} + {PackedLeafPage} => leaf (tree/subtree.cpp:170-191,
 * 211-231), which pushes the update's edits as the NEWER level and the leaf's items as the OLDER one
 * and runs merge_compact_edits over them (core/algo/merge_compact_edits.hpp:26-148).  Its output is
 * what tkv_amq_plan / tkv_amq_build and the lookups read, so an update batch becomes new leaves, new
 * filters and answered lookups without a key or a value leaving the device.
 * A run (tkv_amq_merge_run, a host struct of device pointers) is n_items items: their keys in the key
 * forms of tkv_amq_build (key_offsets[n_items + 1] on the device, or key_offsets NULL and the fixed
 * key_stride), their packed values in the value forms of tkv_amq_get_values (value_offsets[n_items +
 * 1] or the fixed value_stride, clamped to values_bytes as there), and d_begin[n_jobs + 1] (device):
 * job j's items are [d_begin[j], d_begin[j + 1]), both ends clamped to n_items, an end below its
 * begin read as empty (tkv_amq_find_keys' rules).  The two runs' forms are independent.  Ranges of
 * different jobs are disjoint in every leaf update; so that overlapping ones are defined too, a run
 * never reads more than n_items items in all: job j reads the first min(its count, n_items - the
 * counts of the jobs before it) items of its range.
 * PRECONDITION: each run of each job is in strictly ascending std::string_view order (keys unique
 * within a run, as in a leaf and in a compacted result set).  On other input the result is what the
 * procedure below yields: defined, never read or written out of range, and no merge answer (two
 * candidates may then claim one position of their job, which leaves another of its positions
 * unwritten).
 * Per job, with N and O its runs:
 *  - a NEWER item N[i]: r = the lower bound of its key in O; if r is inside O and O[r]'s key equals
 *    it (bytes and length), O[r] is its PARTNER.  It emits one candidate:
 *      no partner                           the item as it is
 *      a partner, newer op not ADD_I32      the item as it is (an empty value reads as NOOP)
 *      newer ADD_I32 over WRITE             op WRITE, i32 = a + b modulo 2^32, TKV_AMQ_VALUE_COMBINED
 *      newer ADD_I32 over DELETE            op WRITE, i32 = a, COMBINED
 *      newer ADD_I32 over ADD_I32           op ADD_I32, i32 = a + b, COMBINED
 *      newer ADD_I32 over any other op (NOOP, PAGE_SLICE, unknown, empty): the item unchanged,
 *                                           TKV_AMQ_VALUE_BAD_COMBINE, bad_combine_count + 1
 *    with a, b the two values' as_i32() exactly as tkv_amq_get_values defines it by data length
 *  - an OLDER item O[k]: u = the upper bound of its key in N; if u > 0 and N[u - 1]'s key equals it
 *    the item is SHADOWED and emits nothing; otherwise it emits itself
 *  - with TKV_AMQ_MERGE_DECAY_TO_ITEMS a candidate whose resolved op is DELETE, NOOP or none of the
 *    five defined ops is dropped (decays_to_item, core/value_view.hpp:372-398); without the flag
 *    every candidate is kept -- leaves keep their tombstones (ResultSet<decay_to_items = false>,
 *    tree/in_memory_leaf.hpp:35)
 *  - the kept candidates of job j appear in key order: a newer item at (kept newer items before it)
 *    + (kept older items before its bound r), an older one at (kept newer items before its bound u)
 *    + (kept older items before it)
 * On runs that meet the precondition this IS the reference's merge, run_compact and keep_item.  The
 * stable merge (merge_compact_edits.hpp:84-94) orders by key, the newer level first among equals; a
 * key occurs at most once in N and once in O, so a group of equal keys is one item, or N[i] followed
 * by its partner O[r] -- and the lower bound finds exactly that partner, the upper bound exactly that
 * shadowing item.  run_compact (core/algo/parallel_compact.hpp:80-116) lets the group's first item
 * stand and folds the later ones into it with combine while it needs_combine()
 * (core/value_view.hpp:279-285, 316-335), which is true of ADD_I32 alone: with one later item that
 * is the table above, and the partner emits nothing of its own.  keep_item
 * (core/algo/decay_to_item.hpp:14-46) then judges the group's folded value, as the decay rule does.
 * Groups come out in key order, and the items before a group are the newer ones before N[i] and the
 * older ones with a smaller key, which are those before r (before u for an older item: every newer
 * key below it, and none equal to it, lies before u).
 *  d_out_begin[n_jobs + 1] (device) the exact prefix sums of the jobs' kept counts -- exact whatever
 *                       out_capacity is (unlike the walk's clamped d_path_begin): the gather and the
 *                       plan need true counts
 *  d_items[out_capacity] (device, 16-byte aligned) the records; job j's are d_items[d_out_begin[j] ..
 *                       d_out_begin[j + 1]); a record at or past out_capacity is not written
 *  d_needed             (device, 8-byte aligned, or NULL) the total, so a short capacity shows
 *  d_counts             (device, 8-byte aligned, or NULL) ADDED to, one atomic per non-zero counter
 *                       per wave; zero it to reset
 * The output positions are a function of the input: no atomic touches one.
 * Asynchronous on `stream`: a fixed chain of kernel launches, no allocation, no synchronisation, no
 * copy; capturable.  n_jobs == 0 is OK and writes d_out_begin[0] = 0 and *d_needed = 0.
 * tkv_amq_merge_leaves_ws_bytes (host): the workspace the call needs, at least 16, monotone in each
 * argument, 0 for counts the call refuses.
 * InvalidArgument, judged before a device is looked for: unknown flag bits; a null run, d_out_begin,
 * or (n_jobs > 0) d_begin or workspace; n_jobs, either n_items or their sum above 0xffffffff; null
 * keys with n_items > 0; null values with n_items > 0 and values_bytes > 0; a fixed form (no offsets)
 * with stride 0, keys or values, either run; a null d_items with out_capacity > 0; d_items not 16-byte
 * aligned; d_needed or d_counts not 8-byte aligned; a workspace below _ws_bytes or not 16-byte
 * aligned.  A valid call on a machine without a device returns Unavailable. */
#define TKV_AMQ_MERGE_DECAY_TO_ITEMS 0x1u

typedef struct tkv_amq_merge_run { /* 64 bytes; a host struct, its pointers device memory */
  const uint8_t* keys;
  const uint64_t* key_offsets;   /* n_items + 1 entries, or NULL: the fixed form */
  const uint8_t* values;
  const uint64_t* value_offsets; /* n_items + 1 entries, or NULL: the fixed form */
  const uint64_t* d_begin;       /* n_jobs + 1 entries (tkv_amq_gather_merged does not read it) */
  uint64_t n_items;
  uint64_t values_bytes;
  uint32_t key_stride;
  uint32_t value_stride;
} tkv_amq_merge_run;

typedef struct tkv_amq_merge_item { /* 16 bytes */
  uint64_t src;      /* bit 63: the run (0 newer, 1 older); bits 0..62: the item's global index in that run's arrays */
  int32_t i32;       /* COMBINED: the folded integer; else 0 */
  uint8_t op;        /* the resolved op (TKV_AMQ_OP_*; an empty value: NOOP) */
  uint8_t flags;     /* TKV_AMQ_VALUE_COMBINED | TKV_AMQ_VALUE_BAD_COMBINE */
  uint16_t reserved; /* 0 */
} tkv_amq_merge_item;

typedef struct tkv_amq_merge_counts { /* 56 bytes, u64 each, ADDED to with atomics (zero to reset) */
  uint64_t newer_count;       /* newer items read */
  uint64_t older_count;       /* older items read */
  uint64_t pair_count;        /* shadowed older items */
  uint64_t combined_count;    /* candidates folded from two items */
  uint64_t bad_combine_count; /* newer ADD_I32 over an item that cannot be combined */
  uint64_t dropped_count;     /* candidates dropped by decay */
  uint64_t out_count;         /* candidates kept */
} tkv_amq_merge_counts;

uint64_t tkv_amq_merge_leaves_ws_bytes(uint64_t n_jobs, uint64_t n_newer, uint64_t n_older);
int tkv_amq_merge_leaves(const tkv_amq_merge_run* newer, const tkv_amq_merge_run* older, uint64_t n_jobs,
                         uint32_t flags, uint64_t* d_out_begin, tkv_amq_merge_item* d_items,
                         uint64_t out_capacity, uint64_t* d_needed, tkv_amq_merge_counts* d_counts,
                         void* d_workspace, uint64_t workspace_bytes, void* stream);

/* The bytes of a batch of tkv_amq_merge_leaves records, as arrays the other entry points take: the
 * merged items' keys (for tkv_amq_plan / tkv_amq_build / the lookups, with d_out_begin as their
 * d_key_begin) and their packed values (for tkv_amq_get_values).
 * n_out, the records gathered, is read on the device: min(d_out_begin[n_jobs], out_capacity,
 * newer->n_items + older->n_items) -- no host read sits between the two calls.  The runs are those of
 * the merge (d_begin is not read).  A record whose src index is at or past its run's n_items is caller
 * memory trusted no further: it gives an empty key and an empty value.
 *  keys    out_key_stride > 0: the fixed form, key p at d_out_keys + p * out_key_stride -- only when
 *          both runs' keys are fixed with that same stride (an untrusted record's slot is left as it
 *          is); out_key_stride == 0: the offsets form, d_out_key_offsets[n_out + 1] written by the call
 *  values  always the offsets form, d_out_value_offsets[n_out + 1] written by the call.  A COMBINED
 *          record writes 5 bytes, the op byte and i32 little-endian; every other record its source
 *          value's bytes verbatim under tkv_amq_get_values' clamps (an empty value stays empty)
 * Offsets are exact whatever the capacities: an item's bytes are written only if the item ends at or
 * below out_keys_capacity / out_values_capacity (bytes), and d_needed_bytes[0], [1] (device, or NULL)
 * report the keys' and the values' totals.  tkv_amq_merge_values_bound (host) bounds the values' total
 * before the merge has run: newer_bytes + older_bytes + 4 * n_newer, as a combined value replaces a
 * non-empty newer value and is 5 bytes.
 * Sixteen lanes move one item, eight bytes per lane and step, with a byte tail where the destination
 * is not 8-byte aligned.  Asynchronous on `stream`, no allocation, no
 * synchronisation; capturable behind tkv_amq_merge_leaves.  tkv_amq_gather_merged_ws_bytes (host): at
 * least 16, monotone.
 * InvalidArgument, judged before a device is looked for: a null run, d_out_begin, d_out_value_offsets
 * or workspace; n_jobs or either n_items or their sum above 0xffffffff; the runs' checks of
 * tkv_amq_merge_leaves (null keys, null values, stride 0); a null d_items with out_capacity > 0, or
 * not 16-byte aligned; out_key_stride > 0 with a run in the offsets form or of another stride;
 * out_key_stride == 0 with a null d_out_key_offsets; a null d_out_keys / d_out_values with its
 * capacity > 0; d_out_key_offsets, d_out_value_offsets or d_needed_bytes not 8-byte aligned; a
 * workspace below _ws_bytes or not 16-byte aligned.  A valid call without a device: Unavailable. */
uint64_t tkv_amq_merge_values_bound(uint64_t newer_bytes, uint64_t older_bytes, uint64_t n_newer);
uint64_t tkv_amq_gather_merged_ws_bytes(uint64_t out_capacity);
int tkv_amq_gather_merged(const tkv_amq_merge_item* d_items, const uint64_t* d_out_begin, uint64_t n_jobs,
                          uint64_t out_capacity, const tkv_amq_merge_run* newer, const tkv_amq_merge_run* older,
                          uint8_t* d_out_keys, uint32_t out_key_stride, uint64_t* d_out_key_offsets,
                          uint64_t out_keys_capacity, uint8_t* d_out_values, uint64_t* d_out_value_offsets,
                          uint64_t out_values_capacity, uint64_t* d_needed_bytes, void* d_workspace,
                          uint64_t workspace_bytes, void* stream);

/* The node merge on the device: a batch of n_jobs independent K-way merges of sorted runs -- the
 * reference's merge_compact_edits over a slice of K segments (core/algo/merge_compact_edits.hpp:
 * 26-148), one MergeCompactor::push_level per level.  The leaf cases push two levels (tree/subtree.cpp:
 * 182-184, 221-223, tkv_amq_merge_leaves); the node path pushes the incoming batch and every
 * update-buffer level it is about to collapse (InMemoryNode::push_levels_to_merge, tree/
 * in_memory_node.cpp:827-866, from the insert at :289-303 and the flushes and compactions at :407,
 * :454), up to TreeOptions::kMaxLevels + 1 = 7 runs.  One call ranks every item once against every
 * other run, where a chain of K - 1 tkv_amq_merge_leaves / tkv_amq_gather_merged calls re-materialises
 * every surviving byte K - 1 times.
 * `runs` is a HOST array of n_runs tkv_amq_merge_run, 1 <= n_runs <= TKV_AMQ_MERGE_MAX_RUNS, runs[0]
 * the NEWEST; each run has its own key form, value form and d_begin[n_jobs + 1].  Job j merges items
 * [d_begin[j], d_begin[j + 1]) of every run (a node merge: one pivot's key range; a leaf update: one
 * leaf), the ranges clamped exactly as tkv_amq_merge_leaves clamps them: both ends to n_items, an end
 * below its begin empty, and job j reads the first min(its count, n_items - the counts of the jobs
 * before it) items of its range, so a run never reads more items in all than it holds.
 * PRECONDITION: within a job each run is in strictly ascending std::string_view order.  On other
 * input the result is what the procedure yields: every search stays inside its job's range, every
 * position inside the job's output range, nothing is read or written out of range.
 * Per job: a GROUP is its items that share a key (bytes and length) -- on sorted input at most one
 * per run, ordered by run index by the stable merge (the pairwise merges of adjacent segments,
 * merge_compact_edits.hpp:53-107, are each stable with src_0 first, so level order survives).  The
 * group's HEAD is its item in the newest run that holds the key; every other item of the group is
 * SHADOWED and emits nothing.
 *  - an item of run s: in each newer run t < s, u = the upper bound of its key; if u > 0 and the item
 *    before u equals it, the item is shadowed.  Otherwise it is a head: in each older run t > s, r =
 *    the lower bound of its key; the item at r, if it equals the key, is a PARTNER
 *  - the head's value is folded through its partners from newer to older WHILE the accumulated op is
 *    ADD_I32 (run_compact, core/algo/parallel_compact.hpp:92-100; needs_combine() is true of ADD_I32
 *    alone):
 *      over WRITE      op WRITE, i32 = the sum modulo 2^32, TKV_AMQ_VALUE_COMBINED
 *      over DELETE     op WRITE, i32 unchanged, COMBINED
 *      over ADD_I32    i32 = the sum, COMBINED
 *      over any other (NOOP, PAGE_SLICE, unknown, empty): the value unchanged, TKV_AMQ_VALUE_
 *                      BAD_COMBINE, bad_combine_count + 1 -- and the fold goes on to the next older
 *                      partner, the value still being an ADD_I32
 *    integers read by as_i32() exactly as tkv_amq_get_values and tkv_amq_merge_leaves read them; both
 *    flags may be set on one record
 *  - with TKV_AMQ_MERGE_DECAY_TO_ITEMS a group whose folded op is not WRITE, ADD_I32 or PAGE_SLICE is
 *    dropped (keep_item, core/algo/decay_to_item.hpp:14-46); without the flag every group is kept
 *  - the kept groups of job j come out in key order: a head at (kept items of its own run before it)
 *    + for every other run (kept items before its bound there)
 * A record (tkv_amq_merge_item): src = the head's run << TKV_AMQ_LEVELS_SRC_SHIFT | its global index in
 * that run's arrays (bits 0..55); i32 the folded integer if COMBINED, else 0; op the resolved op (an
 * empty value: NOOP); flags the two value flags; reserved 0.  With n_runs == 2 every output equals
 * tkv_amq_merge_leaves' but for the position of the run bit in src.
 * tkv_amq_merge_counts, with meanings that are tkv_amq_merge_leaves' when n_runs == 2: newer_count
 * items read of run 0; older_count items read of runs 1 and up; pair_count shadowed items;
 * combined_count groups whose value is COMBINED; bad_combine_count bad combinations, once each;
 * dropped_count groups dropped by decay; out_count groups kept.
 * d_out_begin, d_items, out_capacity, d_needed, d_counts: as tkv_amq_merge_leaves has them --
 * d_out_begin exact whatever out_capacity is, a record at or past out_capacity not written, *d_needed
 * the total, no atomic on an output position.  Asynchronous on `stream`: a fixed linear chain of
 * launches, no allocation, no synchronisation, no copy; capturable.  n_jobs == 0 writes d_out_begin[0]
 * = 0 and *d_needed = 0.
 * tkv_amq_merge_levels_ws_bytes (host): at least 16, monotone in each argument, 0 for counts the call
 * refuses (n_runs 0 or above TKV_AMQ_MERGE_MAX_RUNS, n_jobs or n_items_total above 0xffffffff).
 * InvalidArgument, judged before a device is looked for: n_runs 0 or above 8; null runs; unknown flag
 * bits; any run failing tkv_amq_merge_leaves' checks of a run (n_items above 0xffffffff, null keys
 * with n_items > 0, null values with n_items > 0 and values_bytes > 0, a fixed form with stride 0, a
 * null d_begin with n_jobs > 0); n_jobs or the runs' items in all above 0xffffffff; a null
 * d_out_begin, a null d_items with out_capacity > 0, d_items not 16-byte aligned, d_needed, d_counts or
 * d_out_begin not 8-byte aligned; with n_jobs > 0 a null workspace, one below _ws_bytes or not 16-byte
 * aligned.  A valid call on a machine without a device returns Unavailable. */
#define TKV_AMQ_MERGE_MAX_RUNS 8u
/* tkv_amq_merge_item.src as tkv_amq_merge_levels writes it: bits 56..63 the run (0 = newest),
 * bits 0..55 the item's global index in that run's arrays */
#define TKV_AMQ_LEVELS_SRC_SHIFT 56

uint64_t tkv_amq_merge_levels_ws_bytes(uint64_t n_jobs, uint32_t n_runs, uint64_t n_items_total);
int tkv_amq_merge_levels(const tkv_amq_merge_run* runs, uint32_t n_runs, uint64_t n_jobs, uint32_t flags,
                         uint64_t* d_out_begin, tkv_amq_merge_item* d_items, uint64_t out_capacity,
                         uint64_t* d_needed, tkv_amq_merge_counts* d_counts,
                         void* d_workspace, uint64_t workspace_bytes, void* stream);

/* tkv_amq_gather_merged over a run table: the bytes of a batch of tkv_amq_merge_levels records.
 * Everything said of tkv_amq_gather_merged holds with "either run" read as "any run": n_out =
 * min(d_out_begin[n_jobs], out_capacity, the runs' items in all) is read on the device; offsets are
 * exact whatever the capacities; a COMBINED record writes 5 bytes; a record whose run (bits 56..63) is
 * at or past n_runs, or whose item index is at or past its run's n_items, gives an empty key and an
 * empty value; fixed key slots (out_key_stride > 0) only when every run is in the fixed form with that
 * stride; the values always in the offsets form; d_needed_bytes[0], [1] the totals; sixteen lanes per
 * item, eight bytes per lane and step.  tkv_amq_merge_levels_values_bound (host) bounds the values'
 * total: values_bytes_total + 4 * n_items_not_in_oldest_run -- a combined value replaces a head's
 * non-empty value, and a head in the oldest run has nothing below it to combine with.
 * tkv_amq_gather_levels_ws_bytes (host): at least 16, monotone.
 * InvalidArgument: as tkv_amq_gather_merged, its checks of a run applied to every run, and n_runs 0
 * or above 8 or null runs.  A valid call without a device: Unavailable. */
uint64_t tkv_amq_merge_levels_values_bound(uint64_t values_bytes_total, uint64_t n_items_not_in_oldest_run);
uint64_t tkv_amq_gather_levels_ws_bytes(uint64_t out_capacity);
int tkv_amq_gather_levels(const tkv_amq_merge_item* d_items, const uint64_t* d_out_begin, uint64_t n_jobs,
                          uint64_t out_capacity, const tkv_amq_merge_run* runs, uint32_t n_runs,
                          uint8_t* d_out_keys, uint32_t out_key_stride, uint64_t* d_out_key_offsets,
                          uint64_t out_keys_capacity, uint8_t* d_out_values, uint64_t* d_out_value_offsets,
                          uint64_t out_values_capacity, uint64_t* d_needed_bytes, void* d_workspace,
                          uint64_t workspace_bytes, void* stream);

/* Open built filters without a plan (a store restarting on a checkpoint, filter pages received
 * from elsewhere): reconstructs and validates one segment per filter from the filter bytes on
 * the device -- what KeyQuery::reject_page reads from the page itself (tree/key_query.hpp:
 * 149-247; check_magic, vqf_filter_page_view.hpp:96-100).  Where filter s lives:
 *  d_offsets != NULL    (device, n_filters entries) its payload starts at d_offsets[s] and may
 *                       extend to total_bytes
 *  stride != 0          it starts at s * stride and may extend to min((s+1) * stride, total_bytes)
 *  page_size_log2 != 0  (7..31) slot s is a whole page at s << page_size_log2, the payload 64
 *                       bytes in (tkv_amq_plan_pages' layout), bounded by the page and the
 *                       buffer; the PackedPageHeader fields the builders set (layout_id,
 *                       unused_begin, unused_end, size) must agree with the kind, the payload
 *                       size and the page size, and the segment gets the plan's page_flags
 * Exactly one of the three forms.  d_filters must be 16-byte aligned.  Per filter, in this order
 * (every read is preceded by the check that it lies inside the bound):
 *  1. the start lies inside the buffer (OUT_OF_BOUNDS), is 16-byte aligned (MISALIGNED), and the
 *     header -- 64 bytes Bloom, 80 VQF -- fits the bound (OUT_OF_BOUNDS)
 *  2. the magic: the other kind's is WRONG_KIND, anything else but this kind's BAD_MAGIC
 *  3. the fields that stand alone (BAD_GEOMETRY).  Bloom: layout == 2, 1 <= hash_count <= 32,
 *     block_count >= 1.  VQF: hash_seed is the VQF seed, hash_mask == ~0 << shift for a shift in
 *     0..63, key_remainder_bits 8 or 16, 1 <= nblocks <= 2^24
 *  4. the payload the block count names -- 64 + 64 * block_count, 32 + 48 + 64 * nblocks -- fits
 *     the bound and a uint32_t (OUT_OF_BOUNDS)
 *  5. the fields derived from the block count (BAD_GEOMETRY).  Bloom: bit_count == 512 *
 *     block_count, word_count == 8 * block_count (xxh3_checksum is not interpreted: the builders
 *     write 0).  VQF: total_size_in_bytes == 64 * nblocks, range == nblocks * buckets << tag
 *     bits, nslots == nblocks * slots, nelts <= nslots
 *  6. a page image's header fields (BAD_PAGE)
 * So a block count that points past its slot is OUT_OF_BOUNDS, and one that fits but disagrees
 * with the other fields BAD_GEOMETRY.
 * A filter that passes gets the segment the plan would have produced in out_offset, n_blocks,
 * hash_count, tag_bits, hash_val_shift, mod_magic, src_page_id, payload_bytes and page_flags;
 * n_keys is the header's item_count (Bloom) or nelts (VQF: the keys hash_val_shift did not
 * drop), saturated to 32 bits; bits_per_key, key_begin and block_base, which the page does not
 * record, are 0.  Opened segments serve the probes and tkv_amq_scan_filters; BUILDING INTO THEM
 * IS NOT SUPPORTED.  A filter that fails gets its out_offset and otherwise the all-zero "no
 * filter" segment, so every probe answers 1 (kUnknown) for it and reads none of its bytes.
 *  d_status[n_filters]  (device) the code of every filter
 *  d_summary[7]         (device, or NULL) the count of each code; zeroed by the call
 * Asynchronous on `stream`, capturable: one kernel launch (after a 28-byte memset node for
 * d_summary, if given); no allocation, no synchronisation.  n_filters == 0 is OK.
 * InvalidArgument: unknown kind, not exactly one location form (with n_filters > 0; more than
 * one always), page_size_log2 outside 7..31, a misaligned d_filters, a null required buffer.
 * Both entry points judge their arguments before they look for a device, so a bad call is
 * InvalidArgument everywhere and a good one is Unavailable where no device is visible. */
#define TKV_AMQ_OPEN_OK 0u
#define TKV_AMQ_OPEN_BAD_MAGIC 1u     /* neither kind's magic (all-zero included) */
#define TKV_AMQ_OPEN_WRONG_KIND 2u    /* the other kind's magic */
#define TKV_AMQ_OPEN_BAD_GEOMETRY 3u  /* header fields disagree with each other or the spec */
#define TKV_AMQ_OPEN_OUT_OF_BOUNDS 4u /* header or payload does not fit its slot / the buffer */
#define TKV_AMQ_OPEN_MISALIGNED 5u    /* payload offset not 16-byte aligned */
#define TKV_AMQ_OPEN_BAD_PAGE 6u      /* page-image form: PackedPageHeader fields disagree */
int tkv_amq_open_filters(int kind, const uint8_t* d_filters, uint64_t total_bytes,
                         const uint64_t* d_offsets, uint64_t stride, uint32_t page_size_log2,
                         uint32_t n_filters, tkv_amq_segment* d_segs, uint32_t* d_status,
                         uint32_t* d_summary, void* stream);

/* One read-only pass over the blocks of every filter (plan segments or opened ones; a "no
 * filter" segment gives all-zero stats): what is in the filter bytes.
 * VQF block rules (what vqf_init_in_place and vqf_insert leave behind).  With
 * W = 128 metadata bits, B = 80 buckets, S = 48 slots for 8-bit tags and W = 64, B = 36, S = 28
 * for 16-bit tags: occ = select(md, B-1) - (B-1), the zeros below the B-th set bit.  A block is
 * bad if md has fewer than B set bits or occ > S (it then counts as bad only: it adds nothing to
 * occupied, full_blocks, empty_blocks or max_block), if popcount(md) is not W-1 (occ == 0) or
 * W-occ (otherwise), or if one of the tag slots occ .. S-1 is not zero.
 * The work is split by bytes, not by segment: chunks of 256 blocks (16 KiB), located through a
 * device-side prefix over the segments' chunk counts in the workspace, so 6,104 leaves of 20 KB
 * and one filter of 1.5 GB take the same path.  Integer atomics only: the output is a function
 * of the input.  The call zeroes d_stats itself.
 *  d_stats[n_segs]  (device, 16-byte aligned)
 *  d_workspace      tkv_amq_scan_filters_ws_bytes(n_segs) bytes (host function: >= 16,
 *                   monotone), 16-byte aligned
 * Asynchronous on `stream`, capturable (four kernel launches); no allocation, no
 * synchronisation.  n_segs == 0 is OK.  InvalidArgument: unknown kind, a null buffer with
 * n_segs > 0, a short or misaligned workspace, misaligned d_filters or d_stats. */
typedef struct tkv_amq_filter_stats { /* 32 bytes */
  uint64_t occupied;     /* Bloom: set bits; VQF: occupied tag slots, summed over blocks */
  uint64_t header_items; /* Bloom item_count / VQF nelts as stored in the payload */
  uint32_t full_blocks;  /* Bloom: all 512 bits set; VQF: no free slot */
  uint32_t empty_blocks; /* nothing set / no tag */
  uint32_t max_block;    /* largest per-block count (bits or slots) */
  uint32_t bad_blocks;   /* VQF: blocks that break a rule above; Bloom: 0 */
} tkv_amq_filter_stats;
uint64_t tkv_amq_scan_filters_ws_bytes(uint32_t n_segs);
int tkv_amq_scan_filters(int kind, const uint8_t* d_filters, const tkv_amq_segment* d_segs,
                         uint32_t n_segs, tkv_amq_filter_stats* d_stats, void* d_workspace,
                         uint64_t workspace_bytes, void* stream);

/* Verify built filters against their keys: does every key of every leaf pass its own filter?
 * One leaf-major device pass over a batch of filters (plan segments or opened ones) and the
 * keys they were built from -- the one filter property the reference's tests pin
 * (tree/in_memory_node.test.cpp:101-131: no false negatives), asked before filter pages are
 * committed, after a restart has loaded leaf and filter pages, or after an all-gather.
 * Key i of leaf s is MISSING iff tkv_amq_probe would answer 0 for (key i, segment s); so a VQF
 * hash dropped by hash_val_shift is present, and a Bloom hash_count other than 7 or 8 takes the
 * general bit ladder.  keys / key_offsets / key_stride are the key forms of tkv_amq_build (a
 * fixed stride, or key_offsets[n_keys + 1] on the device), and the 16-byte and 8-byte-aligned
 * 24-byte fast modes are chosen as the build chooses them (16-byte keys 16-byte aligned).
 * Which keys belong to leaf s:
 *  d_key_begin == NULL  keys [seg.key_begin, seg.key_begin + seg.n_keys)
 *  d_key_begin != NULL  (device, n_segs + 1 entries) keys [d_key_begin[s], d_key_begin[s+1]):
 *                       the form for opened segments, whose key_begin is 0 and whose VQF n_keys
 *                       is nelts
 * Both ends are clamped to n_keys and an end below its begin reads as empty (as
 * tkv_amq_path_probe treats its lists), so no input causes an out-of-range key read.
 *  d_result[n_segs]   (device, 16-byte aligned) per leaf: `missing` counts the keys the filter
 *                     rejects (modulo 2^32), `first_missing` is the smallest global key index
 *                     among them (~0ull if none), `flags`:
 *                     NO_FILTER    nothing was checked and missing == 0: a segment the probes
 *                                  answer 1 for without reading it (the all-zero segment
 *                                  tkv_amq_open_filters writes for a refused filter, Bloom
 *                                  hash_count == 0, VQF tag_bits == 0) or one with n_blocks == 0
 *                     ID_MISMATCH  the 8 bytes the probes' page-id check reads from the payload
 *                                  (PackedBloomFilterPage @16, PackedVqfFilter @8) differ from
 *                                  seg.src_page_id.  The keys are still checked: this is an
 *                                  audit, not reject_page
 *  d_total_missing    (device, or NULL) the sum of `missing`
 * The call initialises d_result and d_total_missing itself.  Integer atomics only (atomicAdd,
 * 64-bit atomicMin), so the output is a function of the input.
 *  max_seg_blocks     a HINT that sizes the launch's dynamic LDS (the plan's max_seg_blocks; 0 =
 *                     unknown, or a value past 160 KiB of blocks: the 160 KiB leaf budget).  A
 *                     leaf whose blocks fit what was allocated is copied into LDS and tested
 *                     there; any other leaf is tested in global memory by the same kernel.
 *                     Correctness never depends on the hint
 *  d_workspace        tkv_amq_verify_members_ws_bytes(n_segs) bytes (host function: >= 16,
 *                     monotone), 16-byte aligned
 * The work is split by keys, not by leaf: units of up to chunk_keys consecutive keys of one leaf
 * (chunk_keys chosen from n_keys alone: about 2,048 units per batch, at least 2,048 keys each),
 * located through a device-side prefix over the leaves' unit counts in the workspace, one
 * workgroup per unit; so 6,104 leaves of 16K keys take one workgroup each and one leaf of 3M
 * keys takes 1,465.
 * Asynchronous on `stream`, capturable as one linear chain (three kernel launches); no
 * allocation, no synchronous copy, no synchronisation.  n_segs == 0 is OK (and writes
 * *d_total_missing = 0 if given).  InvalidArgument, judged before a device is looked for:
 * unknown kind; with n_segs > 0 a null d_filters, d_segs, d_result or d_workspace, null keys
 * with n_keys > 0, fixed keys with stride 0, misaligned 16-byte keys, a short or misaligned
 * workspace; a misaligned d_filters or d_result (16 bytes) or d_total_missing (8).  A valid call
 * on a machine without a device returns Unavailable. */
typedef struct tkv_amq_member_check { /* 16 bytes */
  uint64_t first_missing; /* smallest global key index the filter rejects; ~0ull if none */
  uint32_t missing;       /* keys of the leaf the filter rejects (false negatives) */
  uint32_t flags;         /* TKV_AMQ_VERIFY_* */
} tkv_amq_member_check;
#define TKV_AMQ_VERIFY_NO_FILTER 0x1u   /* "no filter" segment: nothing was checked */
#define TKV_AMQ_VERIFY_ID_MISMATCH 0x2u /* payload header src_page_id != the segment's */
uint64_t tkv_amq_verify_members_ws_bytes(uint32_t n_segs);
int tkv_amq_verify_members(int kind, const uint8_t* d_filters, const tkv_amq_segment* d_segs,
                           uint32_t n_segs, uint32_t max_seg_blocks, const uint8_t* keys,
                           const uint64_t* key_offsets, uint32_t key_stride, uint64_t n_keys,
                           const uint64_t* d_key_begin, tkv_amq_member_check* d_result,
                           uint64_t* d_total_missing, void* d_workspace, uint64_t workspace_bytes,
                           void* stream);

/* Key staging, host only (no device needed): the H2D front end.  The reference passes the
 * build a flattened range of EditView whose keys are KeyView = std::string_view into leaf /
 * edit memory (core/merge_compactor.hpp:107-139, tree/filter_builder.hpp:307-331).  This
 * gathers the viewed key bytes into one contiguous, caller-owned (normally pinned) buffer
 * with up to n_threads host threads (<= 0: min(hardware threads, 16)).
 *  views, view_stride  view i is the tkv_amq_key_view at (const uint8_t*)views + i*view_stride;
 *                      the struct has the libstdc++ std::string_view layout {size, data}, so
 *                      &edits[0].key with stride sizeof(EditView) is read in place
 *  fixed_len > 0       every key must be fixed_len bytes (else InvalidArgument); key i lands
 *                      at dst + i*fixed_len (the fixed-stride key form of tkv_amq_build)
 *  fixed_len == 0      variable length: dst_offsets[n+1] (out) byte offsets into dst
 *  dst_capacity        bytes available at dst (ResourceExhausted if the keys do not fit) */
typedef struct tkv_amq_key_view {
  uint64_t size;
  const uint8_t* data;
} tkv_amq_key_view;
int tkv_amq_stage_keys(const void* views, uint64_t view_stride, uint64_t n_keys, uint32_t fixed_len,
                       uint8_t* dst, uint64_t dst_capacity, uint64_t* dst_offsets, int n_threads);

/* Synthetic 16-byte keys on the device: key i = (splitmix64_at(seed, 2(first+i)+1),
 * splitmix64_at(seed, 2(first+i)+2)), little-endian (the bench input). */
int tkv_amq_gen_keys16(uint64_t seed, uint64_t first, uint64_t n_keys, uint8_t* d_keys,
                       void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TKV_AMQ_H */
