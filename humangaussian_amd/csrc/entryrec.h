// entryrec.h - the packed formats the sort stage (binning.hip) hands to the blend kernels and the pair reductions:
//
//   SortRec      the 48 B record of one (tile, Gaussian) entry; its last word is the TAG (hgs_rec_tag)
//   entpair.x    entry id | pairs << HGS_ENTRY_BITS      (hgs_entpair_x; entpair.y = a pair-row id, see hgs_rec_tag)
//   cell key     g * 16 + c of the work items            (hgs_cell_key: global tile g, cell c)
//
// ONE definition: the sort writes through these functions, render_fwd.hip / render_bwd.hip read through them, and the
// static_asserts below refuse an edit that makes the fields overlap or outgrow their word.
//
// Plain C++ (no HIP types), like cellmask.h: the SAME functions are compiled into the kernels and into the host-side
// checker tests/entryrec_host.cpp that tests/test_pair_rows_cpu.py drives.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/hgs_rast.h"
#include "cellmask.h"

struct __attribute__((aligned(16))) SortRec {   // 48 B, one per (tile, Gaussian) entry
  float mx, my;         // pixel-space mean
  float qa, qb, qc;     // conic folded for exp2: qa=-0.5*ca*log2e, qb=-cb*log2e, qc=-0.5*cc*log2e
  float op, r, g, b, depth;
  uint32_t entry;       // entry id = chunk base + geom.offset + position of the tile in the rect (< 2^HGS_ENTRY_BITS)
  uint32_t tag;         // hgs_rec_tag (calls that keep chunk rows), else 0; the blend kernels overwrite their COPY with the list position
};
#define HGS_REC_WORDS ((uint32_t)(sizeof(SortRec) / sizeof(uint32_t)))          // 12: stride of a record in 32-bit words
#define HGS_REC_F4 ((int)(sizeof(SortRec) / 16))                                // 3: float4 / uint4 per record
#define HGS_REC_TAG_WORD ((uint32_t)(offsetof(SortRec, tag) / sizeof(uint32_t)))   // 11: the tag's word inside a record
static_assert(sizeof(SortRec) == 48, "a record is three 16 B words");
static_assert(offsetof(SortRec, entry) == 40 && offsetof(SortRec, tag) == 44, "entry id and tag close the record's third word");

// ---- the tag: SortRec::tag of the record at list position k of a tile of n entries.
// Written by the sort in calls that keep their pair rows CHUNK-cell-major (View::pairchunks: calls of >=
// HGS_CHUNK_ROWS_MIN_VIEWS views); both blend kernels overwrite their copy of the word with the list position when they gather
// a record, the pair reduction hgs_k_pair_reduce_ch reads it: the entry's 16-bit cell mask, its place in the 64-record CHUNK of
// the tile list it belongs to (chunks start at the tile's first record), the chunk's record count - 1, and the layout of the
// chunk's pair rows.  Which row layout the sort leaves, and when:
//  * entry-major ids (calls of 1-2 views: no tag at all; and, tag bit clear, the long-list sort classes of every call):
//    entpair.y = the entry's first row, the rows of an entry are neighbours in cell order; the reduction streams the rows of 64
//    entries as one contiguous block (17 us per view) - the blend backward pays with isolated 40 B stores (+3 us);
//  * chunk-cell-major ids (tag bit set: the LDS sort class in calls of >= 3 views): the rows of every 64-record chunk of the tile
//    list are one block starting at entpair.y, cell by cell, inside a cell in list order: a 16-record batch of the backward
//    writes one or two contiguous runs of rows - with 8 views in flight the isolated stores made it bandwidth-bound
//    (428 -> 273 us) - and the reduction still reads blocks.
#define HGS_CHUNK_RECS 64u            // records per chunk
#define HGS_TAG_MASK_BITS 16          // [0, 16): cell mask
#define HGS_TAG_POS_SHIFT 16          // [16, 22): position in the chunk
#define HGS_TAG_COUNT_SHIFT 22        // [22, 28): records of the chunk - 1
#define HGS_TAG_ROWS_SHIFT 28         // bit 28: chunk-cell-major rows
#define HGS_TAG_CHUNK_BITS 6
#define HGS_TAG_CHUNK_FIELD ((1u << HGS_TAG_CHUNK_BITS) - 1u)
static_assert(HGS_TAG_MASK_BITS == HGS_CELLS_PER_TILE, "one mask bit per cell");
static_assert(HGS_CHUNK_RECS == 1u << HGS_TAG_CHUNK_BITS, "position and count - 1 of a 64-record chunk fit their 6-bit fields");
static_assert(HGS_TAG_POS_SHIFT >= HGS_TAG_MASK_BITS && HGS_TAG_COUNT_SHIFT >= HGS_TAG_POS_SHIFT + HGS_TAG_CHUNK_BITS &&
              HGS_TAG_ROWS_SHIFT >= HGS_TAG_COUNT_SHIFT + HGS_TAG_CHUNK_BITS && HGS_TAG_ROWS_SHIFT < 32,
              "the four tag fields do not overlap");

HGS_HD uint32_t hgs_rec_tag(uint32_t mask, uint32_t k, uint32_t n, bool chunk_rows) {
  const uint32_t left = n - (k & ~(HGS_CHUNK_RECS - 1u));
  return (mask & 0xffffu) | ((k & (HGS_CHUNK_RECS - 1u)) << HGS_TAG_POS_SHIFT) |
         (((left < HGS_CHUNK_RECS ? left : HGS_CHUNK_RECS) - 1u) << HGS_TAG_COUNT_SHIFT) | (chunk_rows ? 1u << HGS_TAG_ROWS_SHIFT : 0u);
}
HGS_HD uint32_t hgs_tag_mask(uint32_t tag) { return tag & 0xffffu; }
HGS_HD uint32_t hgs_tag_pos(uint32_t tag) { return (tag >> HGS_TAG_POS_SHIFT) & HGS_TAG_CHUNK_FIELD; }              // position in the chunk
HGS_HD uint32_t hgs_tag_count(uint32_t tag) { return ((tag >> HGS_TAG_COUNT_SHIFT) & HGS_TAG_CHUNK_FIELD) + 1u; }   // records of the chunk
HGS_HD bool hgs_tag_chunk_rows(uint32_t tag) { return ((tag >> HGS_TAG_ROWS_SHIFT) & 1u) != 0u; }

// ---- entpair.x: the entry id below the entry's pair count (0 .. 16: the set bits of its cell mask)
#define HGS_PAIRS_PER_ENTRY 16 // capacity of the pair arrays per entry of capacity (worst case: every cell)
#define HGS_ENTRY_BITS 27
#define HGS_ENTRY_MASK ((1u << HGS_ENTRY_BITS) - 1u)
static_assert(HGS_MAX_ENTRY_CAPACITY == 1ll << HGS_ENTRY_BITS, "the ABI's capacity limit is what the entry field holds");
static_assert(HGS_PAIRS_PER_ENTRY < (1 << (32 - HGS_ENTRY_BITS)), "the pair count fits above the entry id");
static_assert(HGS_PAIRS_PER_ENTRY == HGS_CELLS_PER_TILE, "an entry has at most one pair per cell");

HGS_HD uint32_t hgs_entpair_x(uint32_t entry, uint32_t pairs) { return entry | (pairs << HGS_ENTRY_BITS); }
HGS_HD uint32_t hgs_entpair_entry(uint32_t x) { return x & HGS_ENTRY_MASK; }
HGS_HD uint32_t hgs_entpair_pairs(uint32_t x) { return x >> HGS_ENTRY_BITS; }

// ---- cell key of the forward / backward work items: global tile g (view * T + tile), cell c
#define HGS_CELL_KEY_BITS 4
static_assert(HGS_CELLS_PER_TILE == 1 << HGS_CELL_KEY_BITS, "the cell index is the key's low bits");
HGS_HD uint32_t hgs_cell_key(uint32_t g, uint32_t c) { return g * (uint32_t)HGS_CELLS_PER_TILE + c; }
HGS_HD int hgs_cell_key_tile(uint32_t key) { return (int)(key >> HGS_CELL_KEY_BITS); }
HGS_HD int hgs_cell_key_cell(uint32_t key) { return (int)(key & ((1u << HGS_CELL_KEY_BITS) - 1u)); }
