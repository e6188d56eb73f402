// Aligned chunk runs of isccsearch_join_segments and isccsearch_join_segments_between (internal interface between isccsearch.hip --
// join_api.hip.h -- and segments.hip).
//
// The OVERLAP form of the join kernels (join.hip.h) stores the two directed hits of a chunk pair in adjacent slots of the hit buffer
// (overlap.h): slot 2s holds (la, lb, row_i, h), slot 2s + 1 holds (lb, la, row_j, h).  Here the chunk pairs of every pair of assets
// become SEGMENTS (isccsearch_segment of include/isccsearch.h): maximal runs of consecutive chunks of one asset that match
// consecutive chunks of the other, sorted by (src, dst, diagonal, first_src).  The hit buffer is only read: the aggregation of
// overlap.hip runs behind this stage and overwrites it.  The cross join of two tables stores the same two hits, la a label of one
// table and lb of the other; which of the two slots holds table_a's hit depends on which table the launch held, so the labels' side
// bit tells them apart, not the slot.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>

#include "../../include/isccsearch.h"
#include "overlap.h"

namespace isksg {

// a row's key as the store holds it: {asset, offset << 32 | size}
struct alignas(16) RowKey { uint64_t asset, place; };
static_assert(sizeof(RowKey) == 16, "the key column of a simprint table holds two words per row");

// the bit a label of table_b carries in the hits of a cross join (isk::LABEL_SIDE_B of join.hip.h; join_api.hip.h asserts they agree)
constexpr uint32_t SIDE_B = 0x80000000u;

// one side of the stage: a table's key column (device memory) and its row count
struct Side { const RowKey* keys; uint64_t n; };

// one chunk pair, oriented so that src < dst (two tables: src of table_a, dst of table_b, its side bit stripped).  `diagonal` is o_dst - o_src + 2^31 (ordinals stay below 2^31: the host refuses longer
// segments), so that unsigned order is the signed order of the difference.  An unused slot is all ones.
struct alignas(16) PairKey { uint32_t src, dst, diagonal, o_src, row_src, row_dst, hamming, reserved; };
static_assert(sizeof(PairKey) == 32, "a pair key is stored as two uint4");

// a run while it is reduced: the ordinals and rows of its first and its last pair, its length and distances
struct alignas(16) Run { uint32_t src, dst, first_src, first_dst, length, sum_hamming, last_src, row_first_src, row_first_dst, row_last_src, row_last_dst, reserved; };
static_assert(sizeof(Run) == sizeof(isccsearch_segment), "a run becomes its record in place");

// bytes of temporary storage locate() needs for sides of n_src and n_dst rows and `capacity` chunk pairs: the largest need of any
// of its steps, both tables' key sorts among them
int locate_temp_bytes(uint64_t n_src, uint64_t n_dst, uint64_t capacity, size_t* bytes, std::string* err);

// All pointers are device memory.  src, dst: the two sides.  The self-join passes its one side twice (the same column and count), and
// a pair is oriented so that src < dst; the cross join passes table_a as src and table_b as dst, and the labels' SIDE_B bit orients a
// pair.  hits[2 * capacity]: the join kernels' output, every unused slot all ones; read, not written.  Scratch: sorted_keys, sorted_rows
// and ordinals of src.n + dst.n entries each, the destination side's part behind the source side's (one table: src.n entries, one
// part); pairs[2 * capacity] {keyed | sorted}; runs[2 * capacity] {one-pair runs | reduced}; temp[temp_bytes].  Rows below 2^31 per
// side and capacity < 2^31 are the caller's to check.  Every row number read from the hits is bounded against the row count of the
// side it indexes before it is used.
// On return (queued on `stream`, nothing is awaited): the first *n_segments elements of runs + capacity, read as isccsearch_segment,
// are the segments in ascending order -- followed, when any slot was unused, by ONE more whose src is iskov::NO_ASSET -- and
// *n_segments counts them all.  Returns 0, or a negative errno-style code with *err describing it.
int locate(const Side& src, const Side& dst, const iskov::Hit* hits, uint64_t capacity, RowKey* sorted_keys, uint32_t* sorted_rows,
           uint32_t* ordinals, PairKey* pairs, Run* runs, unsigned long long* n_segments, void* temp, size_t temp_bytes,
           hipStream_t stream, std::string* err);

}  // namespace isksg
