// Aggregation of isccsearch_join_overlaps (internal interface between isccsearch.hip -- join_api.hip.h -- and overlap.hip).
//
// The OVERLAP form of the join kernels (join.hip.h) appends two directed hits per chunk pair, in no particular order.  Here they
// become one record per ordered pair of assets (isccsearch_overlap of include/isccsearch.h), sorted by (src, dst).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>

#include "../../include/isccsearch.h"

namespace iskov {

// one directed hit: row `row` of asset `src` has a row of asset `dst` at distance `hamming`.  An unused slot is all ones.
struct alignas(16) Hit { uint32_t src, dst, row, hamming; };
static_assert(sizeof(Hit) == 16, "the join kernels store a hit as one uint4");
constexpr uint32_t NO_ASSET = 0xFFFFFFFFu;      // src of an unused slot: no label has this value

// bytes of temporary storage aggregate() needs for m hits
int aggregate_temp_bytes(uint64_t m, size_t* bytes, std::string* err);

// All pointers are device memory.  hits[m]: the kernels' output, every unused slot all ones (the caller fills the buffer with 0xFF
// before the launches, so m is known without asking the device how many were written); overwritten.  sorted[m], marks[m],
// records[m] and temp[temp_bytes] are the call's scratch: 96 bytes per hit with the hits themselves.  On return (queued on
// `stream`, nothing is awaited): records[0 .. *n_records) hold one record per (src, dst) in ascending order -- followed, when any
// slot was unused, by ONE more whose src is NO_ASSET -- and *n_records counts them all.  Returns 0, or a negative errno-style code
// with *err describing it.
int aggregate(Hit* hits, Hit* sorted, isccsearch_overlap* marks, isccsearch_overlap* records, unsigned long long* n_records, uint64_t m,
              void* temp, size_t temp_bytes, hipStream_t stream, std::string* err);

}  // namespace iskov
