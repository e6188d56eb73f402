// Asset scoring of unit searches on the device (internal interface between isccsearch.hip -- assets_api.hip.h -- and asset_score.hip).
//
// What UsearchIndex.search_assets does AFTER its per-unit searches (iscc_search/indexes/usearch/index.py:786-839), for many
// asset queries at once.  Input: every query's unit neighbour lists as select_kernel / merge_kernel left them in device memory
// (records ascending (distance, key), counts).  One block per asset query:
//   items    one per record: (key, position in the query's concatenated lists = unit slot, then rank)
//   sort     by (key, position) -- every key's records adjacent, first appearance first
//   groups   per key: its unit types in first-appearance order with the max score per type (score and score ** exponent from
//            host-computed tables indexed (prefix_bits / 8, hamming)); the threshold; sum(s) and sum(s ** e) over the confident
//            types in that order, sequential or Neumaier-compensated (CPython <= 3.11 / >= 3.12 `sum`); the quotient; the
//            self-exclusion key
//   sort     by (score descending, first appearance): Python's stable `sort(key=score, reverse=True)` over the insertion order
//   emit     the first `limit` assets, their scores and per-type scores, straight into pinned host memory
// The two sorts are bitonic sorts of one block, in LDS up to LDS_ITEMS items per array and in a per-block global scratch
// area beyond that (limit x units up to 4 096 x 64 records).  Built with -ffp-contract=off: the sums and the quotient must
// round as CPython's float operations do.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/isccsearch.h"

namespace iskas {

constexpr uint32_t BLOCK = 256;
constexpr uint32_t LDS_ITEMS = 2048;       // items per sort array held in LDS (two arrays: 64 KiB + the slot header)
constexpr uint32_t MAX_SLOTS = ISCCSEARCH_MAX_ASSET_UNITS;
constexpr uint32_t MAX_TYPES = ISCCSEARCH_MAX_UNIT_TYPES;
constexpr uint32_t TAB_BYTES = ISCCSEARCH_MAX_BYTES + 1;   // score tables are [prefix bytes 0..32][hamming 0..256]
constexpr uint32_t TAB_H = 257;
constexpr uint32_t TAB_SIZE = TAB_BYTES * TAB_H;

struct Item {                 // sort item, ordered by (a, b); b is unique within a sort
    uint64_t a;
    uint32_t b;
    uint32_t c;
};

struct Slot {                 // one unit list of one asset query
    const isccsearch_record* rec;   // its records (device)
    const uint32_t* cnt;            // its count (device)
    uint32_t k;                     // records the list holds at most
    uint32_t type;                  // unit type index (< n_types)
};

struct Params {
    const Slot* slots;
    const uint32_t* slot_off;    // [nq + 1]: slots of query q are [slot_off[q], slot_off[q + 1])
    const uint32_t* qlist;       // queries to score (nullptr: 0 .. n_list - 1)
    uint32_t n_list;
    const double* score_tab;     // [TAB_SIZE] max(0, 1 - float64(float32(h) / float32(8 p)))
    const double* pow_tab;       // [TAB_SIZE] score ** confidence_exponent as CPython computes it
    const uint64_t* exclude;     // [nq] self-exclusion key of every query
    const uint8_t* has_exclude;  // [nq]
    double threshold;
    int compensated;
    uint32_t limit, n_types;
    uint32_t lds_items;          // items per sort array in LDS (dynamic LDS = lds_bytes(lds_items))
    Item* scratch;               // per block 2 x scratch_items items, for queries with more records than lds_items
    uint32_t scratch_items;
    // pinned outputs
    uint64_t* out_keys;          // [nq][limit]
    double* out_scores;          // [nq][limit]
    uint32_t* out_count;         // [nq]
    uint8_t* out_types;          // [nq][limit][n_types] type indices in insertion order, 0xFF past the last
    double* out_type_scores;     // [nq][limit][n_types]
    uint32_t* out_slot_count;    // [total slots] the lists' counts as the search left them
};

size_t lds_bytes(uint32_t lds_items);
// the scoring of every listed query, queued on `stream`; `grid` blocks walk the list
hipError_t queue_assets(const Params& p, uint32_t grid, hipStream_t stream);
// raise the kernel's dynamic LDS limit on the current device (needed above 64 KiB)
hipError_t allow_lds(size_t bytes);

}  // namespace iskas
