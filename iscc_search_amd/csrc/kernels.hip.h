// kernels.hip.h -- gfx950 (MI355X, CDNA4) device code of the brute-force Hamming / NPHD k-NN path.
//
// What is computed (reference: docs/explanation/similarity-search.md:24-29, call sites
// iscc_search/indexes/usearch/index.py:2037 and iscc_search/indexes/simprint/usearch_core.py:165):
// for every query the k stored codes with the smallest (hamming over the common prefix, key).
//
// Data layout: a table is split into SEGMENTS by code length in bytes; inside a
// segment all codes have the same length, so a (query class, segment) pass is a FIXED-length
// Hamming scan over W = ceil(p/8) 64-bit words, p = min(query bytes, segment bytes).  Codes are
// stored structure-of-arrays by word: col[w][row] (uint64, big-endian packed), keys[row*KW].
//
// One header per family (this file keeps Record and is what isccsearch.hip includes):
//   valu_scan_kernel.hip.h
//     scan_kernel    THE hot kernel: streams col[0..W) once per group of TQ queries; queries and
//                    thresholds live in SGPRs; per (row, query) 2 v_xor + 2 v_bcnt per word and half a
//                    v_min3; a lane leaves the streaming loop only when one of its rows beats a
//                    threshold (MODE_HIST: count it, MODE_COLLECT: append (hamming,row) to the
//                    query's candidate list).  Wide query groups (TQ*W >= 24) hold their queries in
//                    LDS instead of SGPRs (queries_in_lds).
//     scan_adapt_kernel   whole 64-bit codes: the plain and the OR-folded fast path, chosen per query group
//   threshold_kernels.hip.h
//     boot_kernel, boot_multi_kernel   threshold bootstrap: exact histogram of the first S0 rows -> per-query bias
//     radius_init_kernel  range-limited searches: the given threshold for every query (no bootstrap, no samples)
//     pick_kernel    threshold from the sample histogram
//     fullhist_kernel exact histogram of one query over a whole segment (overflow fallback)
//   select_kernels.hip.h
//     select_kernel  per query: exact radix select over (hamming, key) of the candidates, bitonic
//                    sort of the k winners in LDS, emit records
//     tiny_search_kernel  a segment of a few thousand rows: distances, candidates and select in one launch
//     fb_keyhist_kernel, fb_collect_kernel   radix select on the key over the table's rows (overflow fallback)
//     merge_kernel   k-way merge of sorted record lists (segments of a table, shards of a node)
//     distinct_kernel     document frequency: distinct assets in a key-ordered collision list
//   table_kernels.hip.h
//     small utilities (synthetic fill, row moves, row / frequency gathers, ingest split); the sort-based
//     frequency column lives in docfreq.hip
//
// No MFMA: this is integer bit work bound by HBM reads (roofline in DESIGN.md section 4).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "scan_params.hip.h"

namespace isk {

struct Record {            // == isccsearch_record (24 bytes)
    uint64_t key_hi;
    uint64_t key_lo;
    uint32_t dist_rank;
    uint16_t hamming;
    uint16_t prefix_bits;
};
static_assert(sizeof(Record) == 24, "record layout");

}  // namespace isk

#include "valu_scan_kernel.hip.h"
#include "threshold_kernels.hip.h"
#include "select_kernels.hip.h"
#include "table_kernels.hip.h"
