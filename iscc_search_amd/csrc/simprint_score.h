// Simprint asset scoring on the device (internal interface between isccsearch.hip -- search_api.hip.h, simprint_api.hip.h -- and simprint_score.hip).
//
// What UsearchSimprintIndex.search_raw does AFTER its batched neighbour search
// (iscc_search/indexes/simprint/usearch_core.py:171-269): threshold on the distance, best chunk per (asset, query
// simprint) in (query, rank) visiting order, IDF-weighted mean per asset in the reference's order of float64
// additions, order (-score, asset), first `limit`.  Input: the neighbour lists as select_kernel left them in
// device memory -- records [nq][k] ascending (hamming, key), the segment row of every record, counts [nq].
//
// The stages, once; the four pipelines below are lists of them.
//   per batch of <= 1 024 query simprints (queue_batch, queued behind its select_kernel, before the batch's one synchronisation):
//     mark     one block per query: matches = the prefix with hamming <= h_max; first occurrence of every asset in it
//              (LDS hash: asset -> smallest rank) = the best chunk of (asset, query); the query's own document
//              frequency from its hamming-0 prefix
//     offsets  exclusive scan of the per-query best counts (one block)
//     compact  the best entries of the batch, in (query, rank) order, appended to (asset[], entry[])
//   once per request or round, over the entries:
//     by asset stable radix sort by asset (rocPRIM) -> every asset's entries adjacent, ascending query
//     weights  per sorted entry its IDF weight, weight x similarity and query index, contiguous; values from host-computed tables
//              (log() of the host libm = CPython's math.log)
//     score    one thread per run of entries, sequential float64 sums in the reference's order (no contraction into fused
//              multiply-adds: -ffp-contract=off; IEEE rounding), one LDS row of a bit per query simprint per thread
//     by score stable radix sort by score, descending (assets are ascending already: ties keep ascending asset order)
//     emit     the first `limit` assets (+ the chunk records of their entries) written straight into pinned host memory
// Where the pipelines differ:
//   queue_score       (one request; a round of isccsearch_simprint_score_many that holds one request takes it too)
//                     by asset, weights, score with a run = an asset, by score, emit with a block per result
//   queue_score_many  (a round of several requests) a stable sort by request behind each of the two sorts, so that a run = a
//                     (request, asset) pair and every request's assets end up in (-score, asset) order: two more sorts, their key
//                     and gather kernels, and a scan of the chunks per result.  The same score kernel, instantiated for such runs;
//                     emit with a wave per result.  See ManyBuffers.
//   queue_exact       (hard-boundary requests) the entries are collisions (exact_prepare and a compaction of its own instead of
//                     queue_batch); by asset, weights and score in the exact form (coverage x quality, no similarity), by score, the
//                     same emit kernel writing collision records.
//   queue_exact_many  (a round of several hard-boundary requests) queue_exact's stages with queue_score_many's regrouping: the
//                     compaction of the round's collisions, by asset, by request, weights, the exact score kernel instantiated for
//                     (request, asset) runs, by score, by request, the scan of the chunks per result, emit with a wave per result
//                     writing collision records.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/isccsearch.h"

namespace isksp {

constexpr uint32_t MAX_QUERY_SIMPRINTS = 8192;   // score_kernel keeps one bit per query simprint and thread in LDS (64 threads x 1 KB)
constexpr uint32_t INFO_WORDS = 4;   // per batch, behind counts / flags / k-th distances: {entries appended so far, some query's
                                     // document frequency could not be read off its list, -, -}

// device buffers of one request (owned by the handle, grown on demand)
struct Buffers {
    const isccsearch_record* rec;   // [nq][k]
    const uint32_t* rows;           // [nq][k] segment row of every record
    uint8_t* best;                  // [nq][k] 1 = best chunk of its (asset, query)
    uint32_t* nbest;                // [nq]
    uint32_t* offs;                 // [nq] position of a query's first best entry in the compacted arrays
    uint32_t* freq_q;               // [nq] document frequency of the query simprint itself
    uint32_t* unknown;              // [nq] 1 = freq_q could not be decided from the list (k equal rows, k < dup_limit)
    uint64_t* c_asset[2];           // [nq*k] compacted asset ids (double buffer of the sort)
    uint32_t* c_entry[2];           // [nq*k] entry index q*k + rank
    double* score[2];               // [entries] per sorted entry: the asset's score at its run head, -1 elsewhere
    uint32_t* order[2];             // [entries] sort payload: index of the run head
    uint32_t* matches;              // [entries] matched query simprints of the run starting here
    double* ws;                     // [entries] IDF weight x similarity of every sorted entry
    double* idf_q;                  // [nq] IDF of every query simprint's own document frequency
    uint32_t* n_assets;             // [1]
    void* temp;                     // rocPRIM scratch
    size_t temp_bytes;
};

size_t sort_temp_bytes(size_t entries);

struct BatchArgs {
    uint32_t pos, m, k;             // queries [pos, pos + m) of the request, k neighbours each
    const uint32_t* cnt;            // [m] valid records per query (this batch)
    int h_max;                      // matches have hamming <= h_max (-1: none)
    uint32_t dup_limit;             // 0: frequencies are not wanted (every one is 1)
    uint32_t base;                  // entries appended by the batches before this one
    uint32_t* info;                 // [INFO_WORDS] device, travels to the host with the batch's counts
};
// mark + offsets + compact of one batch, queued on `stream`
hipError_t queue_batch(const Buffers& b, const BatchArgs& a, hipStream_t stream);

struct ScoreArgs {
    uint32_t nq, k, entries, limit;
    const double* sim_tab;          // [bits + 1] device: 1 - h / bits
    const double* idf_tab;          // [dup_limit + 1] device: idf of a document frequency (dup_limit == 0: one entry, idf of 1)
    uint32_t dup_limit;
    const uint32_t* freq_col;       // segment's document-frequency column (dup_limit > 0)
    const uint64_t* col[4];         // segment's code columns (chunk detail)
    uint32_t W;
    // pinned outputs
    isccsearch_simprint_result* out_results;   // [limit]
    isccsearch_simprint_chunk* out_chunks;     // nullable [limit * nq]
    uint64_t* out_chunk_words;                 // nullable [limit * nq * W]
    uint32_t* out_info;                        // [4] {results, assets matched, -, chunks written}
};
hipError_t queue_score(Buffers& b, const ScoreArgs& a, hipStream_t stream);

// Many requests in one call (a round of two or more requests of isccsearch_simprint_score_many): the query simprints of a round
// are the concatenation of its requests' (request r: queries [qbeg[r], qbeg[r + 1]) of the round), searched, marked and compacted
// as ONE request by queue_batch -- so the entries are grouped by request already.  The score kernel runs the unmatched sum over the
// run's own request only and counts assets per request; emit never takes a block per (request, rank) slot.
// Pinned outputs are staged compactly: request r's results follow those of the requests before it, its chunks likewise;
// out_info[4 r ..] = {results, assets matched, -, chunks written} -- the host moves them into the caller's per-request regions.
struct ManyBuffers {
    uint32_t* req[2];               // [entries] request index per entry (sort keys)
    uint32_t* idx[2];               // [entries] sort payload: position before the sort
    uint32_t* qbeg;                 // [n_req + 1] device: first query simprint of every request in the round
    uint32_t* n_assets;             // [n_req]
    uint32_t* a_start;              // [n_req + 1] first sorted position of every request's assets
    uint32_t* e_start;              // [n_req + 1] first written result of every request
    uint32_t* cnt;                  // [cap] chunks of every written result
    uint32_t* c_pos;                // [cap] their exclusive prefix: the result's first chunk in the staging block
};
size_t many_temp_bytes(size_t entries, size_t cap);

struct ScoreManyArgs {
    ScoreArgs s;                    // nq = query simprints of the round; out_results [cap]; out_chunks / words [<= entries];
    uint32_t n_req;                 //   out_info [n_req * 4]
    uint32_t cap;                   // min(entries, n_req x limit): results the round can write at most
    uint32_t words;                 // LDS words per thread of the score kernel: the most 64-bit words any request's range touches
};
hipError_t queue_score_many(Buffers& b, const ManyBuffers& mb, const ScoreManyArgs& a, hipStream_t stream);

// Hard-boundary requests (search_simprints_exact, lmdb_ops.py:169-301).  Buffers: rec = the collision lists [nd][k] of the DISTINCT
// query simprints, freq_q [nd] their document frequencies, nbest / unknown / offs sized for the GIVEN simprints [ng].
hipError_t exact_prepare(const Buffers& b, const uint32_t* cnt, const uint32_t* d_of_g, uint32_t nd, uint32_t ng, uint32_t k, uint32_t* info, hipStream_t stream);
struct ExactArgs {
    uint32_t nd, ng, k, entries, limit, queried;
    const uint32_t* d_of_g;         // [ng] device: distinct lookup of every given simprint
    double threshold;
    isccsearch_simprint_result* out_results;   // pinned [limit]
    isccsearch_simprint_chunk* out_chunks;     // pinned, nullable [entries]
    uint32_t* out_info;                        // pinned [4]
};
hipError_t queue_exact(Buffers& b, const ExactArgs& a, hipStream_t stream);

// Many hard-boundary requests in one call (a round of two or more requests of isccsearch_simprint_exact_many): the round's lookups
// are the concatenation of its requests' DISTINCT simprints (request r: lookups [dbeg[r], dbeg[r + 1])), its given simprints that of
// theirs (request r: [gbeg[r], gbeg[r + 1]) -- ManyBuffers::qbeg holds gbeg), d_of_g is round-global.  exact_prepare has run over the
// whole round.  A lookup belongs to one request, so the LDS row of a (request, asset) run holds the words of its request only.
// Pinned outputs are staged as queue_score_many's; a chunk's `query` is relative to its request's first given simprint.
struct ExactManyArgs {
    ExactArgs e;                    // nd / ng / entries of the round (queried unused); out_results [cap]; out_chunks [entries]; out_info [n_req * 4]
    uint32_t n_req;
    uint32_t cap;                   // min(entries, n_req x limit): results the round can write at most
    uint32_t words;                 // LDS words per thread of the score kernel: ceil(distinct simprints / 64) of the largest request
    const uint32_t* dbeg;           // [n_req + 1] device
    const uint32_t* queried;        // [n_req] device: query simprints every request was given (coverage denominator)
};
hipError_t queue_exact_many(Buffers& b, const ManyBuffers& mb, const ExactManyArgs& a, hipStream_t stream);

}  // namespace isksp
