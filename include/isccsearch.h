/*
 * isccsearch.h -- C-ABI of libisccsearch_hip.so, the MI355X (gfx950) brute-force
 * Hamming / NPHD k-nearest-neighbour engine behind the `hip:///` ISCC index backend.
 *
 * Drop-in boundary.  The reference (iscc/iscc-search, 100 % Python) reaches its hot path through
 * two third-party objects; every entry point below replaces one of their methods at the call
 * sites listed (paths relative to the reference tree):
 *
 *   iscc_usearch.ShardedNphdIndex   (metric = ISCCSEARCH_METRIC_NPHD, 64-bit keys)
 *     ctor    iscc_search/indexes/usearch/index.py:1617-1625   -> isccsearch_table_open
 *     .add    iscc_search/indexes/usearch/index.py:440         -> isccsearch_add
 *     .remove iscc_search/indexes/usearch/index.py:436         -> isccsearch_remove
 *     .search iscc_search/indexes/usearch/index.py:2037        -> isccsearch_search
 *     `in`    iscc_search/indexes/usearch/index.py:560         -> isccsearch_contains
 *     .size   iscc_search/indexes/usearch/index.py:444,1631    -> isccsearch_size
 *     .reset/.close  index.py:1699, :936                       -> isccsearch_table_drop / isccsearch_destroy
 *   iscc_usearch.ShardedIndex128    (metric = ISCCSEARCH_METRIC_HAMMING, 128-bit keys)
 *     ctor    iscc_search/indexes/simprint/usearch_core.py:73-83 -> isccsearch_table_open
 *     .add    iscc_search/indexes/simprint/usearch_core.py:108   -> isccsearch_add
 *     .remove iscc_search/indexes/simprint/usearch_core.py:119   -> isccsearch_remove
 *     .search iscc_search/indexes/simprint/usearch_core.py:165   -> isccsearch_search
 *     .get    iscc_search/indexes/simprint/usearch_core.py:221   -> isccsearch_get
 *     `in`    iscc_search/indexes/simprint/usearch_core.py:135   -> isccsearch_contains
 *   LMDB dupsort simprint table (hard-boundary matching and document frequency; the reference keeps it beside
 *   the ShardedIndex128, here the same device table answers both)
 *     search_simprints_exact  iscc_search/indexes/simprint/lmdb_ops.py:169-249 -> isccsearch_search_within (max_hamming 0)
 *     count_doc_freq          iscc_search/indexes/simprint/lmdb_ops.py:139-166 -> isccsearch_doc_freq (by code),
 *                                                                                 isccsearch_get_freq (by key)
 *   LMDB dupsort INSTANCE table
 *     _search_instance_unit   iscc_search/indexes/usearch/index.py:1957-2022   -> isccsearch_search_within (max_hamming 0)
 *
 * Unlike the reference's HNSW, every search here is EXACT: the k rows with the smallest
 * (distance, key), ascending, where distance is the rational hamming/prefix_bits for NPHD tables
 * and the raw bit count for Hamming tables (the reference leaves tie order unspecified,
 * iscc_search/indexes/usearch/index.py:836; this library defines it).
 *
 * Conventions
 *   - plain pointers and sizes only; the caller allocates every output; the library owns device memory
 *   - return 0 on success, a negative errno-style code otherwise; isccsearch_last_error() returns
 *     a thread-local human-readable message for the last failure on the calling thread
 *   - every entry point takes the handle's mutex: calls from many threads are serialised
 *   - codes are handed over as 64-bit words: the code's bytes packed BIG-ENDIAN (byte 0 is the
 *     most significant byte of word 0), zero padded to max_words = ceil(max_bytes / 8) words
 *   - 128-bit keys are two words (hi, lo) of the big-endian 16-byte key
 *     (iscc_search/indexes/simprint/lmdb_ops.py:30-49: iscc_id_body(8) | offset(4) | size(4))
 */
#ifndef ISCCSEARCH_H
#define ISCCSEARCH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ISCCSEARCH_METRIC_HAMMING 0 /* fixed length, distance = differing bits                    */
#define ISCCSEARCH_METRIC_NPHD    1 /* variable length, distance = hamming(prefix) / prefix bits  */

#define ISCCSEARCH_MAX_BYTES 32     /* longest code: 256 bits (index.py:135 max_dim)              */
#define ISCCSEARCH_MAX_K     4096   /* largest k per search (reference default limit 100; simprint
                                       oversampling 40 x limit = 4000, usearch_core.py:164)        */

#define ISCCSEARCH_ADD_TRUSTED_UNIQUE 1u /* caller guarantees the keys are new (usearch_core.py:89-92
                                            "skips the expensive contains-check")                   */

typedef struct isccsearch_handle isccsearch_handle;

/* One search result as it lives in device memory (multi-GPU exchange format, 24 bytes). */
typedef struct isccsearch_record {
    uint64_t key_hi;      /* 0 for 64-bit keys */
    uint64_t key_lo;
    uint32_t dist_rank;   /* order-preserving integer for the exact distance (library internal) */
    uint16_t hamming;     /* differing bits over the compared prefix */
    uint16_t prefix_bits; /* bits compared (NPHD denominator; table bit length for Hamming) */
} isccsearch_record;

typedef struct isccsearch_stats {
    uint64_t searches;        /* isccsearch_search* calls served                              */
    uint64_t queries;         /* queries answered                                             */
    uint64_t scan_launches;   /* launches of the collect scan kernel                          */
    uint64_t scan_passes;     /* query groups streamed over a segment by those launches       */
    uint64_t scan_bytes;      /* ALGORITHMIC bytes of those passes: rows * 8 * words compared */
    double   scan_ms;         /* summed device time of those launches (only while profiling)  */
    uint64_t sample_bytes;    /* ALGORITHMIC bytes of the threshold levels (first stretch, read once) */
    uint64_t fallback_queries;/* queries that took the exact full-histogram fallback          */
    uint32_t queries_per_pass;/* T_q: queries held in SGPRs per streaming pass                */
    uint32_t compute_units;   /* CUs of the device                                            */
    uint64_t freq_builds;     /* document-frequency columns (re)built by isccsearch_get_freq  */
    uint64_t mfma_launches;   /* scan launches (single pass, levels, collect) that ran on the matrix cores (FP4) */
    uint64_t mfma_pair_words; /* (row, query, 64-bit word) triples those launches scored: 128 operations each   */
    uint64_t scan_pair_words; /* (row, REAL query, word) triples of the collect launches counted in scan_launches / scan_ms */
    uint64_t scan_mfma_launches; /* how many of scan_launches ran on the matrix cores                          */
    /* the threshold levels (the first stretch of every segment, same scan kernels in MODE_BOTH), timed like the collect launches */
    uint64_t level_launches;
    uint64_t level_pair_words;
    uint64_t level_mfma_launches;
    double   level_ms;
    /* batches whose single self-tightening pass (k <= 512 on the matrix cores) overflowed a candidate list and were answered
       again with threshold levels, which prune after every level, before any query took the per-query exact fallback */
    uint64_t self_retries;
    uint64_t mfma_pack_launches; /* how many of mfma_launches ran the packed form (64-bit codes: two row tiles per accumulator) */
    /* small batches answered by ONE speculative range-limited pass under the previous search's k-th distance / sent on to the
       ordinary path because a query found fewer than k rows within it (or a list overflowed) */
    uint64_t spec_hits, spec_misses;
    /* with option "count_candidates" = 1: candidate-list entries the scan launches appended (summed over queries; the lists of the LAST pipeline run of
       every batch, read back after its synchronisation), and the batches they were counted over */
    uint64_t candidates, candidate_batches;
    /* kernel launches of isccsearch_join_within / isccsearch_join_between (and of the other join calls: components, degrees, live pairs,
       overlaps), and how many of them ran on the matrix cores */
    uint64_t join_launches, join_mfma_launches;
    /* queries that a fixed-radius pass of a large batch (option "radius_batches") left short of k rows and that were asked again,
       alone, under the whole hint -- counted when that second pass completed them (the step is then one of spec_hits) */
    uint64_t spec_repairs;
} isccsearch_stats;

/* Engine lifetime.  One handle drives one GPU (one process per GPU). */
int isccsearch_create(int device_id, isccsearch_handle** out);
int isccsearch_destroy(isccsearch_handle* h);
const char* isccsearch_last_error(void);

/* Options, by name: range, default, meaning (the measurements behind them: struct Options in csrc/isccsearch.hip).
 *   queries_per_pass    8|16      8      queries per streaming pass of the XOR + popcount kernel
 *   profile             0|1       0      time every scan launch with HIP events (read back through isccsearch_stats_get)
 *   count_candidates    0|1       0      read back how many candidates each batch's scan appended (stats candidates / candidate_batches)
 *   tiny_rows           0..2^20   16384  segments of at most this many rows are answered by ONE launch; 0: never
 *   select_wide_from    0..2^32-1 2048   selects whose sort buffer has at least this many slots run 1 024-thread blocks
 *   stretch_mb          0..65536  128    MB of rows per collect launch when several query groups share them; 0: one streaming pass
 *   mfma_stretch_factor 1..64     3      matrix-core launches whose query chunks share the rows take this many times stretch_mb
 *   mfma                0|1       1      large batches scan on the matrix cores (FP4 MFMA, exact sums) instead of XOR + popcount;
 *                                        0: no matrix cores anywhere, the joins included
 *   mfma_min_queries    1..1024   17     ... from this many queries (64-bit codes and segments of up to 12 Mi rows: from 9)
 *   mfma_min_rows       >= 1      65536  ... over at least this many rows
 *   join_mfma           0|1       1      isccsearch_join_within / _between run on the matrix cores too (same pairs, same order)
 *   join_mfma_min_rows  >= 0      65536  ... launches whose two segments both hold at least this many rows; 0: every launch
 *   mfma_pack           0|1       1      64-bit codes: the packed kernel (two row tiles per accumulator) unless a query is all zero
 *   mfma_pack3          0|1       1      ... three row tiles per accumulator for chunks of more than four query groups
 *   self_tighten        0|1       1      the matrix-core scan is ONE pass with self-tightening thresholds instead of threshold levels
 *   self_boot_rows      256..2^20 65536  ... bootstrapped from at least this many rows
 *   self_boot_per_k     0..2^20   1024   ... and this many per wanted neighbour
 *   speculate           0|1       1      small batches first try ONE range-limited pass under the previous k-th distance, verified
 *   spec_max_queries    0..1024   128    ... batches of up to this many queries
 *   self_hint           0|1       1      larger batches START their single pass under that hint instead of a sample, verified
 *   radius_batches      0|1       1      ... those that would run the three-tile kernel: ONE fixed-radius pass under the hint's worst k-th
 *                                        distance instead, the few queries it leaves short asked again under the hint; 0: the hinted single pass
 *   device_search_hint  -1..256   -1     one-shot: the next isccsearch_search_device_async starts under this distance (the caller verifies)
 *   candidate_cap       64..2^22  16384  floor of the per-query candidate buffer, in entries
 * An unknown name, a NULL argument or a value outside the range fails with -EINVAL and changes nothing. */
int isccsearch_set_option(isccsearch_handle* h, const char* name, int64_t value);
int isccsearch_get_option(isccsearch_handle* h, const char* name, int64_t* value);
int isccsearch_stats_get(isccsearch_handle* h, isccsearch_stats* out, int reset);

/* Tables.  max_bytes = longest code in bytes (1..32); for Hamming tables every code has exactly
 * max_bytes bytes.  key_words = 1 (u64 keys) or 2 (128-bit keys). */
int isccsearch_table_open(isccsearch_handle* h, int metric, int key_words, int max_bytes, uint32_t* table_id);
int isccsearch_table_drop(isccsearch_handle* h, uint32_t table);
int isccsearch_reserve(isccsearch_handle* h, uint32_t table, int nbytes, uint64_t rows);
uint64_t isccsearch_size(isccsearch_handle* h, uint32_t table);

/* Rows.  keys[n*key_words], code_words[n*max_words], nbytes[n] (NULL for Hamming tables).
 * A key that is already present (or repeated in the batch) fails the whole call with -EEXIST
 * unless ISCCSEARCH_ADD_TRUSTED_UNIQUE is set.
 * Bits past a code's length -- in its last word and in the words behind it -- are ignored on input and
 * stored as zero: isccsearch_get and isccsearch_export return them as zero whatever the caller left there. */
int isccsearch_add(isccsearch_handle* h, uint32_t table, uint64_t n, const uint64_t* keys,
                   const uint64_t* code_words, const uint8_t* nbytes, uint32_t flags);
int isccsearch_remove(isccsearch_handle* h, uint32_t table, uint64_t n, const uint64_t* keys, uint64_t* n_removed);
int isccsearch_contains(isccsearch_handle* h, uint32_t table, uint64_t n, const uint64_t* keys, uint8_t* out_found);
/* out_nbytes[i] = 0 when keys[i] is absent; out_words[n*max_words] zero padded */
int isccsearch_get(isccsearch_handle* h, uint32_t table, uint64_t n, const uint64_t* keys,
                   uint64_t* out_words, uint8_t* out_nbytes);

/* Snapshot support (the reference's flush/close/rebuild of HNSW shard files has no equivalent: codes live
 * in HBM; iscc_search/indexes/usearch/index.py:883-967).  Segments are addressed by code length in bytes.
 *   segments:    out_rows[ISCCSEARCH_MAX_BYTES + 1], out_rows[b] = rows whose codes are b bytes long
 *   export:      rows [first_row, first_row+n) of one segment: out_keys[n*key_words] and out_cols laid out
 *                COLUMN-major [W][n] (W = ceil(nbytes/8)), i.e. exactly the device layout
 *   add_columns: append n rows of one length from column-major words (no host transposition); bits past
 *                nbytes in the last column are ignored on input and stored as zero, as isccsearch_add does */
int isccsearch_segments(isccsearch_handle* h, uint32_t table, uint64_t* out_rows);
int isccsearch_export(isccsearch_handle* h, uint32_t table, int nbytes, uint64_t first_row, uint64_t n,
                      uint64_t* out_keys, uint64_t* out_cols);
int isccsearch_add_columns(isccsearch_handle* h, uint32_t table, int nbytes, uint64_t n, const uint64_t* keys,
                           const uint64_t* cols, uint32_t flags);

/* Bench / test helper: append n rows generated ON THE DEVICE, nbytes long each:
 *   word w of row i = splitmix64(seed + 4*(first_row + i) + w),  key = key_base + first_row + i
 * (SURVEY.md section 8d synthetic generator).  Rows are not entered into the host key index. */
int isccsearch_add_synthetic(isccsearch_handle* h, uint32_t table, int nbytes, uint64_t n,
                             uint64_t seed, uint64_t first_row, uint64_t key_base);

/* Exact k-NN.  q_words[nq*max_words], q_nbytes[nq] (NULL for Hamming tables), 1 <= k <= ISCCSEARCH_MAX_K.
 * Outputs: out_keys[nq*k*key_words], out_hamming[nq*k], out_prefix_bits[nq*k], out_count[nq]
 * (= min(k, rows)); entries past out_count are zero. */
int isccsearch_search(isccsearch_handle* h, uint32_t table, uint32_t nq, const uint64_t* q_words,
                      const uint8_t* q_nbytes, uint32_t k,
                      uint64_t* out_keys, uint32_t* out_hamming, uint16_t* out_prefix_bits, uint32_t* out_count);

/* Range-limited exact k-NN: as isccsearch_search, but only rows whose Hamming distance over the compared
 * prefix is <= max_hamming (0..256) are reported -- nearest first, ties by ascending key, at most k per query;
 * out_count[q] may be 0.  One streaming pass at a fixed threshold (no sampling passes).
 * max_hamming = 0 is the hard-boundary collision lookup the reference serves from its LMDB dupsort table
 * (search_simprints_exact, iscc_search/indexes/simprint/lmdb_ops.py:169-249; called with exact=True from
 * iscc_search/indexes/usearch/index.py:1261-1304): every row equal to the query, in ascending key order, which
 * is the byte order LMDB iterates duplicate chunk pointers in; k plays the part of its dup_limit (:197-203).
 * On an NPHD table the same call is the INSTANCE prefix match (usearch/index.py:1957-2022). */
int isccsearch_search_within(isccsearch_handle* h, uint32_t table, uint32_t nq, const uint64_t* q_words,
                             const uint8_t* q_nbytes, uint32_t k, uint32_t max_hamming,
                             uint64_t* out_keys, uint32_t* out_hamming, uint16_t* out_prefix_bits, uint32_t* out_count);

/* Several searches in one call, one device synchronisation: what UsearchIndex.search_assets issues as a sequence of
 * per-unit searches (similarity units iscc_search/indexes/usearch/index.py:786-806 -> :2037, INSTANCE unit :791-797
 * -> :1957-2022) for ONE request.  Request i is isccsearch_search (max_hamming < 0) or isccsearch_search_within
 * (max_hamming >= 0) on its own table with its own k and outputs; reqs[i].status receives its result code.  Returns 0
 * or the first request's error code (the others still ran). */
typedef struct isccsearch_request {
    uint32_t table, nq, k;
    int32_t max_hamming;
    const uint64_t* q_words;      /* [nq*max_words] */
    const uint8_t* q_nbytes;      /* [nq], NULL for Hamming tables */
    uint64_t* out_keys;           /* [nq*k*key_words] */
    uint32_t* out_hamming;        /* [nq*k] */
    uint16_t* out_prefix_bits;    /* [nq*k] */
    uint32_t* out_count;          /* [nq] */
    int32_t status;               /* out */
} isccsearch_request;
int isccsearch_search_many(isccsearch_handle* h, uint32_t n, isccsearch_request* reqs);

/* Document frequency of nq codes: out_freq[q] = number of DISTINCT assets among the first dup_limit rows
 * (ascending key) that equal code q.  The asset is the first key word of a 2-word key (the ISCC-ID body of a
 * chunk pointer, lmdb_ops.py:30-49); with 1-word keys every row is its own asset.
 * Replaces count_doc_freq (lmdb_ops.py:139-166, called per matched simprint from usearch/index.py:1395-1403). */
int isccsearch_doc_freq(isccsearch_handle* h, uint32_t table, uint32_t nq, const uint64_t* q_words,
                        const uint8_t* q_nbytes, uint32_t dup_limit, uint32_t* out_freq);
/* The same, and out_collisions[q] = how many rows equal to code q were looked at (<= dup_limit).  What a table SHARDED by
 * asset needs (sharded_engine.py: an asset's chunks share a rank): when the collisions of all shards together stay within
 * dup_limit -- the normal case -- the shards' distinct-asset counts simply add; only otherwise is the merged list needed.
 * Same reference call site: count_doc_freq, lmdb_ops.py:139-166. */
int isccsearch_doc_freq_counted(isccsearch_handle* h, uint32_t table, uint32_t nq, const uint64_t* q_words,
                                const uint8_t* q_nbytes, uint32_t dup_limit, uint32_t* out_freq, uint32_t* out_collisions);

/* Document frequency of STORED codes, by key: out_freq[i] = frequency (as isccsearch_doc_freq defines it) of
 * the code stored under keys[i], 0 when the key is absent.  Served from a per-segment frequency column that is
 * built on the device by sorting the rows by (code, asset) and is rebuilt lazily after rows were added or
 * removed -- so the per-match lookups of the approximate simprint path (doc_freq_fn called once per matched
 * chunk, usearch/index.py:1395-1403 -> usearch_core.py:201-236) cost one gather instead of one scan each.
 * Hamming (fixed-length) tables only. */
int isccsearch_get_freq(isccsearch_handle* h, uint32_t table, uint64_t n, const uint64_t* keys,
                        uint32_t dup_limit, uint32_t* out_freq);

/* Simprint search WITH its asset scoring, on the device: what UsearchSimprintIndex.search_raw does in one call
 * (iscc_search/indexes/simprint/usearch_core.py:137-269) -- the oversampled batched neighbour search (:161-165, `count` =
 * limit x oversampling neighbours per query simprint; max_hamming >= 0 lists the rows within that radius instead, see
 * isccsearch_search_within), then on the neighbour lists as they lie in device memory: the match threshold on
 * score = 1 - distance / ndim (:182-184), the best chunk per (asset, query simprint) in the reference's visiting order
 * (:175-196; the asset is the first word of the 128-bit chunk-pointer key), the IDF-weighted mean per asset in the
 * reference's ORDER of float64 additions (:215-236, idf = log(1 + total_assets / (1 + freq)), lmdb_ops.py:67-81, with log()
 * of the host libm), order (-score, asset) and the cut to `limit` (:268-269).  Only the <= limit winners (and, when
 * out_chunks is given, their matched chunks: `detailed`, :238-255) leave the device.
 *   dup_limit > 0   document frequencies are the device's: of a matched STORED simprint from the table's frequency column
 *                   (isccsearch_get_freq), of an unmatched QUERY simprint the distinct assets among its first dup_limit
 *                   collisions (isccsearch_doc_freq) -- what the reference's doc_freq_fn computes with an LMDB cursor walk
 *                   (usearch/index.py:1395-1403, lmdb_ops.py:139-166)
 *   dup_limit == 0  every frequency is 1 (the reference's doc_freq_fn = None, :204-211)
 * 128-bit-key Hamming tables only, nq <= ISCCSEARCH_MAX_SCORED_SIMPRINTS.  out_results[limit]; out_chunks[limit * nq] and out_chunk_words[limit * nq * max_words]
 * (both or neither; chunks of result r are out_chunks[first_chunk .. first_chunk + matches), ascending query index, words =
 * the STORED simprint); out_info[4] = {results written, assets matched, longest neighbour list (what a caller that asked for
 * a radius compares with `count` to see a list that filled the cap), chunks written}. */
#define ISCCSEARCH_MAX_SCORED_SIMPRINTS 8192
typedef struct isccsearch_simprint_result {
    uint64_t asset;        /* first key word: ISCC-ID body */
    double   score;
    uint32_t matches;      /* query simprints matched by this asset */
    uint32_t first_chunk;  /* index of its first entry in out_chunks */
} isccsearch_simprint_result;
typedef struct isccsearch_simprint_chunk {
    uint64_t key_lo;       /* second key word: offset (high 32 bits) | size (low 32 bits) */
    uint32_t query;        /* index of the query simprint */
    uint32_t hamming;      /* differing bits: score = 1 - hamming / ndim */
    uint32_t freq;         /* document frequency of the stored simprint (1 when dup_limit == 0) */
    uint32_t reserved;
} isccsearch_simprint_chunk;
int isccsearch_simprint_score(isccsearch_handle* h, uint32_t table, uint32_t nq, const uint64_t* q_words,
                              uint32_t count, int32_t max_hamming, double threshold, uint32_t limit,
                              int64_t total_assets, uint32_t dup_limit,
                              isccsearch_simprint_result* out_results, isccsearch_simprint_chunk* out_chunks,
                              uint64_t* out_chunk_words, uint32_t* out_info);

/* Many simprint requests against ONE table in one call, each scored on its own: what isccsearch_simprint_score returns for
 * every request alone, bit for bit -- UsearchSimprintIndex.search_raw once per simprint type and asset query
 * (iscc_search/indexes/usearch/index.py:1357-1469 -> usearch_core.py:137-269).  Request r holds the query simprints
 * q_words[req_offsets[r] .. req_offsets[r + 1]) (req_offsets[n_req + 1], non-decreasing; empty requests are allowed), at most
 * ISCCSEARCH_MAX_SCORED_SIMPRINTS each (-E2BIG).  count, max_hamming, threshold, limit, total_assets and dup_limit are shared.
 * The library cuts the requests into rounds of at most ISCCSEARCH_MAX_SCORED_SIMPRINTS query simprints (never splitting a
 * request); a round is ONE batched search of its simprints and one scoring pipeline that keeps the requests apart.
 * Outputs per request r: out_results[r * limit ..] (its first min(limit, assets) results); out_info[4 r .. 4 r + 4) = {results
 * written, assets matched, longest neighbour list OF THIS REQUEST, chunks written}; out_chunks / out_chunk_words (both or
 * neither) laid out as isccsearch_simprint_score's, request r's starting at limit * req_offsets[r] (out_chunks[limit * total],
 * total = req_offsets[n_req]), first_chunk and the chunks' `query` relative to the request.  128-bit-key Hamming tables only. */
int isccsearch_simprint_score_many(isccsearch_handle* h, uint32_t table, uint32_t n_req, const uint32_t* req_offsets, const uint64_t* q_words,
                                   uint32_t count, int32_t max_hamming, double threshold, uint32_t limit,
                                   int64_t total_assets, uint32_t dup_limit,
                                   isccsearch_simprint_result* out_results, isccsearch_simprint_chunk* out_chunks,
                                   uint64_t* out_chunk_words, uint32_t* out_info);

/* Hard-boundary simprint search WITH its scoring, on the device: search_simprints_exact (iscc_search/indexes/simprint/lmdb_ops.py:169-301,
 * called with exact=True from iscc_search/indexes/usearch/index.py:1261-1304).  q_words[n_distinct * max_words] are the DISTINCT query
 * simprints; given[n_given] names, for every query simprint of valid length AS GIVEN (repeats included: a repeated simprint is matched
 * again, :197), its index among the distinct ones; `queried` = the number of query simprints the caller was given (the denominator
 * of the coverage, :286).  Per distinct simprint every stored row EQUAL to it is listed in ascending key order, at most dup_limit
 * (:199-210; capped at ISCCSEARCH_MAX_K); on those lists, in device memory: document frequencies (distinct assets per list, :213-215),
 * the matches of every asset in visiting order, coverage x quality (:252-301) with the reference's float64 operations in the
 * reference's order, the threshold (:222-223), order (-score, asset) and the cut to `limit` (:247-248).
 * out_results[limit]; out_chunks (nullable) [sum of list lengths over the given simprints]: chunks of result r are out_chunks[first_chunk
 * .. first_chunk + matches), in visiting order -- `query` = position in given[], hamming 0, freq = the simprint's document frequency;
 * out_info[4] = {results written, assets kept, longest collision list, chunks written}.  128-bit-key Hamming tables only. */
int isccsearch_simprint_exact(isccsearch_handle* h, uint32_t table, uint32_t n_distinct, const uint64_t* q_words,
                              uint32_t n_given, const uint32_t* given, uint32_t queried, uint32_t dup_limit, double threshold, uint32_t limit,
                              isccsearch_simprint_result* out_results, isccsearch_simprint_chunk* out_chunks, uint32_t* out_info);

/* Many hard-boundary requests against ONE table in one call, each searched and scored on its own: what isccsearch_simprint_exact
 * returns for every request alone -- assets, matches, order, first_chunk and the chunks' `query` relative to the request, the
 * float64 scores bit for bit.  Request r holds the DISTINCT simprints q_words[distinct_offsets[r] .. distinct_offsets[r + 1]) and
 * the given ones given[given_offsets[r] .. given_offsets[r + 1]) (both offset arrays [n_req + 1], non-decreasing; empty requests are
 * allowed); a `given` value is the index of the simprint among ITS REQUEST's distinct ones (local, 0-based); queried[r] = the
 * query simprints request r was given (its coverage denominator, >= its given count).  A simprint asked by two requests is looked
 * up twice.  At most ISCCSEARCH_MAX_SCORED_SIMPRINTS distinct and as many given simprints per request (-E2BIG).  dup_limit,
 * threshold and limit are shared.  The library cuts the requests into rounds of at most ISCCSEARCH_MAX_SCORED_SIMPRINTS given and
 * at most as many distinct simprints (never splitting a request); a round is ONE search of its distinct simprints at distance 0,
 * k = min(dup_limit, ISCCSEARCH_MAX_K) rows each, and one scoring pipeline that keeps the requests apart.
 * Outputs per request r: out_results[r * limit ..]; out_chunks (nullable) request r's starting at k * given_offsets[r]
 * (out_chunks[k * given_offsets[n_req]]); out_info[4 r .. 4 r + 4) = {results written, assets kept, longest collision list OF
 * THIS REQUEST, chunks written}.  128-bit-key Hamming tables only. */
int isccsearch_simprint_exact_many(isccsearch_handle* h, uint32_t table, uint32_t n_req, const uint32_t* distinct_offsets, const uint64_t* q_words,
                                   const uint32_t* given_offsets, const uint32_t* given, const uint32_t* queried,
                                   uint32_t dup_limit, double threshold, uint32_t limit,
                                   isccsearch_simprint_result* out_results, isccsearch_simprint_chunk* out_chunks, uint32_t* out_info);

/* Many asset queries in one call, scored on the device: what UsearchIndex.search_assets does for the units of ONE query
 * (iscc_search/indexes/usearch/index.py:786-839 -- one search per similarity unit, :2024-2045, one prefix match per INSTANCE
 * unit, :1957-2045; the max per (asset, unit type), the threshold, sum(s ** e) / sum(s) over the confident types, the
 * self-exclusion, the stable sort by score and the cut to `limit`) for nq <= 1 024 queries at once.  Query q holds the units
 * units[unit_offsets[q] .. unit_offsets[q + 1]) (at most ISCCSEARCH_MAX_ASSET_UNITS), in the query's order.  The units of
 * all queries are searched as ONE batch per (table, code length, kind); the lists stay on the device, where one block per
 * query groups them by asset (asset_score.hip).  INSTANCE units (max_hamming = 0) list instance_first_k rows first; the
 * lists that came back full are searched again with instance_max_k.
 *   score_table / pow_table   [(ISCCSEARCH_MAX_BYTES + 1) x 257] host-computed: entry [prefix_bits / 8][hamming] holds the unit
 *                             score max(0, 1 - float64(float32(h) / float32(prefix_bits))) and its power score ** exponent
 *   exclude / has_exclude     [nq] per query the asset key left out of its results (an iscc_id query's own asset)
 *   compensated               0: sums are sequential float64 additions (CPython <= 3.11 sum), 1: Neumaier's compensated form (>= 3.12)
 * Outputs: out_keys[nq*limit], out_scores[nq*limit] (min(1, total)), out_count[nq]; per result its unit types in insertion
 * order out_types[nq*limit*n_types] (type index, 0xFF past the last) with their scores out_type_scores[nq*limit*n_types];
 * out_unit_count[total units] the final length of every unit's list (an INSTANCE list that reaches instance_max_k was cut). */
#define ISCCSEARCH_MAX_ASSET_UNITS 64
#define ISCCSEARCH_MAX_UNIT_TYPES  16
typedef struct isccsearch_asset_unit {
    uint32_t table;       /* NPHD table of the unit's type, 64-bit keys */
    uint32_t type;        /* index of the unit type (< n_types) */
    int32_t max_hamming;  /* < 0: similarity unit (k = limit); 0: INSTANCE prefix match */
    uint32_t nbytes;      /* code length in bytes */
    uint64_t words[4];    /* the code, packed as for isccsearch_search */
} isccsearch_asset_unit;
int isccsearch_match_assets(isccsearch_handle* h, uint32_t nq, const uint32_t* unit_offsets, const isccsearch_asset_unit* units,
                            uint32_t limit, uint32_t instance_first_k, uint32_t instance_max_k,
                            const uint64_t* exclude, const uint8_t* has_exclude,
                            const double* score_table, const double* pow_table, double threshold, int compensated, uint32_t n_types,
                            uint64_t* out_keys, double* out_scores, uint32_t* out_count, uint8_t* out_types, double* out_type_scores,
                            uint32_t* out_unit_count);

/* All unordered pairs of distinct rows of ONE table whose Hamming distance over their common prefix of p bytes is
 * <= max_hamming[p] (p = 1..32; entry 0 unused; a negative entry: no pair with that prefix qualifies).  NPHD tables
 * compare min(len_a, len_b) bytes, as isccsearch_search does; HAMMING tables compare their one length.
 * On success (*out_total <= capacity): pairs in out_*[0 .. *out_total), key_a < key_b (128-bit keys compared as
 * (hi, lo) unsigned), sorted ascending by (key_a, key_b).  out_keys_a / out_keys_b hold key_words words per pair.
 * If *out_total > capacity: returns -ENOSPC with *out_total set and the outputs unspecified, so the caller can retry
 * with exactly that capacity.  Device memory for the outputs: capacity x (16 * key_words + 6) bytes.
 * No reference counterpart (the reference has no index-wide join). */
int isccsearch_join_within(isccsearch_handle* h, uint32_t table, const int16_t* max_hamming /* [33] */,
                           uint64_t capacity, uint64_t* out_keys_a, uint64_t* out_keys_b,
                           uint32_t* out_hamming, uint16_t* out_prefix_bits, uint64_t* out_total);

/* All pairs (row a of table_a, row b of table_b) of TWO tables of one handle whose Hamming distance over their common
 * prefix of p = min(len_a, len_b) bytes is <= max_hamming[p]: the prefix rule, the masking of a partial last word and the
 * meaning of max_hamming are those of isccsearch_join_within.  out_keys_a always holds the key from table_a and
 * out_keys_b the key from table_b (never swapped; a pair of equal keys -- one asset in both tables -- is a pair like any
 * other), sorted ascending by (key_a, key_b), 128-bit keys compared as (hi, lo) unsigned.  Capacity protocol and device
 * memory as for isccsearch_join_within: -ENOSPC with *out_total set, and a retry with exactly that capacity succeeds.
 * -EINVAL: table_a == table_b (isccsearch_join_within joins a table with itself), tables that differ in metric or
 * key_words, HAMMING tables that differ in max_bytes (NPHD tables may), NULL arguments as for isccsearch_join_within.
 * No reference counterpart (the reference has no index-wide join, within one index or between two). */
int isccsearch_join_between(isccsearch_handle* h, uint32_t table_a, uint32_t table_b,
                            const int16_t* max_hamming /* [33] */, uint64_t capacity,
                            uint64_t* out_keys_a, uint64_t* out_keys_b,
                            uint32_t* out_hamming, uint16_t* out_prefix_bits, uint64_t* out_total);

/* Connected components under the pairs of isccsearch_join_within, without the pairs: max_hamming, the prefix rule, the masking
 * and the launches (one per pair of segments, la <= lb, the larger segment held) are those of isccsearch_join_within, but a row
 * pair within its threshold is not written -- the labels of its two rows are united in a union-find array on the device.
 * Memory: 4 bytes per label and 4 bytes per row, whatever the number of pairs; the call has no capacity and no -ENOSPC.
 *   live_keys[n_live]    strictly ascending: the rows that take part.  A row of key live_keys[i] has label live_labels[i]
 *                        (< n_labels; several keys may share a label).  A row whose key is not listed has no label: it is
 *                        compared, but never linked and never counted.  A listed key the table does not hold does nothing.
 *                        Both arrays may be NULL only when n_live is 0.
 *   parent[n_labels]     in/out.  On entry a forest with parent[i] <= i for every i (the identity: no links yet).  On exit
 *                        FLAT: parent[i] is the smallest label of i's component under the links of the input forest plus one
 *                        link per qualifying row pair.  The output of one call is a valid input of the next (another table,
 *                        other thresholds): the components then are those of all the calls' pairs together.
 *   *out_links           the row pairs within their threshold whose two rows both have labels (for live_keys = all keys of the
 *                        table: the *out_total of isccsearch_join_within).
 * -EINVAL, each naming the offending index, all checked on the host before anything is launched, `parent` left unchanged:
 * a NULL argument; a table with key_words != 1; n_labels = 0 or 2^32 - 1 (the value that means "no label"); live_keys not
 * strictly ascending; a label >= n_labels; parent[i] > i (the bound of every loop of the device code: nothing runs on an
 * array that fails it).
 * No reference counterpart (the reference has no index-wide join and no grouping of its assets). */
int isccsearch_join_components(isccsearch_handle* h, uint32_t table, const int16_t* max_hamming /* [33] */,
                               uint64_t n_live, const uint64_t* live_keys, const uint32_t* live_labels,
                               uint32_t n_labels, uint32_t* parent /* in/out [n_labels] */, uint64_t* out_links);

/* The DEGREE of every listed row under the pairs of isccsearch_join_within, without the pairs: max_hamming, the prefix rule, the
 * masking and the launches (one per pair of segments, la <= lb, the larger segment held, the same dispatch between the kernels) are
 * those of isccsearch_join_within, but a row pair within its threshold is not written -- it adds 1 to a counter of either row on
 * the device.  Memory: 4 bytes per listed key and 4 bytes per row (and the 8 bytes of every listed key), whatever the number of
 * pairs, in the handle's scratch buffers; the call has no capacity and no -ENOSPC.  Which rows are the hubs of a table, and how
 * many near-duplicates each row has, is answered without materialising h * (h - 1) / 2 pairs per hub of h rows.
 *   live_keys[n_live]    strictly ascending: the rows that take part.  The LABEL of a row is the index of its key here.  A row
 *                        whose key is not listed is compared but never counted.  A listed key the table does not hold does
 *                        nothing; its degree is 0.  May be NULL only when n_live is 0 (as out_degree).
 *   out_degree[n_live]   out_degree[i]: the number of OTHER listed rows within the threshold of the row of live_keys[i].
 *   *out_links           the number of such pairs: sum(out_degree) == 2 * *out_links.  With every key of the table listed it is
 *                        the *out_total of isccsearch_join_within.
 * With fewer than two rows or n_live < 2 nothing is launched and the outputs are still filled (zeros).
 * -EINVAL, each naming the offending index, all checked on the host before anything is launched, the outputs left untouched:
 * a NULL argument; a table with key_words != 1; n_live >= 2^32 - 1 (the value that means "no label"); live_keys not strictly
 * ascending.  One lock covers the call; everything runs on the handle's one stream and ONE synchronisation comes before the
 * results are copied.  The launches count in stats join_launches / join_mfma_launches.
 * No reference counterpart (the reference has no index-wide join). */
int isccsearch_join_degrees(isccsearch_handle* h, uint32_t table, const int16_t* max_hamming /* [33] */,
                            uint64_t n_live, const uint64_t* live_keys,
                            uint32_t* out_degree /* [n_live] */, uint64_t* out_links);

/* isccsearch_join_within over the listed rows only: the pairs of isccsearch_join_within whose two rows' keys are both in
 * live_keys (strictly ascending; NULL only when n_live is 0; a row whose key is not listed is compared but takes no room and is
 * not counted; a listed key the table does not hold does nothing).  Outputs, their order and the capacity protocol are those of
 * isccsearch_join_within: -ENOSPC with *out_total exact, and a retry with exactly that capacity succeeds.  With every key of the
 * table listed the outputs are byte for byte those of isccsearch_join_within.  With fewer than two rows or n_live < 2 nothing is
 * launched and *out_total is 0.  Device memory: that of isccsearch_join_within plus 8 bytes per listed key and 4 bytes per row.
 * -EINVAL and execution as for isccsearch_join_degrees (64-bit keys only). */
int isccsearch_join_within_live(isccsearch_handle* h, uint32_t table, const int16_t* max_hamming /* [33] */,
                                uint64_t n_live, const uint64_t* live_keys, uint64_t capacity,
                                uint64_t* out_keys_a, uint64_t* out_keys_b,
                                uint32_t* out_hamming, uint16_t* out_prefix_bits, uint64_t* out_total);

/* The pairs of ASSETS that share chunks: a self-join of ONE simprint table (HAMMING, key_words 2, one code length of ndim bits),
 * aggregated on the device.  A row is a chunk; its asset is the first key word (the ISCC-ID body), the second is
 * offset << 32 | size.
 *   asset_keys[n_assets]  strictly ascending: the assets that take part.  The LABEL of an asset is its rank in this array.  A
 *                         row is live if its asset is listed; a listed asset the table does not hold has no rows.
 *   max_hamming           the radius, in bits over the ndim bits (>= 0; values above ndim mean ndim).
 *   max_doc_freq          a live row is a STOP CHUNK if its entry in the segment's frequency column, built with dup_limit (the
 *   dup_limit             value isccsearch_get_freq returns for it: distinct assets among the first dup_limit rows of equal code
 *                         by ascending key), is greater than max_doc_freq.  max_doc_freq 0: no cut, and the column is neither
 *                         read nor built (dup_limit is then not looked at).
 * A chunk pair is an unordered pair of rows (i, j), both live, neither a stop chunk, asset(i) != asset(j), hamming(i, j) <=
 * max_hamming.  Pairs of rows of one asset, rows of unlisted assets and stop chunks are compared, but take no room and are not
 * counted.
 *   out_pairs[2 * capacity]  one record per ORDERED pair of assets (src, dst) with at least one chunk pair -- so every unordered
 *                         pair of assets has two, (a, b) and (b, a) -- sorted ascending by (src, dst).  Every field is an integer
 *                         and defined by the set of chunk pairs alone: the records do not depend on which kernel ran (see the
 *                         options join_mfma, join_mfma_min_rows) or on the order in which pairs were found.
 *   out_chunks[n_assets]  live rows per asset, stop chunks included: the denominator of a coverage.
 *   out_info[4]           {chunk pairs found, records written, live rows, stop chunks}.
 * Capacity protocol as for isccsearch_join_within, counted in chunk pairs: more than `capacity` return -ENOSPC with out_info[0]
 * exact and every other output unspecified, and a retry with exactly that capacity succeeds; pairs past the capacity are
 * counted and not written.  Device memory: 192 bytes per chunk pair of the capacity, 4 bytes per row and 12 per asset, kept by
 * the handle as its other scratch buffers are.
 * -EINVAL, each naming the offending index, all checked on the host before anything is launched, the outputs left untouched:
 * a NULL argument (out_pairs may be NULL only when capacity is 0); a table that is not HAMMING with key_words 2; n_assets = 0 or
 * 2^32 - 1 (the value that means "no label"); asset_keys not strictly ascending; max_hamming < 0; max_doc_freq > dup_limit when
 * max_doc_freq > 0 (the column counts no further than dup_limit rows).  -E2BIG, checked likewise: a segment of 2^32 rows or more
 * (row numbers travel as 32 bits), a capacity of 2^31 chunk pairs or more (their hits are numbered with 32 bits).
 * One lock covers the call; everything runs on the handle's one stream -- labelling, the join launch (the one
 * isccsearch_join_within would make for the table), sort, reduction -- and ONE synchronisation comes before the results are copied.
 * No reference counterpart (the reference has no index-wide join: it finds shared chunks one query asset at a time). */
typedef struct isccsearch_overlap {
    uint32_t src, dst;       /* labels (ranks in asset_keys) */
    uint32_t matched;        /* distinct rows of src with >= 1 row of dst within max_hamming */
    uint32_t reserved;       /* 0 */
    uint64_t sum_hamming;    /* over those rows, the SMALLEST distance to a row of dst, summed */
    uint64_t chunk_pairs;    /* chunk pairs between the two assets (equal in both directions) */
} isccsearch_overlap;        /* 32 bytes */
int isccsearch_join_overlaps(isccsearch_handle* h, uint32_t table, int32_t max_hamming,
                             uint32_t max_doc_freq, uint32_t dup_limit,
                             uint32_t n_assets, const uint64_t* asset_keys,
                             uint64_t capacity,                    /* chunk pairs */
                             isccsearch_overlap* out_pairs,        /* [2 * capacity] */
                             uint32_t* out_chunks,                 /* [n_assets] */
                             uint64_t* out_info                    /* [4] */);

/* WHERE two assets share chunks: isccsearch_join_overlaps, and from the same join launch the chunk pairs of every pair of assets as
 * aligned runs -- "chunks 40..95 of asset A are chunks 3..58 of asset B".  Table, asset_keys, max_hamming, max_doc_freq, dup_limit and
 * capacity as for isccsearch_join_overlaps; the chunk pairs are exactly its chunk pairs (listing, stop chunk, same-asset and radius
 * rules unchanged).
 *   ORDINAL of a row: the number of rows of the table with the same first key word (the same asset) and a smaller second key word --
 *                         the row's rank within its asset by ascending (offset, size).  Every row of the table counts, a stop chunk
 *                         too: a stop chunk in the middle of a clip keeps its place and splits the run.  For a listed asset the ordinals
 *                         are 0 .. out_chunks[asset] - 1.
 *   SEGMENT: for an unordered pair of assets with labels src < dst let P be its chunk pairs as (o_src, o_dst, hamming), o the ordinals
 *                         of the pair's two rows.  A segment is a maximal set {(o_src + t, o_dst + t) : t = 0 .. length - 1} in P: a
 *                         run on one diagonal o_dst - o_src.  Every chunk pair lies in exactly one segment, so the lengths of the
 *                         segments of (src, dst) add up to the chunk_pairs of the overlap record (src, dst).
 *   out_pairs[2 * capacity], out_chunks[n_assets], out_info[0 .. 3]: byte for byte what isccsearch_join_overlaps returns for the same
 *                         arguments.
 *   out_segments[capacity]  one record per segment, sorted ascending by (src, dst, first_dst - first_src as a signed value, first_src).
 *                         Every field is an integer defined by the set of chunk pairs and the table's keys alone: which kernel ran and
 *                         the order in which pairs were found never show.
 *   out_info[5]           {chunk pairs found, records written, live rows, stop chunks, segments written}.
 * Capacity protocol as for isccsearch_join_overlaps: more than `capacity` chunk pairs return -ENOSPC with out_info[0] exact and every
 * other output unspecified, and a retry with exactly that capacity succeeds; pairs past the capacity are counted and not written.
 * Device memory: 352 bytes per chunk pair of the capacity (the 192 of isccsearch_join_overlaps; 64 for the pairs keyed by diagonal,
 * unsorted and sorted, 96 for the runs before and after their reduction), 28 bytes per row (4 as isccsearch_join_overlaps; the sorted
 * keys, 16, the sorted rows and the ordinals, 4 each) and 12 per asset, besides rocPRIM's temporary storage; kept by the handle as its
 * other scratch buffers are.
 * -EINVAL and -E2BIG as for isccsearch_join_overlaps, all checked on the host before anything is launched, the outputs left untouched;
 * out_segments may be NULL only when capacity is 0, like out_pairs.  -E2BIG also for a segment of 2^31 rows or more: the difference
 * of two ordinals travels as 32 bits.
 * One lock covers the call; everything runs on the handle's one stream -- labelling, the ONE join launch isccsearch_join_overlaps
 * makes, then ordinals (a sort of the table's keys on the device: the host never sees them), the pairs keyed and sorted by (src, dst,
 * diagonal, ordinal), run heads, a reduction per run, the byte ranges gathered from the key column, then sort and reduction of
 * isccsearch_join_overlaps -- and ONE synchronisation comes before the results are copied.  With fewer than two rows or capacity 0
 * nothing of this is launched; chunks and info are filled all the same.
 * Reference counterpart: IsccChunkMatch (schema.py:445-530) carries offset and size of a matched chunk for ONE query asset; the
 * reference has no index-wide form. */
typedef struct isccsearch_segment {
    uint32_t src, dst;              /* labels (ranks in asset_keys), src < dst; isccsearch_join_segments_between: src a rank in
                                       asset_keys_a, dst a rank in asset_keys_b */
    uint32_t first_src, first_dst;  /* ordinals of the run's first chunk pair */
    uint32_t length;                /* chunk pairs in the run */
    uint32_t sum_hamming;           /* their distances, summed */
    uint32_t begin_src, begin_dst;  /* byte offset of the first chunk on either side (key word 1 >> 32) */
    uint64_t end_src, end_dst;      /* offset + size of the LAST chunk on either side (may pass 2^32) */
} isccsearch_segment;               /* 48 bytes */
int isccsearch_join_segments(isccsearch_handle* h, uint32_t table, int32_t max_hamming,
                             uint32_t max_doc_freq, uint32_t dup_limit,
                             uint32_t n_assets, const uint64_t* asset_keys,
                             uint64_t capacity,                    /* chunk pairs */
                             isccsearch_overlap* out_pairs,        /* [2 * capacity] */
                             isccsearch_segment* out_segments,     /* [capacity] */
                             uint32_t* out_chunks,                 /* [n_assets] */
                             uint64_t* out_info                    /* [5] */);

/* The pairs of assets of TWO simprint tables of one handle that share chunks: the cross join of table_a and table_b (both HAMMING,
 * key_words 2, equal max_bytes), aggregated on the device as isccsearch_join_overlaps aggregates the self-join.  A row is a chunk; its
 * asset is the first key word.
 *   asset_keys_a[n_assets_a]  strictly ascending each: the assets that take part on either side.  There are TWO label spaces: an asset
 *   asset_keys_b[n_assets_b]  of table_a is labelled by its rank in asset_keys_a, an asset of table_b by its rank in asset_keys_b.  A row
 *                         is live if its asset is listed on its own side; a listed asset its table does not hold has no rows.
 *   max_hamming           the radius, as for isccsearch_join_overlaps.
 *   max_doc_freq          stop chunks are decided PER TABLE, from that table's own frequency column built with dup_limit, exactly as
 *   dup_limit             isccsearch_join_overlaps decides them: a live row is a stop chunk if its frequency in its own table exceeds
 *                         max_doc_freq.  max_doc_freq 0: no cut, and no column is read or built.
 *   flags                 ISCCSEARCH_OVERLAPS_SKIP_SAME_ASSET: a pair whose two rows have the same asset key (one asset held by both
 *                         tables) is not a chunk pair, as the self-join treats the chunks of one asset -- it takes no slot, is not
 *                         counted and cannot push a call over its capacity.  Without the flag it is a pair like any other
 *                         (isccsearch_join_between's rule for equal keys).  No other bit is defined.
 * A chunk pair is (row i of table_a, row j of table_b), both live, neither a stop chunk in its own table, hamming(i, j) <= max_hamming.
 *   out_pairs[2 * capacity]  one record per ORDERED pair of assets with at least one chunk pair, in both directions: `reserved` 0 means
 *                         src is a label of side A and dst a label of side B, `reserved` 1 means src is a label of side B and dst a
 *                         label of side A.  Sorted ascending by (reserved, src, dst).  matched, sum_hamming and chunk_pairs as for
 *                         isccsearch_join_overlaps; every pair of assets has exactly one record in each direction, with equal
 *                         chunk_pairs.  Every field is an integer and defined by the set of chunk pairs alone: which kernel ran, which
 *                         table was held and the order in which pairs were found never show.
 *   out_chunks_a[n_assets_a]  live rows per asset of either side, stop chunks included.
 *   out_chunks_b[n_assets_b]
 *   out_info[6]           {chunk pairs found, records written, live rows a, stop chunks a, live rows b, stop chunks b}.
 * Capacity protocol as for isccsearch_join_overlaps: more than `capacity` chunk pairs return -ENOSPC with out_info[0] exact and every
 * other output unspecified, and a retry with exactly that capacity succeeds; pairs past the capacity are counted and not written.
 * Device memory: 192 bytes per chunk pair of the capacity, 4 bytes per row of both tables and 12 per listed asset of both sides, kept
 * in the handle's scratch buffers.
 * -EINVAL, each naming the offending index or argument, all checked on the host before anything is launched, the outputs left
 * untouched: a NULL argument (out_pairs may be NULL only when capacity is 0); table_a == table_b (isccsearch_join_overlaps joins a
 * table with itself); a table that is not HAMMING with key_words 2, or tables that differ in max_bytes; n_assets_a or n_assets_b
 * outside 1 .. 2^31 - 1 (a label of side B carries one more bit inside the device's hit format); either key array not strictly
 * ascending; max_hamming < 0; max_doc_freq > dup_limit when max_doc_freq > 0; unknown flag bits.  -E2BIG, checked likewise: a segment
 * of 2^32 rows or more, a capacity of 2^31 chunk pairs or more.
 * One lock covers the call; everything runs on the handle's one stream.  The two frequency columns are built first (each build drains
 * the stream), then labelling (once per table), ONE join launch (the one isccsearch_join_between would make for the two tables: the
 * table with more rows is held), sort and reduction are queued, and ONE synchronisation comes before the records are copied.  If
 * either table has no row nothing is launched; chunks and info are filled all the same.
 * No reference counterpart (the reference has no index-wide join: it finds shared chunks one query asset at a time). */
#define ISCCSEARCH_OVERLAPS_SKIP_SAME_ASSET 1u
int isccsearch_join_overlaps_between(isccsearch_handle* h, uint32_t table_a, uint32_t table_b, int32_t max_hamming,
                                     uint32_t max_doc_freq, uint32_t dup_limit,
                                     uint32_t n_assets_a, const uint64_t* asset_keys_a,
                                     uint32_t n_assets_b, const uint64_t* asset_keys_b,
                                     uint32_t flags, uint64_t capacity,    /* chunk pairs */
                                     isccsearch_overlap* out_pairs,        /* [2 * capacity] */
                                     uint32_t* out_chunks_a,               /* [n_assets_a] */
                                     uint32_t* out_chunks_b,               /* [n_assets_b] */
                                     uint64_t* out_info                    /* [6] */);

/* WHERE the assets of two tables share chunks: isccsearch_join_overlaps_between, and from the same join launch the chunk pairs of every
 * pair (asset of table_a, asset of table_b) as aligned runs -- "chunks 40..95 of asset a of my catalogue are chunks 3..58 of asset b of
 * that registry".  Tables, the two label spaces, asset_keys_a / asset_keys_b, max_hamming, max_doc_freq, dup_limit (stop chunks per
 * table), flags (ISCCSEARCH_OVERLAPS_SKIP_SAME_ASSET) and capacity as for isccsearch_join_overlaps_between; the chunk pairs are exactly
 * its chunk pairs.
 *   ORDINAL of a row: its rank within its asset IN ITS OWN TABLE by ascending second key word (offset, size) -- the rule of
 *                         isccsearch_join_segments, applied per table.  Every row of that table counts: the rows of unlisted assets
 *                         do not matter (they are other assets), a stop chunk keeps its place and splits a run, and the rows the
 *                         OTHER table holds of the same asset key count nothing.
 *   SEGMENT: for a pair (asset a of table_a, asset b of table_b) let P be its chunk pairs as (o_a, o_b, hamming).  A segment is a maximal
 *                         set {(o_a + t, o_b + t) : t = 0 .. length - 1} in P: a run on one diagonal o_b - o_a.  Every chunk pair lies
 *                         in exactly one segment, so the lengths of the segments of (a, b) add up to the chunk_pairs of the overlap
 *                         record (`reserved` 0, a, b), which equals that of (`reserved` 1, b, a).
 *   out_pairs[2 * capacity], out_chunks_a[n_assets_a], out_chunks_b[n_assets_b], out_info[0 .. 5]: byte for byte what
 *                         isccsearch_join_overlaps_between returns for the same arguments.
 *   out_segments[capacity]  one isccsearch_segment per segment.  `src` is ALWAYS the label of the table_a asset (its rank in
 *                         asset_keys_a) and `dst` the label of the table_b asset (its rank in asset_keys_b), without any side bit: there
 *                         is no src < dst rule between the two label spaces and no second direction.  first_src, begin_src and end_src
 *                         come from table_a's ordinals and keys, the _dst fields from table_b's.  Sorted ascending by (src, dst,
 *                         first_dst - first_src as a signed value, first_src).  Every field is an integer defined by the set of chunk
 *                         pairs and the two tables' keys alone: which kernel ran, which table was held and the order in which pairs
 *                         were found never show.
 *   out_info[7]           {chunk pairs found, records written, live rows a, stop chunks a, live rows b, stop chunks b, segments
 *                         written}.
 * Capacity protocol as for isccsearch_join_overlaps_between: more than `capacity` chunk pairs return -ENOSPC with out_info[0] exact and
 * every other output unspecified, and a retry with exactly that capacity succeeds; pairs past the capacity are counted and not written.
 * Device memory: 352 bytes per chunk pair of the capacity (the 192 of isccsearch_join_overlaps_between; 64 for the pairs keyed by
 * diagonal, unsorted and sorted, 96 for the runs before and after their reduction), 28 bytes per row of BOTH tables (4 as
 * isccsearch_join_overlaps_between; the sorted keys, 16, the sorted rows and the ordinals, 4 each, the two tables' side by side in one
 * buffer each) and 12 per listed asset of both sides, besides rocPRIM's temporary storage (the largest need of any step, both tables'
 * key sorts among them); kept by the handle as its other scratch buffers are.
 * -EINVAL and -E2BIG as for isccsearch_join_overlaps_between, all checked on the host before anything is launched, the outputs left
 * untouched; out_segments may be NULL only when capacity is 0, like out_pairs.  -E2BIG also for a segment of 2^31 rows or more in
 * EITHER table: the difference of two ordinals travels as 32 bits.
 * One lock covers the call; everything runs on the handle's one stream.  The two frequency columns are built first (each build drains
 * the stream), then labelling (once per table), the ONE join launch isccsearch_join_between would make for the two tables, then the
 * stage of isccsearch_join_segments over the two tables -- ordinals (one sort of the keys per table), the pairs keyed (the hit whose
 * label lacks the side bit is table_a's, whichever table was held) and sorted, run heads, a reduction per run, the byte ranges
 * gathered from either table's key column --, then sort and reduction of isccsearch_join_overlaps_between, and ONE synchronisation
 * comes before the counters are read.  If either table has no row or capacity is 0 nothing of the stage is sized, allocated or queued;
 * chunks and info are filled all the same.
 * Reference counterpart: IsccChunkMatch (schema.py:445-530) carries offset and size of a matched chunk for ONE query asset; the
 * reference has no index-wide form. */
int isccsearch_join_segments_between(isccsearch_handle* h, uint32_t table_a, uint32_t table_b, int32_t max_hamming,
                                     uint32_t max_doc_freq, uint32_t dup_limit,
                                     uint32_t n_assets_a, const uint64_t* asset_keys_a,
                                     uint32_t n_assets_b, const uint64_t* asset_keys_b,
                                     uint32_t flags, uint64_t capacity,    /* chunk pairs */
                                     isccsearch_overlap* out_pairs,        /* [2 * capacity] */
                                     isccsearch_segment* out_segments,     /* [capacity] */
                                     uint32_t* out_chunks_a,               /* [n_assets_a] */
                                     uint32_t* out_chunks_b,               /* [n_assets_b] */
                                     uint64_t* out_info                    /* [7] */);

/* Multi-GPU building blocks (row-range shards, one process per GPU).
 * search_device: same search, results left in caller-provided DEVICE memory
 *   d_records[nq*k] (isccsearch_record), d_counts[nq]; queries must share one byte length.
 *   The call returns after the library's stream has drained, so the buffers can go straight
 *   into an RCCL all-gather on any stream.
 * merge_device: k-way merge of n_lists result sets held in DEVICE memory into host outputs shaped
 *   as for isccsearch_search.  List l has its records [nq][k] at d_records + l*list_stride and its
 *   counts [nq] at d_counts + l*count_stride (strides in bytes), so one all-gathered buffer of
 *   per-rank blocks {records | counts} can be merged in place. */
int isccsearch_search_device(isccsearch_handle* h, uint32_t table, uint32_t nq, const uint64_t* q_words,
                             const uint8_t* q_nbytes, uint32_t k, void* d_records, uint32_t* d_counts);
/* search_within_device: the range-limited search (isccsearch_search_within) with device-resident results. */
int isccsearch_search_within_device(isccsearch_handle* h, uint32_t table, uint32_t nq, const uint64_t* q_words,
                                    const uint8_t* q_nbytes, uint32_t k, uint32_t max_hamming,
                                    void* d_records, uint32_t* d_counts);
int isccsearch_merge_device(isccsearch_handle* h, uint32_t n_lists, uint32_t nq, uint32_t k, int key_words,
                            const void* d_records, const void* d_counts, uint64_t list_stride, uint64_t count_stride,
                            uint64_t* out_keys, uint32_t* out_hamming, uint16_t* out_prefix_bits, uint32_t* out_count);

/* The same two steps WITHOUT host round-trips in between (one synchronisation per multi-GPU search step instead of four):
 *   search_device_async   enqueues the search on the library's stream and makes `consumer_stream` (a hipStream_t, e.g. the
 *                         stream the all-gather is issued on) wait for it; it does not wait itself.  max_hamming < 0 = plain
 *                         top-k.  A query whose candidate list overflowed cannot take the exact fallback without the host,
 *                         so its count is written as ISCCSEARCH_COUNT_OVERFLOW; merge_kernel propagates the marker and the
 *                         caller re-runs the step through the synchronous entry points (rare; every rank sees the same
 *                         merged counts, so all ranks take the same decision).  Tables with several segments and batches
 *                         beyond 1 024 queries run the synchronous path inside the call.
 *   merge_device_after    as merge_device, ordered after everything queued on `producer_stream` (the stream the gathered
 *                         blocks were produced on); ONE device->host copy and ONE synchronisation.  out_count[q] ==
 *                         ISCCSEARCH_COUNT_OVERFLOW reports the marker. */
#define ISCCSEARCH_COUNT_OVERFLOW 0xFFFFFFFFu
/* The library's stream (a hipStream_t, owned by the handle).  A host that issues the exchange between the two calls ON this
 * stream (torch: torch.cuda.ExternalStream) and passes it as consumer_stream / producer_stream needs no event between the
 * streams: search, exchange and merge are one in-order queue (two cross-queue hand-overs, ~12 and ~21 us per step, dropped). */
void* isccsearch_stream(isccsearch_handle* h);
int isccsearch_search_device_async(isccsearch_handle* h, uint32_t table, uint32_t nq, const uint64_t* q_words,
                                   const uint8_t* q_nbytes, uint32_t k, int32_t max_hamming,
                                   void* d_records, uint32_t* d_counts, void* consumer_stream);
int isccsearch_merge_device_after(isccsearch_handle* h, uint32_t n_lists, uint32_t nq, uint32_t k, int key_words,
                                  const void* d_records, const void* d_counts, uint64_t list_stride, uint64_t count_stride,
                                  void* producer_stream,
                                  uint64_t* out_keys, uint32_t* out_hamming, uint16_t* out_prefix_bits, uint32_t* out_count);

/* Several merge_device_after calls behind ONE synchronisation (the per-unit searches of one request on a sharded index share one
 * all-gather: their merges are queued back to back and read after a single synchronisation).  Every request is shaped as the
 * arguments of isccsearch_merge_device_after; all results together must fit the directly written result block (1 MB), else -E2BIG. */
typedef struct isccsearch_merge_request {
    uint32_t n_lists, nq, k;
    int32_t key_words;
    const void* d_records;
    const void* d_counts;
    uint64_t list_stride, count_stride;
    uint64_t* out_keys;
    uint32_t* out_hamming;
    uint16_t* out_prefix_bits;
    uint32_t* out_count;
} isccsearch_merge_request;
int isccsearch_merge_many_after(isccsearch_handle* h, uint32_t n, isccsearch_merge_request* reqs, void* producer_stream);

#ifdef __cplusplus
}
#endif
#endif /* ISCCSEARCH_H */
