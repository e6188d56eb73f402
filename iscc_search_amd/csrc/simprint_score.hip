// Simprint asset scoring on the device: see simprint_score.h for the pipeline and the reference lines it restates
// (iscc_search/indexes/simprint/usearch_core.py:171-269).  Built for gfx950 only.
#include <cstring>   // rocPRIM's texture iterator calls memset without including it
#include <type_traits>

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "simprint_score.h"

namespace isksp {
namespace {

constexpr int BLOCK = 256;
constexpr uint64_t EMPTY = ~0ULL;
constexpr uint32_t COUNT_OVERFLOW = ISCCSEARCH_COUNT_OVERFLOW;

// block-wide exclusive prefix of one value per thread (4 waves); `total` = sum over the block
__device__ __forceinline__ uint32_t block_exclusive(uint32_t v, uint32_t* wtot /*[4] shared*/, uint32_t& total) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t incl = v;
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t o = __shfl_up(incl, off);
        if (lane >= (uint32_t)off) incl += o;
    }
    __syncthreads();                 // (wtot may still be read from the previous use)
    if (lane == 63) wtot[wave] = incl;
    __syncthreads();
    uint32_t before = 0;
    total = 0;
    for (uint32_t w = 0; w < 4; ++w) { if (w < wave) before += wtot[w]; total += wtot[w]; }
    return before + incl - v;
}

// adds one value per thread of the block into *total (shared, zeroed before the last barrier; complete after the next one): a
// shuffle sum per wave, then one atomic per wave that has something to add
__device__ __forceinline__ void block_add(uint32_t v, uint32_t* total) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(total, v);
}

// this thread's share of the distinct assets among the first n records of a list that ascends by key (an asset's rows are adjacent)
__device__ __forceinline__ uint32_t distinct_assets(const isccsearch_record* r, uint32_t n) {
    uint32_t mine = 0;
    for (uint32_t i = threadIdx.x; i < n; i += BLOCK) mine += (i == 0 || r[i].key_hi != r[i - 1].key_hi) ? 1u : 0u;
    return mine;
}

// ---------------------------------------------------------------------------------------------
// mark_kernel: one block per query simprint of the batch.
//   matches   = the prefix of the list with hamming <= h_max (the list ascends by (hamming, key)): the reference's threshold
//               on score = 1 - d / ndim (usearch_core.py:182-184), restated on the integer by the host
//   best      = first occurrence of an asset (key_hi) among the matches = the chunk the reference keeps for (asset, query)
//               (:191-196: the first one seen wins, a later one only with a strictly better score -- never in an ascending list)
//   freq_q    = document frequency of the query simprint itself: distinct assets among the first dup_limit rows EQUAL to it
//               = among the hamming-0 prefix of its list (ascending key, so an asset's rows are adjacent).  Undecidable only when
//               the whole list of k rows is at distance 0 and k < dup_limit: flagged, the host asks isccsearch_doc_freq.
// dynamic LDS: keys[S] u64 | idx[S] u32, S = 2^log2s >= 2 k
// ---------------------------------------------------------------------------------------------
struct MarkParams {
    const isccsearch_record* rec;   // batch base
    const uint32_t* cnt;
    uint8_t* best;                  // batch base
    uint32_t* nbest;                // batch base
    uint32_t* freq_q;               // batch base
    uint32_t* unknown;              // batch base
    uint32_t* info;
    uint32_t k;
    int h_max;
    uint32_t dup_limit, log2s;
};
__device__ __forceinline__ uint32_t slot_of(uint64_t a, uint32_t log2s) { return (uint32_t)((a * 0x9E3779B97F4A7C15ULL) >> (64 - log2s)); }

__global__ __launch_bounds__(BLOCK) void mark_kernel(const MarkParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ uint32_t s_nm, s_n0, s_ones, s_best, s_dist;
    const uint32_t S = 1u << p.log2s, mask = S - 1;
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(smem);
    uint32_t* idx = reinterpret_cast<uint32_t*>(smem + (size_t)S * 8);
    const uint32_t q = blockIdx.x, tid = threadIdx.x;
    const uint32_t c = p.cnt[q];
    const uint32_t n = c == COUNT_OVERFLOW ? 0 : (c < p.k ? c : p.k);
    const isccsearch_record* r = p.rec + (uint64_t)q * p.k;
    uint8_t* best = p.best + (uint64_t)q * p.k;
    for (uint32_t i = tid; i < S; i += BLOCK) { keys[i] = EMPTY; idx[i] = 0xFFFFFFFFu; }
    if (tid == 0) { s_nm = 0; s_n0 = 0; s_ones = 0xFFFFFFFFu; s_best = 0; s_dist = 0; }
    __syncthreads();
    for (uint32_t i = tid; i < n; i += BLOCK) {
        const int h = r[i].hamming;
        const int hn = i + 1 < n ? (int)r[i + 1].hamming : 0x10000;
        if (h <= p.h_max && hn > p.h_max) s_nm = i + 1;
        if (h == 0 && hn != 0) s_n0 = i + 1;
    }
    __syncthreads();
    const uint32_t nm = s_nm, n0 = s_n0;
    for (uint32_t i = tid; i < nm; i += BLOCK) {
        const uint64_t a = r[i].key_hi;
        if (a == EMPTY) { atomicMin(&s_ones, i); continue; }
        uint32_t s = slot_of(a, p.log2s);
        for (;;) {
            const unsigned long long old = atomicCAS(&keys[s], (unsigned long long)EMPTY, (unsigned long long)a);
            if (old == EMPTY || old == a) { atomicMin(&idx[s], i); break; }
            s = (s + 1) & mask;
        }
    }
    __syncthreads();
    uint32_t mine = 0;
    for (uint32_t i = tid; i < p.k; i += BLOCK) {
        uint8_t b = 0;
        if (i < nm) {
            const uint64_t a = r[i].key_hi;
            if (a == EMPTY) b = s_ones == i;
            else {
                uint32_t s = slot_of(a, p.log2s);
                while (keys[s] != a) s = (s + 1) & mask;
                b = idx[s] == i;
            }
        }
        best[i] = b;
        mine += b;
    }
    // the query's own document frequency
    const uint32_t m0 = p.dup_limit ? (n0 < p.dup_limit ? n0 : p.dup_limit) : 0;
    block_add(mine, &s_best);
    block_add(distinct_assets(r, m0), &s_dist);
    __syncthreads();
    if (tid == 0) {
        p.nbest[q] = s_best;
        p.freq_q[q] = p.dup_limit ? s_dist : 1u;
        const uint32_t unk = (p.dup_limit && n0 == n && n == p.k && p.k < p.dup_limit) ? 1u : 0u;
        p.unknown[q] = unk;
    }
}

// offs[q] = base + exclusive prefix of nbest over the batch (m <= 1 024: four queries per thread); info = {base + total, some
// query's frequency is unknown, 0, 0}
__global__ __launch_bounds__(BLOCK) void offsets_kernel(const uint32_t* nbest, const uint32_t* unknown, uint32_t* offs, uint32_t m, uint32_t base, uint32_t* info) {
    __shared__ uint32_t wtot[4], wunk[4];
    const uint32_t tid = threadIdx.x;
    uint32_t running = base, unk = 0;
    for (uint32_t c0 = 0; c0 < m; c0 += 4 * BLOCK) {
        uint32_t v[4], sum = 0;
        for (uint32_t j = 0; j < 4; ++j) { const uint32_t q = c0 + 4 * tid + j; v[j] = q < m ? nbest[q] : 0; sum += v[j]; unk |= q < m ? unknown[q] : 0; }
        uint32_t total;
        uint32_t at = running + block_exclusive(sum, wtot, total);
        for (uint32_t j = 0; j < 4; ++j) { const uint32_t q = c0 + 4 * tid + j; if (q < m) offs[q] = at; at += v[j]; }
        running += total;
    }
    const unsigned long long any = __ballot(unk != 0);
    if ((tid & 63) == 0) wunk[tid >> 6] = any != 0;
    __syncthreads();
    if (tid == 0) { info[0] = running; info[1] = wunk[0] | wunk[1] | wunk[2] | wunk[3]; info[2] = 0; info[3] = 0; }
}

// the best entries of query q, in rank order, to positions offs[q] ...
struct CompactParams {
    const isccsearch_record* rec;   // batch base
    const uint8_t* best;            // batch base
    const uint32_t* offs;           // batch base
    uint64_t* c_asset;
    uint32_t* c_entry;
    uint32_t k, pos;
};
__global__ __launch_bounds__(BLOCK) void compact_kernel(const CompactParams p) {
    __shared__ uint32_t wtot[4];
    const uint32_t q = blockIdx.x, tid = threadIdx.x;
    const isccsearch_record* r = p.rec + (uint64_t)q * p.k;
    const uint8_t* best = p.best + (uint64_t)q * p.k;
    uint32_t running = p.offs[q];
    for (uint32_t c0 = 0; c0 < p.k; c0 += BLOCK) {
        const uint32_t i = c0 + tid;
        const uint32_t f = i < p.k ? best[i] : 0;
        uint32_t total;
        const uint32_t at = running + block_exclusive(f, wtot, total);
        if (f) { p.c_asset[at] = r[i].key_hi; p.c_entry[at] = (p.pos + q) * p.k + i; }
        running += total;
    }
}

// ---------------------------------------------------------------------------------------------
// weights_kernel: per sorted entry, its IDF weight and weight x similarity (two roundings, as `idf * sim` then `+=` in
// usearch_core.py:224-226), and the query index; per query simprint, the IDF of its own document frequency (:232-234).
// Everything score_kernel's sequential sums need lies in contiguous arrays afterwards: no pointer chasing in the chain.
// ---------------------------------------------------------------------------------------------
struct WeightParams {
    const uint32_t* entry;          // sorted by asset
    const isccsearch_record* rec;
    const uint32_t* rows;
    const uint32_t* freq_col;
    const uint32_t* freq_q;
    const double* sim_tab;
    const double* idf_tab;
    double* w;                      // [entries]
    double* ws;                     // [entries]
    uint32_t* q;                    // [entries]
    double* idf_q;                  // [nq]
    uint32_t* n_assets;             // zeroed here for score_kernel
    uint32_t entries, nq, k, dup_limit;
};
__global__ __launch_bounds__(BLOCK) void weights_kernel(const WeightParams p) {
#pragma clang fp contract(off)
    const uint32_t t = blockIdx.x * BLOCK + threadIdx.x;
    if (t == 0) *p.n_assets = 0;
    if (t < p.entries) {
        const uint32_t ent = p.entry[t];
        uint32_t f = 0;
        if (p.dup_limit) { f = p.freq_col[p.rows[ent]]; f = f < p.dup_limit ? f : p.dup_limit; }
        const double idf = p.idf_tab[f];
        p.w[t] = idf;
        p.ws[t] = idf * p.sim_tab[p.rec[ent].hamming];
        p.q[t] = ent / p.k;
    }
    if (t < p.nq) {
        uint32_t f = 0;
        if (p.dup_limit) { f = p.freq_q[t]; f = f < p.dup_limit ? f : p.dup_limit; }
        p.idf_q[t] = p.idf_tab[f];
    }
}

// ---------------------------------------------------------------------------------------------
// score_kernel: one thread per sorted entry; the thread at the head of a run scores it.  A run is an asset's entries (ScoreParams,
// queue_score) or a (request, asset) pair's (ScoreManyParams, queue_score_many: entries sorted by request, then asset).
//   usearch_core.py:215-236 -- total_idf and weighted_sim over the matched query simprints in ascending query order (the
//   insertion order of best_per_query), then total_idf over every unmatched query simprint in ascending order; score =
//   weighted / total when total > 0.  Sequential float64 operations with IEEE rounding, none contracted.
//   The run is walked eight entries at a time (its loads do not depend on the sums), and leaves a bit per matched query in the
//   thread's LDS row, so that the second sum runs over the query simprints without touching memory it has to wait for.
//   With many requests the unmatched sum runs over the run's own request [qbeg[r], qbeg[r + 1]) only, and the LDS row holds the
//   64-bit words that range touches, relative to its first word.
// dynamic LDS: mask[words][threads] u64 (ScoreParams: words = ceil(nq / 64))
// ---------------------------------------------------------------------------------------------
struct ScoreParams {
    const uint64_t* asset;          // sorted
    const double* w;
    const double* ws;
    const uint32_t* q;
    const double* idf_q;
    double* score;
    uint32_t* order;
    uint32_t* matches;
    uint32_t* n_assets;
    uint32_t entries, nq, words;
};
struct ScoreManyParams {
    const uint64_t* asset;          // sorted by (request, asset)
    const uint32_t* req;            // sorted
    const double* w;
    const double* ws;
    const uint32_t* q;
    const double* idf_q;
    const uint32_t* qbeg;
    double* score;
    uint32_t* order;
    uint32_t* matches;
    uint32_t* n_assets;             // [n_req]
    uint32_t entries, nq, words;
};
template <class P>
__global__ void score_kernel(const P p) {
    // HIP's __dadd_rn / __dmul_rn are plain `+` / `*`, and device code is compiled with -ffp-contract=fast: without this pragma
    // (and the file's -ffp-contract=off) `weighted + idf * sim` becomes ONE fused multiply-add -- a single rounding where the
    // reference's Python does two (found by tests/test_gpu_simprint_score.py: scores one ulp off)
#pragma clang fp contract(off)
    constexpr bool MANY = std::is_same<P, ScoreManyParams>::value;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned long long* mask = reinterpret_cast<unsigned long long*>(smem);
    const uint32_t T = blockDim.x, tid = threadIdx.x, lane = tid & 63;
    const uint32_t e = blockIdx.x * T + tid;
    const uint64_t a = e < p.entries ? p.asset[e] : 0;
    uint32_t r = 0;
    bool head;
    if constexpr (MANY) {
        r = e < p.entries ? p.req[e] : 0;
        head = e < p.entries && (e == 0 || p.asset[e - 1] != a || p.req[e - 1] != r);
    } else {
        head = e < p.entries && (e == 0 || p.asset[e - 1] != a);
    }
    double total = 0.0, weighted = 0.0;
    uint32_t end = e, qb = 0, qe = 0, wb = 0, we = 0;
    if (e < p.entries) p.order[e] = e;
    if (head) {
        // 1. the matched query simprints, ascending (the run is sorted by asset, stably: by query inside an asset)
        uint32_t words = p.words;
        if constexpr (MANY) {
            qb = p.qbeg[r]; qe = p.qbeg[r + 1];                   // (qe > qb: the request has entries)
            wb = qb >> 6; we = ((qe - 1) >> 6) + 1;
            words = we - wb;
        }
        for (uint32_t w = 0; w < words; ++w) mask[w * T + tid] = 0;
        constexpr int U = 8;
        uint32_t j = e;
        for (bool more = true; more;) {
            uint64_t aa[U]; double ww[U], ss[U]; uint32_t qq[U], rr[U];
            for (int u = 0; u < U; ++u) {
                const uint32_t jj = j + u < p.entries ? j + u : p.entries - 1;
                aa[u] = p.asset[jj]; if constexpr (MANY) rr[u] = p.req[jj]; ww[u] = p.w[jj]; ss[u] = p.ws[jj]; qq[u] = p.q[jj];
            }
            int u = 0;
            for (; u < U; ++u) {
                if (j + u >= p.entries || aa[u] != a || (MANY && rr[u] != r)) { more = false; break; }
                total = total + ww[u];
                weighted = weighted + ss[u];
                mask[((qq[u] >> 6) - wb) * T + tid] |= 1ull << (qq[u] & 63);
            }
            j += u;
        }
        end = j;
    }
    // 2. every unmatched query simprint, ascending.  The whole wave walks the queries together -- lane l holds the IDF of query
    //    64 w + l, each step broadcasts one of them from a register (v_readlane) -- so nothing in a head's chain of additions waits
    //    for memory; lanes that head no run tag along.  With many requests the wave walks the union of its heads' ranges, and a
    //    lane skips the query simprints outside its own range like matched ones.
    if (__ballot(head)) {
        uint32_t lo = 0, hi = p.words;
        if constexpr (MANY) {
            lo = head ? wb : 0xFFFFFFFFu; hi = head ? we : 0;
            for (int off = 32; off > 0; off >>= 1) {
                const uint32_t l2 = __shfl_xor(lo, off), h2 = __shfl_xor(hi, off);
                lo = l2 < lo ? l2 : lo;
                hi = h2 > hi ? h2 : hi;
            }
        }
        for (uint32_t w = lo; w < hi; ++w) {
            const uint32_t q0 = 64 * w, n = p.nq - q0 < 64 ? p.nq - q0 : 64;
            unsigned long long m;
            if constexpr (MANY) {
                m = ~0ULL;
                if (head && w >= wb && w < we) {
                    m = mask[(w - wb) * T + tid];
                    if (q0 < qb) m |= (1ull << (qb - q0)) - 1;     // before the request (w == wb: qb - q0 < 64)
                    if (qe - q0 < 64) m |= ~0ULL << (qe - q0);      // behind it (qe > q0 here)
                }
            } else {
                // (bits of queries beyond nq are set: skipped like matched ones, so that the loop below has a fixed trip count)
                m = (head ? mask[w * T + tid] : ~0ULL) | (n < 64 ? ~0ULL << n : 0ULL);
            }
            const double mine = lane < n ? p.idf_q[q0 + lane] : 0.0;
            const int lo_w = __double2loint(mine), hi_w = __double2hiint(mine);
#pragma unroll
            for (uint32_t i = 0; i < 64; ++i) {
                const double x = __hiloint2double(__builtin_amdgcn_readlane(hi_w, i), __builtin_amdgcn_readlane(lo_w, i));
                total = (m >> i) & 1 ? total : total + x;
            }
        }
    }
    if (e < p.entries) {
        p.score[e] = !head ? -1.0 : (total > 0.0 ? weighted / total : 0.0);       // (f64 division: correctly rounded by default)
        p.matches[e] = end - e;
    }
    if constexpr (MANY) {
        if (head) atomicAdd(&p.n_assets[r], 1u);
    } else {
        const unsigned long long heads = __ballot(head);
        if (lane == 0 && heads) atomicAdd(p.n_assets, (uint32_t)__popcll(heads));
    }
}

// ---------------------------------------------------------------------------------------------
// The chunk record of a matched entry (emit_kernel, emit_many_kernel): the query simprint it matched, counted from q0 (the first
// query simprint of its request), the stored chunk's key, distance, document frequency and code words, at position `at` of the
// pinned chunk arrays.
// ---------------------------------------------------------------------------------------------
struct ChunkParams {
    const isccsearch_record* rec;
    const uint32_t* rows;
    const uint32_t* freq_col;
    const uint64_t* col[4];
    isccsearch_simprint_chunk* out_chunks;      // nullptr: no chunks wanted
    uint64_t* out_chunk_words;
    uint32_t k, W, dup_limit;
};
__device__ __forceinline__ void write_chunk(const ChunkParams& p, uint32_t ent, uint32_t q0, uint32_t at) {
    const isccsearch_record& rec = p.rec[ent];
    const uint32_t row = p.rows[ent];
    isccsearch_simprint_chunk c;
    c.query = ent / p.k - q0;
    c.reserved = 0;
    c.key_lo = rec.key_lo;
    c.hamming = rec.hamming;
    c.freq = p.dup_limit ? p.freq_col[row] : 1u;
    p.out_chunks[at] = c;
    for (uint32_t w = 0; w < p.W; ++w) p.out_chunk_words[(uint64_t)at * p.W + w] = p.col[w][row];
}
// ... and of a collision (queue_exact, queue_exact_many): an entry is (given simprint g) * k + rank, its record belongs to distinct
// lookup d_of_g[g]; stored simprint == query simprint, score 1.0 (lmdb_ops.py:228-235), so no code words.  `query` counts from g0,
// the first given simprint of the entry's request
__device__ __forceinline__ void write_collision(const ChunkParams& p, const uint32_t* d_of_g, const uint32_t* freq_d, uint32_t ent, uint32_t g0, uint32_t at) {
    isccsearch_simprint_chunk c;
    const uint32_t g = ent / p.k;
    c.query = g - g0;
    c.reserved = 0;
    const uint32_t d = d_of_g[g];
    c.key_lo = p.rec[(uint64_t)d * p.k + ent % p.k].key_lo;
    c.hamming = 0;
    c.freq = freq_d[d];
    p.out_chunks[at] = c;
}

// ---------------------------------------------------------------------------------------------
// emit_kernel: block r writes result r of the first min(limit, assets) runs in (-score, asset) order -- and its matched
// chunks -- into pinned host memory; its chunks start behind those of the results before it.
// ---------------------------------------------------------------------------------------------
struct EmitParams {
    const double* score;            // sorted descending
    const uint32_t* order;          // run head of every sorted position
    const uint64_t* asset;
    const uint32_t* entry;
    const uint32_t* matches;
    const uint32_t* n_assets;
    ChunkParams c;
    isccsearch_simprint_result* out_results;
    uint32_t* out_info;
    uint32_t limit;
    // hard-boundary requests (queue_exact): the chunks are collisions
    const uint32_t* d_of_g;         // nullptr: the approximate path
    const uint32_t* freq_d;         // document frequency per distinct lookup
};
__global__ __launch_bounds__(BLOCK) void emit_kernel(const EmitParams p) {
    __shared__ uint32_t s_first;
    const uint32_t tid = threadIdx.x, r = blockIdx.x;
    const uint32_t assets = *p.n_assets;
    const uint32_t n = assets < p.limit ? assets : p.limit;
    if (r == 0 && tid == 0) { p.out_info[0] = n; p.out_info[1] = assets; p.out_info[2] = 0; if (n == 0) p.out_info[3] = 0; }
    if (r >= n) return;
    if (tid == 0) s_first = 0;
    __syncthreads();
    // chunks of the results before this one (block n - 1 also adds its own: the total)
    uint32_t before = 0;
    for (uint32_t i = tid; i < r; i += BLOCK) before += p.matches[p.order[i]];
    block_add(before, &s_first);
    __syncthreads();
    const uint32_t at = s_first, e = p.order[r], m = p.matches[e];
    if (tid == 0) {
        isccsearch_simprint_result res;
        res.asset = p.asset[e];
        res.score = p.score[r];
        res.matches = m;
        res.first_chunk = at;
        p.out_results[r] = res;
        if (r == n - 1) p.out_info[3] = p.c.out_chunks ? at + m : 0;
    }
    if (!p.c.out_chunks) return;
    for (uint32_t j = tid; j < m; j += BLOCK) {
        const uint32_t ent = p.entry[e + j];
        if (p.d_of_g) write_collision(p.c, p.d_of_g, p.freq_d, ent, 0, at + j);
        else write_chunk(p.c, ent, 0, at + j);
    }
}

// =====================================================================================================================
// Hard-boundary requests: search_simprints_exact (iscc_search/indexes/simprint/lmdb_ops.py:169-301) on the device.
// Input: the collision lists of the DISTINCT query simprints (records [nd][k] of a range-limited search at distance 0: every row
// equal to the query, ascending key = the order LMDB iterates the duplicates of a simprint key, k = dup_limit) and, for every query
// simprint AS GIVEN (repeats included, :197), the distinct lookup it maps to.
//   exact_freq_kernel     document frequency of every looked-up simprint: distinct assets in its list (:213-215)
//   exact_count_kernel    hits of every given simprint = length of its lookup's list -> offsets (offsets_kernel)
//   exact_compact_kernel  entries (asset, g * k + rank) in visiting order (given simprint, then key)
//   [stable sort by asset]
//   exact_weights_kernel  per sorted entry: its lookup d and that lookup's frequency, contiguous
//   exact_score_kernel    per asset (thread at the head of its run): coverage x quality (:252-301) -- distinct matched query
//                         simprints in first-seen order (a bit per lookup in the thread's LDS row), min / max frequency, then the
//                         min-max normalised inverse frequencies summed in that order; score < threshold: dropped (:222-223)
// =====================================================================================================================
__global__ __launch_bounds__(BLOCK) void exact_freq_kernel(const isccsearch_record* rec, const uint32_t* cnt, uint32_t* freq_d, uint32_t k) {
    __shared__ uint32_t total;
    const uint32_t d = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) total = 0;
    __syncthreads();
    const uint32_t n = cnt[d] < k ? cnt[d] : k;
    block_add(distinct_assets(rec + (uint64_t)d * k, n), &total);
    __syncthreads();
    if (tid == 0) freq_d[d] = total;
}

__global__ __launch_bounds__(BLOCK) void exact_count_kernel(const uint32_t* cnt, const uint32_t* d_of_g, uint32_t* hits, uint32_t* zero, uint32_t ng, uint32_t k) {
    const uint32_t g = blockIdx.x * BLOCK + threadIdx.x;
    if (g < ng) {
        const uint32_t c = cnt[d_of_g[g]];
        hits[g] = c < k ? c : k;
        zero[g] = 0;                      // (offsets_kernel's "unknown" input: nothing is unknown here)
    }
}

struct ExactCompactParams {
    const isccsearch_record* rec;
    const uint32_t* d_of_g;
    const uint32_t* hits;
    const uint32_t* offs;
    uint64_t* c_asset;
    uint32_t* c_entry;
    uint32_t k;
};
__global__ __launch_bounds__(BLOCK) void exact_compact_kernel(const ExactCompactParams p) {
    const uint32_t g = blockIdx.x, n = p.hits[g], at = p.offs[g];
    const isccsearch_record* r = p.rec + (uint64_t)p.d_of_g[g] * p.k;
    for (uint32_t i = threadIdx.x; i < n; i += BLOCK) { p.c_asset[at + i] = r[i].key_hi; p.c_entry[at + i] = g * p.k + i; }
}

__global__ __launch_bounds__(BLOCK) void exact_weights_kernel(const uint32_t* entry, const uint32_t* d_of_g, const uint32_t* freq_d, uint32_t* e_d, uint32_t* e_f,
                                                              uint32_t* n_assets, uint32_t entries, uint32_t k) {
    const uint32_t t = blockIdx.x * BLOCK + threadIdx.x;
    if (t == 0) *n_assets = 0;
    if (t < entries) {
        const uint32_t d = d_of_g[entry[t] / k];
        e_d[t] = d;
        e_f[t] = freq_d[d];
    }
}

struct ExactScoreParams {
    const uint64_t* asset;          // sorted
    const uint32_t* e_d;
    const uint32_t* e_f;
    double* score;
    uint32_t* order;
    uint32_t* matches;
    uint32_t* n_assets;
    uint32_t entries, words, queried;
    double threshold;
};
// ... of a round of several requests (queue_exact_many): a run is a (request, asset) pair, the bit of lookup d in the thread's LDS row
// is d - dbeg[request] (the row holds the words of the run's own request only), coverage is over the request's own `queried`, and the
// kept assets are counted per request
struct ExactScoreManyParams {
    const uint64_t* asset;          // sorted by (request, asset)
    const uint32_t* req;            // sorted
    const uint32_t* e_d;
    const uint32_t* e_f;
    const uint32_t* dbeg;           // [n_req + 1] first distinct lookup of every request in the round
    const uint32_t* queried;        // [n_req]
    double* score;
    uint32_t* order;
    uint32_t* matches;
    uint32_t* n_assets;             // [n_req]
    uint32_t entries, words;        // words: the most LDS words one request's lookups take
    double threshold;
};
template <class P>
__global__ void exact_score_kernel(const P p) {
#pragma clang fp contract(off)
    constexpr bool MANY = std::is_same<P, ExactScoreManyParams>::value;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned long long* mask = reinterpret_cast<unsigned long long*>(smem);
    const uint32_t T = blockDim.x, tid = threadIdx.x;
    const uint32_t e = blockIdx.x * T + tid;
    bool counted = false;
    uint32_t r = 0;
    if (e < p.entries) {
        const uint64_t a = p.asset[e];
        bool head;
        if constexpr (MANY) {
            r = p.req[e];
            head = e == 0 || p.asset[e - 1] != a || p.req[e - 1] != r;
        } else {
            head = e == 0 || p.asset[e - 1] != a;
        }
        p.order[e] = e;
        double score = -1.0;
        uint32_t len = 0;
        if (head) {
            // query_to_best_freq (:277-283): one entry per distinct matched query simprint, in first-seen order; the frequency of a
            // collision's stored simprint is that of the query simprint itself, so "best" is that one value
            uint32_t words = p.words, d0 = 0, queried;
            if constexpr (MANY) {
                d0 = p.dbeg[r];
                words = (p.dbeg[r + 1] - d0 + 63) >> 6;               // (<= p.words: the launch's LDS row)
                queried = p.queried[r];
            } else {
                queried = p.queried;
            }
            for (uint32_t w = 0; w < words; ++w) mask[w * T + tid] = 0;
            uint32_t distinct = 0, fmin = 0xFFFFFFFFu, fmax = 0;
            uint32_t j = e;
            for (; j < p.entries && p.asset[j] == a; ++j) {
                if constexpr (MANY) { if (p.req[j] != r) break; }
                const uint32_t d = p.e_d[j] - d0, f = p.e_f[j];
                const unsigned long long bit = 1ull << (d & 63);
                unsigned long long& word = mask[(d >> 6) * T + tid];
                if (!(word & bit)) {
                    word |= bit;
                    distinct += 1;
                    fmin = f < fmin ? f : fmin;
                    fmax = f > fmax ? f : fmax;
                }
            }
            len = j - e;
            double quality = 1.0;
            if (distinct > 1 && fmin != fmax) {                       // (:291-299)
                const double min_inv = 1.0 / (double)fmax, max_inv = 1.0 / (double)fmin;
                const double span = max_inv - min_inv;
                for (uint32_t w = 0; w < words; ++w) mask[w * T + tid] = 0;
                double sum = 0.0;
                for (uint32_t i = e; i < j; ++i) {
                    const uint32_t d = p.e_d[i] - d0;
                    const unsigned long long bit = 1ull << (d & 63);
                    unsigned long long& word = mask[(d >> 6) * T + tid];
                    if (!(word & bit)) {
                        word |= bit;
                        const double inv = 1.0 / (double)p.e_f[i];
                        const double term = (inv - min_inv) / span;
                        sum = sum + term;
                    }
                }
                quality = sum / (double)distinct;
            }
            const double coverage = (double)distinct / (double)queried;
            score = coverage * quality;
            if (score < p.threshold) score = -1.0;                    // (:222-223) dropped: sorts behind every kept asset
            else counted = true;
        }
        p.score[e] = score;
        p.matches[e] = len;
    }
    if constexpr (MANY) {
        if (counted) atomicAdd(&p.n_assets[r], 1u);
    } else {
        const unsigned long long kept = __ballot(counted);
        if ((tid & 63) == 0 && kept) atomicAdd(p.n_assets, (uint32_t)__popcll(kept));
    }
}

// =====================================================================================================================
// Many requests per call (queue_score_many; see simprint_score.h).  A run is a (request, asset) pair; everything a single
// request computes is computed per request, in the same float64 operations and the same order.
// =====================================================================================================================
// last r in [0, n) with starts[r] <= v (starts ascending, starts[0] == 0 <= v)
__device__ __forceinline__ uint32_t segment_of(const uint32_t* starts, uint32_t n, uint32_t v) {
    uint32_t lo = 0, hi = n;          // starts[lo] <= v < starts[hi] (starts[n] taken as +inf)
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (starts[mid] <= v) lo = mid; else hi = mid;
    }
    return lo;
}

// after the sort by asset: per entry its request (from the query simprint it belongs to) and its position
__global__ __launch_bounds__(BLOCK) void req_key_kernel(const uint32_t* entry, const uint32_t* qbeg, uint32_t n_req, uint32_t k,
                                                        uint32_t* req, uint32_t* idx, uint32_t entries) {
    const uint32_t t = blockIdx.x * BLOCK + threadIdx.x;
    if (t < entries) { req[t] = segment_of(qbeg, n_req, entry[t] / k); idx[t] = t; }
}

// the entries in (request, asset) order
__global__ __launch_bounds__(BLOCK) void gather_kernel(const uint32_t* idx, const uint64_t* asset_in, const uint32_t* entry_in,
                                                       uint64_t* asset_out, uint32_t* entry_out, uint32_t entries) {
    const uint32_t t = blockIdx.x * BLOCK + threadIdx.x;
    if (t < entries) { const uint32_t i = idx[t]; asset_out[t] = asset_in[i]; entry_out[t] = entry_in[i]; }
}

// after the sort by score: the request of every run head as the key of the regrouping sort (n_req behind every head: the
// non-heads, score -1, stay at the end)
__global__ __launch_bounds__(BLOCK) void head_key_kernel(const double* score, const uint32_t* order, const uint32_t* req, uint32_t n_req,
                                                         uint32_t* key, uint32_t* idx, uint32_t entries) {
    const uint32_t t = blockIdx.x * BLOCK + threadIdx.x;
    if (t < entries) { const uint32_t e = order[t]; key[t] = score[t] >= 0.0 ? req[e] : n_req; idx[t] = e; }
}

// one block: a_start = exclusive prefix of the assets per request, e_start = of the results written per request; out_info
__global__ __launch_bounds__(BLOCK) void req_scan_kernel(const uint32_t* n_assets, uint32_t n_req, uint32_t limit, uint32_t* a_start, uint32_t* e_start, uint32_t* out_info) {
    __shared__ uint32_t wtot[4];
    const uint32_t tid = threadIdx.x;
    uint32_t ra = 0, re = 0;
    for (uint32_t c0 = 0; c0 < n_req; c0 += BLOCK) {
        const uint32_t r = c0 + tid;
        const uint32_t na = r < n_req ? n_assets[r] : 0, n = na < limit ? na : limit;
        uint32_t ta, te;
        const uint32_t pa = ra + block_exclusive(na, wtot, ta);
        const uint32_t pe = re + block_exclusive(n, wtot, te);
        if (r < n_req) {
            a_start[r] = pa; e_start[r] = pe;
            out_info[4 * r] = n; out_info[4 * r + 1] = na; out_info[4 * r + 2] = 0; out_info[4 * r + 3] = 0;
        }
        ra += ta; re += te;
    }
    if (tid == 0) { a_start[n_req] = ra; e_start[n_req] = re; }
}

// chunks of written result t (0 past the last one)
__global__ __launch_bounds__(BLOCK) void result_chunks_kernel(const uint32_t* e_start, const uint32_t* a_start, const uint32_t* idx, const uint32_t* matches,
                                                              uint32_t n_req, uint32_t* cnt, uint32_t cap) {
    const uint32_t t = blockIdx.x * BLOCK + threadIdx.x;
    if (t >= cap) return;
    uint32_t m = 0;
    if (t < e_start[n_req]) {
        const uint32_t r = segment_of(e_start, n_req, t);
        m = matches[idx[a_start[r] + t - e_start[r]]];
    }
    cnt[t] = m;
}

// one wave per written result (grid-stride): result t = rank t - e_start[r] of request r, its chunks behind those of the results
// before it (first_chunk relative to the request's first chunk)
struct EmitManyParams {
    const double* score;            // per run head
    const uint32_t* idx;            // run head of every sorted position
    const uint64_t* asset;
    const uint32_t* entry;
    const uint32_t* matches;
    const uint32_t* a_start;
    const uint32_t* e_start;
    const uint32_t* c_pos;
    const uint32_t* qbeg;
    ChunkParams c;
    isccsearch_simprint_result* out_results;
    uint32_t* out_info;
    uint32_t n_req;
};
// ... of hard-boundary requests (queue_exact_many): the chunks are collisions; m.qbeg = the first GIVEN simprint of every request
struct EmitExactManyParams {
    EmitManyParams m;
    const uint32_t* d_of_g;         // distinct lookup of every given simprint, round-global
    const uint32_t* freq_d;         // document frequency per distinct lookup
};
template <class P>
__global__ __launch_bounds__(BLOCK) void emit_many_kernel(const P pp) {
    constexpr bool EXACT = std::is_same<P, EmitExactManyParams>::value;
    const EmitManyParams& p = [&]() -> const EmitManyParams& { if constexpr (EXACT) return pp.m; else return pp; }();
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t waves = gridDim.x * (BLOCK / 64);
    const uint32_t total = p.e_start[p.n_req];
    for (uint32_t t = (blockIdx.x * BLOCK + threadIdx.x) / 64; t < total; t += waves) {
        const uint32_t r = segment_of(p.e_start, p.n_req, t);
        const uint32_t first = p.e_start[r], j = t - first, n = p.e_start[r + 1] - first;
        const uint32_t e = p.idx[p.a_start[r] + j], m = p.matches[e];
        const uint32_t at = p.c_pos[t], rel = at - p.c_pos[first];
        if (lane == 0) {
            isccsearch_simprint_result res;
            res.asset = p.asset[e];
            res.score = p.score[e];
            res.matches = m;
            res.first_chunk = rel;
            p.out_results[t] = res;
            if (j == n - 1) p.out_info[4 * r + 3] = p.c.out_chunks ? rel + m : 0;
        }
        if (!p.c.out_chunks) continue;
        const uint32_t q0 = p.qbeg[r];
        for (uint32_t jj = lane; jj < m; jj += 64) {
            if constexpr (EXACT) write_collision(p.c, pp.d_of_g, pp.freq_d, p.entry[e + jj], q0, at + jj);
            else write_chunk(p.c, p.entry[e + jj], q0, at + jj);
        }
    }
}

uint32_t log2_slots(uint32_t k) {   // hash slots of mark_kernel: the power of two >= 2 k (>= 64)
    uint32_t l = 6;
    while ((1u << l) < 2 * k) ++l;
    return l;
}

}  // namespace

size_t sort_temp_bytes(size_t entries) {
    size_t a = 0, b = 0;
    uint64_t* k64 = nullptr;
    double* kd = nullptr;
    uint32_t* v = nullptr;
    (void)rocprim::radix_sort_pairs(nullptr, a, k64, k64, v, v, entries, 0, 64, (hipStream_t) nullptr);
    (void)rocprim::radix_sort_pairs_desc(nullptr, b, kd, kd, v, v, entries, 0, 64, (hipStream_t) nullptr);
    return a > b ? a : b;
}

hipError_t queue_batch(const Buffers& b, const BatchArgs& a, hipStream_t stream) {
    static bool attr_set = false;
    if (!attr_set) {
        // k = 4 096: 8 192 slots x 12 bytes
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&mark_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
        if (e != hipSuccess) return e;
        attr_set = true;
    }
    const size_t off = (size_t)a.pos * a.k;
    MarkParams mp{b.rec + off, a.cnt, b.best + off, b.nbest + a.pos, b.freq_q + a.pos, b.unknown + a.pos, a.info, a.k, a.h_max, a.dup_limit, log2_slots(a.k)};
    const size_t lds = ((size_t)1 << mp.log2s) * 12;
    hipLaunchKernelGGL(mark_kernel, dim3(a.m), dim3(BLOCK), lds, stream, mp);
    hipLaunchKernelGGL(offsets_kernel, dim3(1), dim3(BLOCK), 0, stream, b.nbest + a.pos, b.unknown + a.pos, b.offs + a.pos, a.m, a.base, a.info);
    CompactParams cp{b.rec + off, b.best + off, b.offs + a.pos, b.c_asset[0], b.c_entry[0], a.k, a.pos};
    hipLaunchKernelGGL(compact_kernel, dim3(a.m), dim3(BLOCK), 0, stream, cp);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// The stages the four pipelines share (simprint_score.h lists them); each queue_* below is the list of what differs.
// ---------------------------------------------------------------------------------------------
namespace {
constexpr uint32_t MAX_WORDS = MAX_QUERY_SIMPRINTS / 64;   // LDS words per thread a score kernel is launched with at most

// stable by asset: (c_asset, c_entry)[0] -> [1]
hipError_t sort_by_asset(const Buffers& b, uint32_t entries, hipStream_t stream) {
    size_t bytes = b.temp_bytes;
    return rocprim::radix_sort_pairs(b.temp, bytes, b.c_asset[0], b.c_asset[1], b.c_entry[0], b.c_entry[1], entries, 0, 64, stream);
}
// stable by score, descending: (score, order)[0] -> [1].  Until it runs its outputs are free: the weights (score[1]) and query
// indices (order[1]) of the approximate pipelines, the lookup index (order[1]) and frequency (score[1]) per entry of the exact one
// live there meanwhile
hipError_t sort_by_score(const Buffers& b, uint32_t entries, hipStream_t stream) {
    size_t bytes = b.temp_bytes;
    return rocprim::radix_sort_pairs_desc(b.temp, bytes, b.score[0], b.score[1], b.order[0], b.order[1], entries, 0, 64, stream);
}
// weights_kernel over the entries in `entry`'s order
void queue_weights(const Buffers& b, const ScoreArgs& a, const uint32_t* entry, hipStream_t stream) {
    const WeightParams wp{entry, b.rec, b.rows, a.freq_col, b.freq_q, a.sim_tab, a.idf_tab, b.score[1], b.ws, b.order[1], b.idf_q,
                          b.n_assets, a.entries, a.nq, a.k, a.dup_limit};
    const uint32_t wn = a.entries > a.nq ? a.entries : a.nq;
    hipLaunchKernelGGL(weights_kernel, dim3((wn + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, stream, wp);
}
// a score kernel, one thread per sorted entry with one LDS row of `words` u64 per thread: as many threads as keep a block <= 64 KB
template <class P>
void queue_scoring(void (*kernel)(P), const P& p, uint32_t entries, uint32_t words, hipStream_t stream) {
    const uint32_t T = words <= 32 ? 256 : (words <= 64 ? 128 : 64);
    hipLaunchKernelGGL(kernel, dim3((entries + T - 1) / T), dim3(T), (size_t)words * T * 8, stream, p);
}
// what the chunk records of the approximate pipelines are made of
ChunkParams chunk_params(const Buffers& b, const ScoreArgs& a) {
    ChunkParams c{b.rec, b.rows, a.freq_col, {}, a.out_chunks, a.out_chunk_words, a.k, a.W, a.dup_limit};
    for (uint32_t w = 0; w < 4; ++w) c.col[w] = a.col[w];
    return c;
}
// emit_kernel: a block per result that can exist
void queue_emit(const EmitParams& ep, uint32_t entries, hipStream_t stream) {
    hipLaunchKernelGGL(emit_kernel, dim3(ep.limit < entries ? ep.limit : entries), dim3(BLOCK), 0, stream, ep);
}
}  // namespace

// (every queue_* refuses more LDS words than a score kernel can have before it launches anything.  The entry points bound a
//  request at MAX_QUERY_SIMPRINTS query simprints, so no call reaches these refusals today.)
hipError_t queue_exact(Buffers& b, const ExactArgs& a, hipStream_t stream) {
    hipError_t e;
    const uint32_t words = (a.nd + 63) / 64;
    if (words > MAX_WORDS) return hipErrorInvalidValue;
    // (the caller has run exact_prepare: hits / offsets / entries are in place and `entries` is known)
    ExactCompactParams cp{b.rec, a.d_of_g, b.nbest, b.offs, b.c_asset[0], b.c_entry[0], a.k};
    hipLaunchKernelGGL(exact_compact_kernel, dim3(a.ng), dim3(BLOCK), 0, stream, cp);
    if ((e = sort_by_asset(b, a.entries, stream)) != hipSuccess) return e;
    uint32_t* const e_d = b.order[1];
    uint32_t* const e_f = reinterpret_cast<uint32_t*>(b.score[1]);
    hipLaunchKernelGGL(exact_weights_kernel, dim3((a.entries + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, stream, b.c_entry[1], a.d_of_g, b.freq_q, e_d, e_f, b.n_assets, a.entries, a.k);
    const ExactScoreParams sp{b.c_asset[1], e_d, e_f, b.score[0], b.order[0], b.matches, b.n_assets, a.entries, words, a.queried, a.threshold};
    queue_scoring(exact_score_kernel<ExactScoreParams>, sp, a.entries, words, stream);
    if ((e = sort_by_score(b, a.entries, stream)) != hipSuccess) return e;
    const ChunkParams collisions{b.rec, nullptr, nullptr, {}, a.out_chunks, nullptr, a.k, 0, 0};
    queue_emit(EmitParams{b.score[1], b.order[1], b.c_asset[1], b.c_entry[1], b.matches, b.n_assets, collisions, a.out_results, a.out_info, a.limit, a.d_of_g, b.freq_q},
               a.entries, stream);
    return hipGetLastError();
}

// document frequencies of the lookups, hits per given simprint and their offsets; info[0] = entries (travels to the host)
hipError_t exact_prepare(const Buffers& b, const uint32_t* cnt, const uint32_t* d_of_g, uint32_t nd, uint32_t ng, uint32_t k, uint32_t* info, hipStream_t stream) {
    hipLaunchKernelGGL(exact_freq_kernel, dim3(nd), dim3(BLOCK), 0, stream, b.rec, cnt, b.freq_q, k);
    hipLaunchKernelGGL(exact_count_kernel, dim3((ng + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, stream, cnt, d_of_g, b.nbest, b.unknown, ng, k);
    hipLaunchKernelGGL(offsets_kernel, dim3(1), dim3(BLOCK), 0, stream, b.nbest, b.unknown, b.offs, ng, 0u, info);
    return hipGetLastError();
}

hipError_t queue_score(Buffers& b, const ScoreArgs& a, hipStream_t stream) {
    hipError_t e;
    const uint32_t words = (a.nq + 63) / 64;
    if (words > MAX_WORDS) return hipErrorInvalidValue;
    if ((e = sort_by_asset(b, a.entries, stream)) != hipSuccess) return e;
    queue_weights(b, a, b.c_entry[1], stream);
    const ScoreParams sp{b.c_asset[1], b.score[1], b.ws, b.order[1], b.idf_q, b.score[0], b.order[0], b.matches, b.n_assets, a.entries, a.nq, words};
    queue_scoring(score_kernel<ScoreParams>, sp, a.entries, words, stream);
    if ((e = sort_by_score(b, a.entries, stream)) != hipSuccess) return e;
    queue_emit(EmitParams{b.score[1], b.order[1], b.c_asset[1], b.c_entry[1], b.matches, b.n_assets, chunk_params(b, a), a.out_results, a.out_info, a.limit, nullptr, nullptr},
               a.entries, stream);
    return hipGetLastError();
}

size_t many_temp_bytes(size_t entries, size_t cap) {
    size_t a = sort_temp_bytes(entries), b = 0, c = 0;
    uint32_t* v = nullptr;
    (void)rocprim::radix_sort_pairs(nullptr, b, v, v, v, v, entries, 0, 32, (hipStream_t) nullptr);
    (void)rocprim::exclusive_scan(nullptr, c, v, v, 0u, cap, rocprim::plus<uint32_t>(), (hipStream_t) nullptr);
    return std::max(a, std::max(b, c));
}

hipError_t queue_score_many(Buffers& b, const ManyBuffers& mb, const ScoreManyArgs& ma, hipStream_t stream) {
    const ScoreArgs& a = ma.s;
    hipError_t e;
    const uint32_t nr = ma.n_req, grid = (a.entries + BLOCK - 1) / BLOCK;
    uint32_t req_bits = 1;                                   // request keys 0 .. n_req (n_req: the non-heads of the regrouping sort)
    while ((1u << req_bits) <= nr) ++req_bits;
    if (ma.words == 0 || ma.words > MAX_WORDS) return hipErrorInvalidValue;
    // stable by request: (req, idx)[0] -> [1]
    auto sort_by_request = [&] {
        size_t bytes = b.temp_bytes;
        return rocprim::radix_sort_pairs(b.temp, bytes, mb.req[0], mb.req[1], mb.idx[0], mb.idx[1], a.entries, 0, (int)req_bits, stream);
    };
    // (request, asset) order: stable by asset, then stable by request
    if ((e = sort_by_asset(b, a.entries, stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(req_key_kernel, dim3(grid), dim3(BLOCK), 0, stream, b.c_entry[1], mb.qbeg, nr, a.k, mb.req[0], mb.idx[0], a.entries);
    if ((e = sort_by_request()) != hipSuccess) return e;
    hipLaunchKernelGGL(gather_kernel, dim3(grid), dim3(BLOCK), 0, stream, mb.idx[1], b.c_asset[1], b.c_entry[1], b.c_asset[0], b.c_entry[0], a.entries);
    queue_weights(b, a, b.c_entry[0], stream);
    if ((e = hipMemsetAsync(mb.n_assets, 0, (size_t)nr * sizeof(uint32_t), stream)) != hipSuccess) return e;
    const ScoreManyParams sp{b.c_asset[0], mb.req[1], b.score[1], b.ws, b.order[1], b.idf_q, mb.qbeg, b.score[0], b.order[0], b.matches, mb.n_assets,
                             a.entries, a.nq, ma.words};
    queue_scoring(score_kernel<ScoreManyParams>, sp, a.entries, ma.words, stream);
    // every request's assets in (-score, asset) order: stable by score (descending), then stable by request
    if ((e = sort_by_score(b, a.entries, stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(head_key_kernel, dim3(grid), dim3(BLOCK), 0, stream, b.score[1], b.order[1], mb.req[1], nr, mb.req[0], mb.idx[0], a.entries);
    if ((e = sort_by_request()) != hipSuccess) return e;
    hipLaunchKernelGGL(req_scan_kernel, dim3(1), dim3(BLOCK), 0, stream, mb.n_assets, nr, a.limit, mb.a_start, mb.e_start, a.out_info);
    hipLaunchKernelGGL(result_chunks_kernel, dim3((ma.cap + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, stream, mb.e_start, mb.a_start, mb.idx[1], b.matches, nr, mb.cnt, ma.cap);
    size_t bytes = b.temp_bytes;
    e = rocprim::exclusive_scan(b.temp, bytes, mb.cnt, mb.c_pos, 0u, ma.cap, rocprim::plus<uint32_t>(), stream);
    if (e != hipSuccess) return e;
    const EmitManyParams ep{b.score[0], mb.idx[1], b.c_asset[0], b.c_entry[0], b.matches, mb.a_start, mb.e_start, mb.c_pos, mb.qbeg,
                            chunk_params(b, a), a.out_results, a.out_info, nr};
    const uint32_t waves_wanted = ma.cap, blocks = std::min<uint32_t>((waves_wanted + 3) / 4, 2048);
    hipLaunchKernelGGL(emit_many_kernel<EmitManyParams>, dim3(blocks ? blocks : 1), dim3(BLOCK), 0, stream, ep);
    return hipGetLastError();
}

hipError_t queue_exact_many(Buffers& b, const ManyBuffers& mb, const ExactManyArgs& ma, hipStream_t stream) {
    const ExactArgs& a = ma.e;
    hipError_t e;
    const uint32_t nr = ma.n_req, grid = (a.entries + BLOCK - 1) / BLOCK;
    uint32_t req_bits = 1;                                   // request keys 0 .. n_req (n_req: the non-heads and the dropped assets)
    while ((1u << req_bits) <= nr) ++req_bits;
    if (ma.words == 0 || ma.words > MAX_WORDS) return hipErrorInvalidValue;
    auto sort_by_request = [&] {
        size_t bytes = b.temp_bytes;
        return rocprim::radix_sort_pairs(b.temp, bytes, mb.req[0], mb.req[1], mb.idx[0], mb.idx[1], a.entries, 0, (int)req_bits, stream);
    };
    // (the caller has run exact_prepare over the round's lookups and given simprints: hits / offsets / entries are in place)
    ExactCompactParams cp{b.rec, a.d_of_g, b.nbest, b.offs, b.c_asset[0], b.c_entry[0], a.k};
    hipLaunchKernelGGL(exact_compact_kernel, dim3(a.ng), dim3(BLOCK), 0, stream, cp);
    // (request, asset) order: stable by asset, then stable by request (an entry's request is that of its given simprint; mb.qbeg
    // holds the first GIVEN simprint of every request).  The compaction wrote the entries in visiting order -- given simprint
    // ascending, then key -- and BOTH sorts are stable, so inside a (request, asset) run the entries are still in that order: the
    // first-seen order of exact_score_kernel's distinct matched simprints is the reference's, per request.
    if ((e = sort_by_asset(b, a.entries, stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(req_key_kernel, dim3(grid), dim3(BLOCK), 0, stream, b.c_entry[1], mb.qbeg, nr, a.k, mb.req[0], mb.idx[0], a.entries);
    if ((e = sort_by_request()) != hipSuccess) return e;
    hipLaunchKernelGGL(gather_kernel, dim3(grid), dim3(BLOCK), 0, stream, mb.idx[1], b.c_asset[1], b.c_entry[1], b.c_asset[0], b.c_entry[0], a.entries);
    uint32_t* const e_d = b.order[1];
    uint32_t* const e_f = reinterpret_cast<uint32_t*>(b.score[1]);
    hipLaunchKernelGGL(exact_weights_kernel, dim3(grid), dim3(BLOCK), 0, stream, b.c_entry[0], a.d_of_g, b.freq_q, e_d, e_f, b.n_assets, a.entries, a.k);
    if ((e = hipMemsetAsync(mb.n_assets, 0, (size_t)nr * sizeof(uint32_t), stream)) != hipSuccess) return e;
    const ExactScoreManyParams sp{b.c_asset[0], mb.req[1], e_d, e_f, ma.dbeg, ma.queried, b.score[0], b.order[0], b.matches, mb.n_assets,
                                  a.entries, ma.words, a.threshold};
    queue_scoring(exact_score_kernel<ExactScoreManyParams>, sp, a.entries, ma.words, stream);
    // every request's kept assets in (-score, asset) order: stable by score (descending), then stable by request (a dropped asset's
    // score is -1: it goes behind every request with the non-heads)
    if ((e = sort_by_score(b, a.entries, stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(head_key_kernel, dim3(grid), dim3(BLOCK), 0, stream, b.score[1], b.order[1], mb.req[1], nr, mb.req[0], mb.idx[0], a.entries);
    if ((e = sort_by_request()) != hipSuccess) return e;
    hipLaunchKernelGGL(req_scan_kernel, dim3(1), dim3(BLOCK), 0, stream, mb.n_assets, nr, a.limit, mb.a_start, mb.e_start, a.out_info);
    hipLaunchKernelGGL(result_chunks_kernel, dim3((ma.cap + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, stream, mb.e_start, mb.a_start, mb.idx[1], b.matches, nr, mb.cnt, ma.cap);
    size_t bytes = b.temp_bytes;
    e = rocprim::exclusive_scan(b.temp, bytes, mb.cnt, mb.c_pos, 0u, ma.cap, rocprim::plus<uint32_t>(), stream);
    if (e != hipSuccess) return e;
    const ChunkParams collisions{b.rec, nullptr, nullptr, {}, a.out_chunks, nullptr, a.k, 0, 0};
    const EmitExactManyParams ep{{b.score[0], mb.idx[1], b.c_asset[0], b.c_entry[0], b.matches, mb.a_start, mb.e_start, mb.c_pos, mb.qbeg,
                                  collisions, a.out_results, a.out_info, nr}, a.d_of_g, b.freq_q};
    const uint32_t blocks = std::min<uint32_t>((ma.cap + 3) / 4, 2048);
    hipLaunchKernelGGL(emit_many_kernel<EmitExactManyParams>, dim3(blocks ? blocks : 1), dim3(BLOCK), 0, stream, ep);
    return hipGetLastError();
}

}  // namespace isksp
