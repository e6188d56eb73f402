// select_kernels.hip.h -- from candidates to records: the exact top-k select, the one-launch search of tiny segments, the
// key-radix fallback over the table's rows, the merge of sorted lists and the distinct-asset count (included by kernels.hip.h,
// which defines Record).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "scan_params.hip.h"
#include "threshold_kernels.hip.h"

namespace isk {

// ---------------------------------------------------------------------------------------------
// select_kernel<KW>: one block per query.  Exact top-k of the candidate list under (hamming, key).
//   1. histogram of hamming over the candidates -> cut h*, `less` = candidates below it
//   2. tie class h == h*: MSB-first radix select on the key (8 bits per pass) until the r smallest
//      keys of the class are pinned down
//   3. compact the keff winners into LDS, bitonic sort by (hamming, key_hi, key_lo), emit records
// dynamic LDS: sh[P] u32 | pad | klo[P] u64 | khi[P] u64 (KW == 2) | row[P] u32 (ROWS)
// ROWS: the segment row of every result travels through the sort and is written beside the records (out_rows) -- the
// simprint scoring kernels (simprint_score.hip) read the stored code and its document frequency by row, not by key.
// ---------------------------------------------------------------------------------------------
struct SelectParams {
    const uint32_t* cnt;      // [nq_pad * CNT_STRIDE]
    const uint64_t* cand;     // [nq_pad][cap]
    uint64_t cap;
    const uint64_t* keys;     // segment key column [rows*KW]
    const uint16_t* rank;     // [257] hamming -> order-preserving distance rank for this prefix
    Record* out;              // [nq][k]
    uint32_t* out_count;      // [nq]
    uint32_t* overflow;       // [nq] set to 1 when the candidate list overflowed
    uint32_t k;
    uint32_t P;               // power of two >= min(k, cap)
    uint32_t prefix_bits;
    uint32_t q_base;          // block b serves query q_base + b
    uint32_t overflow_count;  // what out_count[q] becomes when the candidate list overflowed: 0, or COUNT_OVERFLOW for callers
                              // that cannot look at the flags before the results travel on (search_device_async)
    uint32_t* out_rows;       // [nq][k] segment row of every record (select_kernel<KW, true> only)
    uint32_t* out_kth;        // nullable [nq]: hamming of the query's LAST result (0 when it has none) -- what the host needs of a
                              // result block that stays on the device to seed the next batch's threshold hint
};

template <int KW>
__device__ __forceinline__ void load_key(const uint64_t* keys, uint64_t row, uint64_t& hi, uint64_t& lo) {
    if constexpr (KW == 2) { hi = keys[2 * row]; lo = keys[2 * row + 1]; }
    else { hi = 0; lo = keys[row]; }
}
// digit d (0 = most significant byte) of a KW-word key
template <int KW>
__device__ __forceinline__ uint32_t key_digit(uint64_t hi, uint64_t lo, int d) {
    if constexpr (KW == 2) return d < 8 ? (uint32_t)(hi >> (56 - 8 * d)) & 255u : (uint32_t)(lo >> (56 - 8 * (d - 8))) & 255u;
    else return (uint32_t)(lo >> (56 - 8 * d)) & 255u;
}
// the key with everything below its first d bytes cleared
template <int KW>
__device__ __forceinline__ void key_top(uint64_t hi, uint64_t lo, int d, uint64_t& thi, uint64_t& tlo) {
    if constexpr (KW == 2) {
        if (d >= 16) { thi = hi; tlo = lo; }
        else if (d >= 8) { thi = hi; tlo = d == 8 ? 0 : lo & (~0ULL << (64 - 8 * (d - 8))); }
        else { thi = d == 0 ? 0 : hi & (~0ULL << (64 - 8 * d)); tlo = 0; }
    } else {
        thi = 0;
        tlo = d >= 8 ? lo : (d == 0 ? 0 : lo & (~0ULL << (64 - 8 * d)));
    }
}

// NT: threads per block.  One block per query holds its sort buffer in LDS (P = 4 096 slots with 128-bit keys and rows: 112 KB, one
// block per CU): with 256 threads that CU runs FOUR waves through ~60 bitonic stages and two rounds of dependent gathers -- a k = 400
// select took 47 us for 16 queries, 93 us for 512.  Large buffers (P >= 1 024) are launched with 1 024 threads.
// select_body: the whole select of query q over `total` candidates at `cand` (the block's dynamic LDS at smem); every thread of the block calls it.
template <int KW, bool ROWS, int NT>
__device__ __forceinline__ void select_body(const SelectParams& p, const uint32_t q, const uint64_t* cand, const uint32_t total, unsigned char* smem) {
    __shared__ uint32_t hist[320];
    __shared__ uint32_t res[2];
    __shared__ uint32_t n_out;
    const uint32_t P = p.P;
    uint32_t* sh = reinterpret_cast<uint32_t*>(smem);
    uint64_t* sklo = reinterpret_cast<uint64_t*>(smem + (((size_t)P * 4 + 15) & ~(size_t)15));
    uint64_t* skhi = sklo + P;   // only touched when KW == 2
    uint32_t* srow = reinterpret_cast<uint32_t*>(sklo + (size_t)P * KW);   // only touched when ROWS

    const uint32_t tid = threadIdx.x;
    if (tid == 0) p.overflow[q] = total > p.cap ? 1u : 0u;   // always written: the host never has to clear the flags
    if (total > p.cap) {             // candidate list overflowed: host reruns this query exactly
        if (tid == 0) { p.out_count[q] = p.overflow_count; if (p.out_kth) p.out_kth[q] = 0; }
        return;
    }
    const uint32_t keff = p.k < total ? p.k : total;
    if (keff == 0) {
        if (tid == 0) { p.out_count[q] = 0; if (p.out_kth) p.out_kth[q] = 0; }
        return;
    }

    // 1. cut on the hamming distance
    for (uint32_t i = tid; i < 320; i += NT) hist[i] = 0;
    if (tid == 0) n_out = 0;
    __syncthreads();
    for (uint32_t i = tid; i < total; i += NT) atomicAdd(&hist[(uint32_t)(cand[i] >> 48)], 1u);
    __syncthreads();
    uint32_t hstar, less;
    block_find_cut(hist, NBINS, keff, res, hstar, less);
    uint32_t tie = hist[hstar];
    uint32_t r = keff - less;            // 1 <= r <= tie
    __syncthreads();

    // 2. radix select on the key inside the tie class -- skipped when everything up to and including the tie
    //    class fits the sort buffer (the usual case: a few dozen rows): the sort then orders the ties by key and
    //    the first keff entries are the answer, without up to 8*KW dependent passes over the gathered keys
    uint64_t phi = 0, plo = 0;           // selected key prefix (first d bytes)
    int d = 0;
    const bool fits = less + tie <= P;
    while (!fits && r < tie && d < KW * 8) {
        for (uint32_t i = tid; i < 320; i += NT) hist[i] = 0;
        __syncthreads();
        for (uint32_t i = tid; i < total; i += NT) {
            const uint64_t c = cand[i];
            if ((uint32_t)(c >> 48) != hstar) continue;
            uint64_t khi, klo, thi, tlo;
            load_key<KW>(p.keys, c & 0xFFFFFFFFFFFFULL, khi, klo);
            key_top<KW>(khi, klo, d, thi, tlo);
            if (thi == phi && tlo == plo) atomicAdd(&hist[key_digit<KW>(khi, klo, d)], 1u);
        }
        __syncthreads();
        uint32_t b, below;
        block_find_cut(hist, 256, r, res, b, below);
        tie = hist[b];
        r -= below;
        if (KW == 2 && d < 8) phi |= (uint64_t)b << (56 - 8 * d);
        else plo |= (uint64_t)b << (56 - 8 * (KW == 2 ? d - 8 : d));
        ++d;
        __syncthreads();
    }
    // winners: hamming < h*, or hamming == h* and top-d key bytes <= selected prefix
    // (when the loop stopped with r == tie every key sharing the prefix is taken)

    // 3. compact
    for (uint32_t i = tid; i < total; i += NT) {
        const uint64_t c = cand[i];
        const uint32_t h = (uint32_t)(c >> 48);
        if (h > hstar) continue;
        uint64_t khi, klo;
        load_key<KW>(p.keys, c & 0xFFFFFFFFFFFFULL, khi, klo);
        if (h == hstar) {
            uint64_t thi, tlo;
            key_top<KW>(khi, klo, d, thi, tlo);
            if (thi > phi || (thi == phi && tlo > plo)) continue;
        }
        const uint32_t pos = atomicAdd(&n_out, 1u);
        if (pos < P) { sh[pos] = h; sklo[pos] = klo; if (KW == 2) skhi[pos] = khi; if (ROWS) srow[pos] = (uint32_t)(c & 0xFFFFFFFFFFFFULL); }
    }
    __syncthreads();
    const uint32_t got = n_out < P ? n_out : P;     // == keff when keys are unique
    // sort only as many slots as hold winners (a range-limited search asks for a large k and finds few rows)
    uint32_t Ps = 1;
    while (Ps < got) Ps <<= 1;
    for (uint32_t i = got + tid; i < Ps; i += NT) { sh[i] = 0xFFFFFFFFu; sklo[i] = ~0ULL; if (KW == 2) skhi[i] = ~0ULL; }
    __syncthreads();

    // bitonic sort ascending by (h, khi, klo)
    for (uint32_t size = 2; size <= Ps; size <<= 1) {
        for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
            for (uint32_t i = tid; i < (Ps >> 1); i += NT) {
                const uint32_t lo_i = 2 * i - (i & (stride - 1));
                const uint32_t hi_i = lo_i + stride;
                const bool up = (lo_i & size) == 0;
                const uint32_t ha = sh[lo_i], hb = sh[hi_i];
                const uint64_t la = sklo[lo_i], lb = sklo[hi_i];
                uint64_t ka = 0, kb = 0;
                if (KW == 2) { ka = skhi[lo_i]; kb = skhi[hi_i]; }
                const bool a_gt_b = ha != hb ? ha > hb : (ka != kb ? ka > kb : la > lb);
                if (a_gt_b == up) {
                    sh[lo_i] = hb; sh[hi_i] = ha;
                    sklo[lo_i] = lb; sklo[hi_i] = la;
                    if (KW == 2) { skhi[lo_i] = kb; skhi[hi_i] = ka; }
                    if (ROWS) { const uint32_t ra = srow[lo_i]; srow[lo_i] = srow[hi_i]; srow[hi_i] = ra; }
                }
            }
            __syncthreads();
        }
    }
    const uint32_t nres = got < keff ? got : keff;
    for (uint32_t i = tid; i < nres; i += NT) {
        Record rec;
        rec.key_hi = KW == 2 ? skhi[i] : 0;
        rec.key_lo = sklo[i];
        rec.dist_rank = p.rank[sh[i]];
        rec.hamming = (uint16_t)sh[i];
        rec.prefix_bits = (uint16_t)p.prefix_bits;
        p.out[(uint64_t)q * p.k + i] = rec;
        if (ROWS) p.out_rows[(uint64_t)q * p.k + i] = srow[i];
    }
    if (tid == 0) { p.out_count[q] = nres; if (p.out_kth) p.out_kth[q] = nres ? sh[nres - 1] : 0; }
}

template <int KW, bool ROWS = false, int NT = BLOCK>
__global__ __launch_bounds__(NT) void select_kernel(const SelectParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t q = p.q_base + blockIdx.x;
    select_body<KW, ROWS, NT>(p, q, p.cand + (uint64_t)q * p.cap, p.cnt[(uint64_t)q * CNT_STRIDE], smem);
}

// ---------------------------------------------------------------------------------------------
// tiny_search_kernel: a segment of a few thousand rows (option "tiny_rows", default 16 384) answered by ONE launch, one block per
// query: the block computes the distance of every row (range-limited searches keep the rows within the radius), lists them as
// candidates and runs the select on them -- exact by construction, no threshold to find or verify.  Such a search used to be
// three launches (threshold, scan, select: ~20 us of launches and hand-overs around ~5 us of work): the reference's own call shape
// on the index sizes its deployment guide names (BASELINE config 1: 2 500 rows per unit type).
// ---------------------------------------------------------------------------------------------
struct TinyParams {
    const uint64_t* col[4];
    const uint64_t* queries;  // [nq_pad][4] device copy (used when !use_inline)
    uint64_t* cand;           // [nq_pad][cap]
    uint64_t mask_last;       // of the last compared word
    uint32_t n_rows;          // <= cap
    uint32_t W;               // compared words
    int32_t radius;           // >= 0: rows within it only
    uint32_t use_inline;
};
template <int KW, bool ROWS, int NT>
__global__ __launch_bounds__(NT) void tiny_search_kernel(const TinyParams t, const SelectParams p, const InlineQueries iq) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ uint32_t n_cand;
    const uint32_t tid = threadIdx.x;
    const uint32_t q = p.q_base + blockIdx.x;
    uint64_t qw[4];
#pragma unroll
    for (int w = 0; w < 4; ++w) qw[w] = t.use_inline ? iq.w[(q % INLINE_QUERIES) * 4 + w] : t.queries[(uint64_t)q * 4 + w];
    if (tid == 0) n_cand = 0;
    __syncthreads();
    uint64_t* const cand = t.cand + (uint64_t)q * p.cap;
#pragma unroll 4
    for (uint32_t row = tid; row < t.n_rows; row += NT) {
        uint32_t hd = 0;
#pragma unroll
        for (uint32_t w = 0; w < 4; ++w) {
            if (w < t.W) {
                uint64_t x = t.col[w][row] ^ qw[w];
                if (w + 1 == t.W) x &= t.mask_last;
                hd += (uint32_t)__popcll(x);
            }
        }
        if (t.radius < 0 || hd <= (uint32_t)t.radius) cand[atomicAdd(&n_cand, 1u)] = ((uint64_t)hd << 48) | row;
    }
    __syncthreads();             // (a workgroup-scope fence with it: the block reads back its own candidate words)
    select_body<KW, ROWS, NT>(p, q, cand, n_cand, smem);
}

// ---------------------------------------------------------------------------------------------
// Overflow fallback for tie classes too large to collect: radix select on the KEY over the rows of
// the table itself.  One query at a time; plain (unpipelined) scans -- this path only runs for
// adversarial data (e.g. millions of identical codes).
//   fb_keyhist_kernel  histogram of key byte `d` over rows with hamming == tau whose first d key
//                      bytes equal the selected prefix
//   fb_collect_kernel  append rows with hamming < tau, or hamming == tau and top-d key bytes <= prefix
// ---------------------------------------------------------------------------------------------
struct FbParams {
    const uint64_t* col[4];
    const uint64_t* keys;
    uint64_t n_rows;
    const uint64_t* query;    // [4]
    uint32_t W, KW;
    uint64_t mask_last;
    uint32_t tau;
    int d;                    // key bytes already fixed
    uint64_t phi, plo;        // the fixed prefix (as a key with the lower bytes cleared)
    uint32_t* ghist;          // [256]  (fb_keyhist_kernel)
    uint32_t* cnt;            // [1]    (fb_collect_kernel)
    uint64_t* cand;           // [cap]
    uint32_t cap;
};
__device__ __forceinline__ uint32_t fb_hamming(const FbParams& p, const uint64_t (&qw)[4], uint64_t r) {
    uint32_t h = 0;
    for (uint32_t w = 0; w < p.W; ++w) {
        uint64_t x = p.col[w][r] ^ qw[w];
        if (w == p.W - 1) x &= p.mask_last;
        h += (uint32_t)__builtin_popcountll(x);
    }
    return h;
}
template <int KW>
__global__ __launch_bounds__(BLOCK) void fb_keyhist_kernel(const FbParams p) {
    __shared__ uint32_t hist[256];
    const uint32_t tid = threadIdx.x;
    hist[tid] = 0;
    __syncthreads();
    uint64_t qw[4];
    for (uint32_t w = 0; w < 4; ++w) qw[w] = w < p.W ? p.query[w] : 0;
    for (uint64_t r = (uint64_t)blockIdx.x * BLOCK + tid; r < p.n_rows; r += (uint64_t)gridDim.x * BLOCK) {
        if (fb_hamming(p, qw, r) != p.tau) continue;
        uint64_t khi, klo, thi, tlo;
        load_key<KW>(p.keys, r, khi, klo);
        key_top<KW>(khi, klo, p.d, thi, tlo);
        if (thi == p.phi && tlo == p.plo) atomicAdd(&hist[key_digit<KW>(khi, klo, p.d)], 1u);
    }
    __syncthreads();
    if (hist[tid]) atomicAdd(&p.ghist[tid], hist[tid]);
}
template <int KW>
__global__ __launch_bounds__(BLOCK) void fb_collect_kernel(const FbParams p) {
    const uint32_t tid = threadIdx.x;
    uint64_t qw[4];
    for (uint32_t w = 0; w < 4; ++w) qw[w] = w < p.W ? p.query[w] : 0;
    for (uint64_t r = (uint64_t)blockIdx.x * BLOCK + tid; r < p.n_rows; r += (uint64_t)gridDim.x * BLOCK) {
        const uint32_t h = fb_hamming(p, qw, r);
        if (h > p.tau) continue;
        if (h == p.tau && p.d > 0) {
            uint64_t khi, klo, thi, tlo;
            load_key<KW>(p.keys, r, khi, klo);
            key_top<KW>(khi, klo, p.d, thi, tlo);
            if (thi > p.phi || (thi == p.phi && tlo > p.plo)) continue;
        }
        const uint32_t slot = atomicAdd(p.cnt, 1u);
        if (slot < p.cap) p.cand[slot] = ((uint64_t)h << 48) | r;
    }
}

// ---------------------------------------------------------------------------------------------
// merge_kernel: per query, k-way merge of n_lists record lists, each sorted by (dist_rank, key).
//   rank of an element = its position in its own list + the number of elements of every other
//   list that sort before it (binary search); ranks are distinct because keys are.
// ---------------------------------------------------------------------------------------------
struct MergeParams {
    const unsigned char* lists;   // list l: records at lists + l*list_stride, laid out [nq][k]
    const unsigned char* counts;  // list l: counts  at counts + l*count_stride, laid out [nq]
    uint64_t list_stride;         // bytes between the record blocks of consecutive lists
    uint64_t count_stride;        // bytes between the count blocks of consecutive lists
    Record* out;                  // [nq][k]
    uint32_t* out_count;          // [nq]
    uint32_t n_lists, nq, k;
};
__device__ __forceinline__ bool rec_less(const Record& a, const Record& b) {
    if (a.dist_rank != b.dist_rank) return a.dist_rank < b.dist_rank;
    if (a.key_hi != b.key_hi) return a.key_hi < b.key_hi;
    return a.key_lo < b.key_lo;
}
__global__ __launch_bounds__(BLOCK) void merge_kernel(const MergeParams p) {
    const uint32_t q = blockIdx.x, tid = threadIdx.x;
    auto list_of = [&](uint32_t l) { return reinterpret_cast<const Record*>(p.lists + (uint64_t)l * p.list_stride) + (uint64_t)q * p.k; };
    auto raw_count = [&](uint32_t l) { return reinterpret_cast<const uint32_t*>(p.counts + (uint64_t)l * p.count_stride)[q]; };
    auto count_of = [&](uint32_t l) {
        const uint32_t c = raw_count(l);
        return c < p.k ? c : p.k;
    };
    uint32_t total = 0;
    for (uint32_t l = 0; l < p.n_lists; ++l) {
        if (raw_count(l) == COUNT_OVERFLOW) {      // a list that could not be completed without the host: pass the marker on
            if (tid == 0) p.out_count[q] = COUNT_OVERFLOW;
            return;
        }
        total += count_of(l);
    }
    const uint32_t keff = total < p.k ? total : p.k;
    for (uint32_t e = tid; e < p.n_lists * p.k; e += BLOCK) {
        const uint32_t l = e / p.k, i = e % p.k;
        if (i >= count_of(l)) continue;
        const Record me = list_of(l)[i];
        uint32_t rank = i;
        for (uint32_t o = 0; o < p.n_lists && rank < keff; ++o) {
            if (o == l) continue;
            const Record* lst = list_of(o);
            uint32_t lo = 0, hi = count_of(o);
            // elements of list o sorting before `me`; an (impossible) exact tie goes to the lower list id
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                const bool before = o < l ? !rec_less(me, lst[mid]) : rec_less(lst[mid], me);
                if (before) lo = mid + 1; else hi = mid;
            }
            rank += lo;
        }
        if (rank < keff) p.out[(uint64_t)q * p.k + rank] = me;
    }
    if (tid == 0) p.out_count[q] = keff;
}

// ---------------------------------------------------------------------------------------------
// document frequency: distinct assets in one query's collision list.  The list is ordered by key, so
// the rows of one asset (= first key word of a 2-word key) are adjacent: count the boundaries.
// ---------------------------------------------------------------------------------------------
struct DistinctParams {
    const Record* rec;        // [nq][k] ascending (dist_rank, key)
    const uint32_t* count;    // [nq]
    uint32_t* out;            // [nq]
    uint32_t k, KW;
};
__global__ __launch_bounds__(BLOCK) void distinct_kernel(const DistinctParams p) {
    __shared__ uint32_t total;
    const uint32_t q = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) total = 0;
    __syncthreads();
    const uint32_t n = p.count[q] < p.k ? p.count[q] : p.k;
    const Record* r = p.rec + (uint64_t)q * p.k;
    uint32_t mine = 0;
    for (uint32_t i = tid; i < n; i += BLOCK)
        mine += (i == 0 || p.KW == 1 || r[i].key_hi != r[i - 1].key_hi) ? 1u : 0u;
    for (int off = 32; off > 0; off >>= 1) mine += __shfl_down(mine, off);
    if ((tid & 63) == 0 && mine) atomicAdd(&total, mine);
    __syncthreads();
    if (tid == 0) p.out[q] = total;
}

}  // namespace isk
