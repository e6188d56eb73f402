// threshold_kernels.hip.h -- where a query's threshold comes from: the histogram cut finder, the given radius, the bootstrap
// over the first rows (one query or BOOT_QB queries per block), the pick between levels, the exact histogram of the fallback.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "scan_params.hip.h"

namespace isk {

// ---------------------------------------------------------------------------------------------
// find the first histogram bin where the running count reaches `need`  (wave 0 does the work)
//   returns the bin in res[0] and the count strictly below it in res[1]; every thread gets both.
//   nbins <= 320.  If the total is below `need` the last bin is returned.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void block_find_cut(const uint32_t* hist, uint32_t nbins, uint32_t need,
                                               uint32_t* res, uint32_t& bin, uint32_t& less) {
    const uint32_t tid = threadIdx.x;
    if (tid < 64) {
        uint32_t c[5], s = 0;
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            const uint32_t b = tid * 5 + j;
            c[j] = b < nbins ? hist[b] : 0u;
            s += c[j];
        }
        uint32_t incl = s;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t t = __shfl_up(incl, off, 64);
            if (tid >= (uint32_t)off) incl += t;
        }
        const uint32_t excl = incl - s;
        const uint32_t total = __shfl(incl, 63, 64);
        if (tid == 0 && total < need) {          // not enough entries: take everything
            uint32_t last = 0, run = 0, below = 0;
            for (uint32_t b = 0; b < nbins; ++b) { if (hist[b]) { last = b; below = run; } run += hist[b]; }
            res[0] = last; res[1] = below;
        }
        if (total >= need && excl < need && need <= incl) {
            uint32_t run = excl;
#pragma unroll
            for (int j = 0; j < 5; ++j) {
                if (run + c[j] >= need) { res[0] = tid * 5 + j; res[1] = run; break; }
                run += c[j];
            }
        }
    }
    __syncthreads();
    bin = res[0];
    less = res[1];
    __syncthreads();
}

// range-limited searches have a given threshold: one launch sets every bias and zeroes the candidate counters
__global__ __launch_bounds__(BLOCK) void radius_init_kernel(uint32_t* bias, uint32_t* cnt, uint32_t nq, uint32_t nq_pad, uint32_t value) {
    const uint32_t q = blockIdx.x * BLOCK + threadIdx.x;
    if (q >= nq_pad) return;
    bias[q] = q < nq ? value : BIAS_NEVER;
    cnt[(uint64_t)q * CNT_STRIDE] = 0;
}

// ... and for a handful of queries the queries themselves, carried in the kernel's arguments ([nq_pad][4] words)
constexpr uint32_t INLINE_QUERIES = 16;
struct InlineQueries { uint64_t w[INLINE_QUERIES * 4]; };
__global__ __launch_bounds__(BLOCK) void radius_init_inline_kernel(uint32_t* bias, uint32_t* cnt, uint32_t nq, uint32_t nq_pad, uint32_t value,
                                                                   uint64_t* queries, const InlineQueries iq) {
    const uint32_t i = threadIdx.x;
    if (i < nq_pad * 4) queries[i] = iq.w[i];
    if (i < nq_pad) {
        bias[i] = i < nq ? value : BIAS_NEVER;
        cnt[(uint64_t)i * CNT_STRIDE] = 0;
    }
}

struct BootParams {
    const uint64_t* col[4];
    const uint64_t* queries;  // [nq_pad][4]
    uint32_t* bias;           // [nq_pad] out
    uint32_t* cnt;            // [nq_pad * CNT_STRIDE] candidate counters: zeroed here (saves the host a memset)
    uint64_t s0;              // rows [0, s0) are sampled (s0 >= 1)
    uint32_t nq;              // real queries; blocks q >= nq write BIAS_NEVER
    uint32_t k;
    uint32_t W;
    uint64_t mask_last;
    float* thr;               // [nq_pad] out, nullable: tau0 - popc(query) as the MFMA scan compares it (MODE_SELF)
    uint32_t thr_packed;      // ... written PACKED (pack_threshold, scan_params.hip.h) for mfma_pack_kernel
    uint32_t* counts;         // [nq_pad][HB], nullable: zeroed here -- the distance counters of the self-tightening pass
    uint32_t hint;            // BOOT_NO_HINT, or the threshold itself (no sample): the k-th distance a previous batch of this size ended at + margin
};
constexpr uint32_t BOOT_NO_HINT = 0xFFFFFFFFu;
// the bootstrap threshold (dot-product form: tau0 - popc(query); never = no row can be a candidate) in the scan's representation
__device__ __forceinline__ void store_boot_threshold(const BootParams& p, uint32_t q, int thr, bool never) {
    if (p.thr_packed) reinterpret_cast<uint32_t*>(p.thr)[q] = never ? 0u : pack_threshold(thr);
    else p.thr[q] = never ? -1.0e9f : (float)thr;
}
constexpr uint64_t BOOT_EXACT_ROWS = 4096;   // rows of the full histogram; the rest of a longer sample only counts under its cut
// ... unless k is large: then the whole sample stays exact (the cut of the first rows must leave >= k rows under it)
__device__ __forceinline__ uint64_t boot_exact_rows(const BootParams& p) {
    return (p.s0 <= BOOT_EXACT_ROWS || (uint64_t)p.k * 4 > BOOT_EXACT_ROWS) ? p.s0 : BOOT_EXACT_ROWS;
}

// the longer part of the bootstrap sample: rows [s1, s0) that lie at or under `cut` go into the histogram.  W is a
// template argument so that the eight rows of a trip are eight INDEPENDENT loads (with a run-time word loop hipcc keeps
// them in program order and the loop waits out one L2 latency per row: 115 us per 65 536 rows instead of ~15)
template <int W>
__device__ __forceinline__ void boot_tail(const BootParams& p, const uint64_t (&qw)[4], uint64_t s1, uint32_t cut, uint32_t* hist) {
    const uint32_t tid = threadIdx.x, nthr = blockDim.x;
    for (uint64_t r0 = s1 + tid; r0 < p.s0; r0 += 8 * nthr) {
        uint64_t x[8][W];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const uint64_t r = r0 + (uint64_t)u * nthr;
            const uint64_t rr = r < p.s0 ? r : s1;          // clamped: the value is discarded below
#pragma unroll
            for (int w = 0; w < W; ++w) x[u][w] = p.col[w][rr];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            uint32_t h = 0;
#pragma unroll
            for (int w = 0; w < W; ++w) {
                uint64_t y = x[u][w] ^ qw[w];
                if (w == W - 1) y &= p.mask_last;
                h += (uint32_t)__builtin_popcountll(y);
            }
            if (h <= cut && r0 + (uint64_t)u * nthr < p.s0) atomicAdd(&hist[h], 1u);
        }
    }
}

// one block per (padded) query: tau0 = k-th smallest hamming over the first s0 rows.  The first BOOT_EXACT_ROWS rows
// go into a full histogram (LDS atomics on a handful of hot bins: ~6 us); a longer sample then only counts the rows at
// or under THAT cut -- a few per thousand.  Any block size from 64 to 1 024 threads: with a handful of queries the host
// launches wide blocks, or the sample of a query would be one block's latency-bound walk.
__global__ __launch_bounds__(1024) void boot_kernel(const BootParams p) {
    __shared__ uint32_t hist[320];
    __shared__ uint32_t res[2];
    const uint32_t q = blockIdx.x, tid = threadIdx.x, nthr = blockDim.x;
    if (tid == 0) p.cnt[(uint64_t)q * CNT_STRIDE] = 0;
    if (p.counts)
        for (uint32_t i = tid; i < HB; i += nthr) p.counts[(uint64_t)q * HB + i] = 0;      // (saves the host a memset launch)
    if (q >= p.nq) {
        if (tid == 0) {
            p.bias[q] = BIAS_NEVER;
            if (p.thr) store_boot_threshold(p, q, 0, true);       // below every dot product: never a candidate
        }
        return;
    }
    uint64_t qw[4];
    for (uint32_t w = 0; w < 4; ++w) qw[w] = w < p.W ? p.queries[(uint64_t)q * 4 + w] : 0;
    if (p.hint != BOOT_NO_HINT) {      // (uniform: a launch parameter) the threshold is given -- the host verifies that it held k rows
        if (tid == 0) {
            p.bias[q] = 0x7FFFFFFFu - p.hint;
            if (p.thr) {
                uint32_t pc = 0;
                for (uint32_t w = 0; w < p.W; ++w) pc += (uint32_t)__builtin_popcountll(w == p.W - 1 ? qw[w] & p.mask_last : qw[w]);
                store_boot_threshold(p, q, (int)p.hint - (int)pc, false);
            }
        }
        return;
    }
    for (uint32_t i = tid; i < 320; i += nthr) hist[i] = 0;
    __syncthreads();
    const uint64_t s1 = boot_exact_rows(p);
    for (uint64_t r = tid; r < s1; r += nthr) {
        uint32_t h = 0;
        for (uint32_t w = 0; w < p.W; ++w) {
            uint64_t x = p.col[w][r] ^ qw[w];
            if (w == p.W - 1) x &= p.mask_last;
            h += (uint32_t)__builtin_popcountll(x);
        }
        atomicAdd(&hist[h], 1u);
    }
    __syncthreads();
    uint32_t bin, less;
    block_find_cut(hist, NBINS, p.k < s1 ? p.k : (uint32_t)s1, res, bin, less);
    if (p.s0 > s1) {
        // (uniform branch: s0 is a launch parameter)  bins <= `bin` become exact over [0, s0); the k-th smallest lies there
        switch (p.W) {
            case 1: boot_tail<1>(p, qw, s1, bin, hist); break;
            case 2: boot_tail<2>(p, qw, s1, bin, hist); break;
            case 3: boot_tail<3>(p, qw, s1, bin, hist); break;
            default: boot_tail<4>(p, qw, s1, bin, hist); break;
        }
        __syncthreads();
        block_find_cut(hist, NBINS, p.k < p.s0 ? p.k : (uint32_t)p.s0, res, bin, less);
    }
    if (tid == 0) {
        p.bias[q] = 0x7FFFFFFFu - bin;
        if (p.thr) {
            uint32_t pc = 0;
            for (uint32_t w = 0; w < p.W; ++w) pc += (uint32_t)__builtin_popcountll(w == p.W - 1 ? qw[w] & p.mask_last : qw[w]);
            store_boot_threshold(p, q, (int)bin - (int)pc, false);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// boot_multi_kernel<W>: the same bootstrap for LARGE batches, BOOT_QB queries per 1 024-thread block.  With one block per query
// 1 024 blocks each read the whole 512 KB sample from the L2 (~0.5 GB per launch, ~11 TB/s for 45 us): here a row is loaded
// once per BOOT_QB queries and the kernel is bound by its XOR + popcount work instead.  nq_pad is a multiple of 8, hence of 4.
// ---------------------------------------------------------------------------------------------
constexpr int BOOT_QB = 4;      // (8 measured slower: 128 blocks leave the chip short of waves; 1 M rows x 1 024 queries 0.213 against 0.191 ms)
template <int W>
__global__ __launch_bounds__(1024) void boot_multi_kernel(const BootParams p) {
    __shared__ uint32_t hist[BOOT_QB][320];
    __shared__ uint32_t res[2];
    const uint32_t q0 = blockIdx.x * BOOT_QB, tid = threadIdx.x, nthr = blockDim.x;
    if (tid < BOOT_QB) p.cnt[(uint64_t)(q0 + tid) * CNT_STRIDE] = 0;
    if (p.counts)
        for (uint32_t i = tid; i < BOOT_QB * HB; i += nthr) p.counts[(uint64_t)q0 * HB + i] = 0;
    for (uint32_t i = tid; i < BOOT_QB * 320; i += nthr) (&hist[0][0])[i] = 0;
    uint64_t qw[BOOT_QB][W];
#pragma unroll
    for (int i = 0; i < BOOT_QB; ++i)
#pragma unroll
        for (int w = 0; w < W; ++w) qw[i][w] = p.queries[(uint64_t)(q0 + i) * 4 + w];     // uniform addresses: scalar loads
    __syncthreads();
    auto hamming = [&](const uint64_t (&x)[W], int i) {
        uint32_t h = 0;
#pragma unroll
        for (int w = 0; w < W; ++w) {
            uint64_t y = x[w] ^ qw[i][w];
            if (w == W - 1) y &= p.mask_last;
            h += (uint32_t)__builtin_popcountll(y);
        }
        return h;
    };
    const uint64_t s1 = boot_exact_rows(p);
    for (uint64_t r = tid; r < s1; r += nthr) {
        uint64_t x[W];
#pragma unroll
        for (int w = 0; w < W; ++w) x[w] = p.col[w][r];
#pragma unroll
        for (int i = 0; i < BOOT_QB; ++i) atomicAdd(&hist[i][hamming(x, i)], 1u);
    }
    __syncthreads();
    uint32_t cut[BOOT_QB], less;
#pragma unroll
    for (int i = 0; i < BOOT_QB; ++i) block_find_cut(hist[i], NBINS, p.k < s1 ? p.k : (uint32_t)s1, res, cut[i], less);
    if (p.s0 > s1) {
        // bins <= cut[i] become exact over [0, s0); the k-th smallest of query i lies there.  Eight independent rows per
        // thread and trip, each scored against the block's queries.
        for (uint64_t r0 = s1 + tid; r0 < p.s0; r0 += 8 * (uint64_t)nthr) {
            uint64_t x[8][W];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const uint64_t r = r0 + (uint64_t)u * nthr;
                const uint64_t rr = r < p.s0 ? r : s1;          // clamped: the value is discarded below
#pragma unroll
                for (int w = 0; w < W; ++w) x[u][w] = p.col[w][rr];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const bool real = r0 + (uint64_t)u * nthr < p.s0;
#pragma unroll
                for (int i = 0; i < BOOT_QB; ++i) {
                    const uint32_t h = hamming(x[u], i);
                    if (h <= cut[i] && real) atomicAdd(&hist[i][h], 1u);
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < BOOT_QB; ++i) block_find_cut(hist[i], NBINS, p.k < p.s0 ? p.k : (uint32_t)p.s0, res, cut[i], less);
    }
    if (tid == 0) {
#pragma unroll
        for (int i = 0; i < BOOT_QB; ++i) {
            const uint32_t q = q0 + i;
            if (q >= p.nq) {
                p.bias[q] = BIAS_NEVER;
                if (p.thr) store_boot_threshold(p, q, 0, true);       // below every dot product: never a candidate
                continue;
            }
            p.bias[q] = 0x7FFFFFFFu - cut[i];
            if (p.thr) {
                uint32_t pc = 0;
#pragma unroll
                for (int w = 0; w < W; ++w) pc += (uint32_t)__builtin_popcountll(w == W - 1 ? qw[i][w] & p.mask_last : qw[i][w]);
                store_boot_threshold(p, q, (int)cut[i] - (int)pc, false);
            }
        }
    }
}

struct PickParams {
    const uint32_t* ghist;   // [nq_pad][HB]
    uint32_t* bias;          // [nq_pad] in/out
    uint32_t nq;
    uint32_t need;           // min(k, rows seen so far)
    uint32_t* cnt;           // [nq_pad * CNT_STRIDE] candidate counters   (nullptr: no pruning)
    uint64_t* cand;          // [nq_pad][cap] candidate lists, pruned in place to the new threshold
    uint32_t cap;
};

// one block per query: tau = first bin of the running histogram where the count reaches `need`; then the
// candidates collected so far under looser thresholds are pruned to it, so that the list holds ~need entries
// (+ ties) whatever the number of levels.
__global__ __launch_bounds__(BLOCK) void pick_kernel(const PickParams p) {
    __shared__ uint32_t hist[320];
    __shared__ uint32_t res[2];
    __shared__ uint32_t wsum[BLOCK / 64];
    __shared__ uint32_t base;
    const uint32_t q = blockIdx.x, tid = threadIdx.x;
    if (q >= p.nq) return;
    for (uint32_t i = tid; i < 320; i += BLOCK) hist[i] = i < NBINS ? p.ghist[(uint64_t)q * HB + i] : 0u;
    __syncthreads();
    uint32_t bin, less;
    block_find_cut(hist, NBINS, p.need, res, bin, less);
    // never loosen the threshold (the histogram only holds bins <= the threshold its rows were scanned under)
    const uint32_t tau0 = 0x7FFFFFFFu - p.bias[q];
    const uint32_t tau = bin < tau0 ? bin : tau0;
    if (tid == 0) { p.bias[q] = 0x7FFFFFFFu - tau; base = 0; }
    if (!p.cand) return;
    const uint32_t total = p.cnt[(uint64_t)q * CNT_STRIDE];
    if (total > p.cap) return;            // overflowed: select_kernel flags it, the host reruns the query exactly
    uint64_t* list = p.cand + (uint64_t)q * p.cap;
    __syncthreads();
    // in-place stable compaction, one 256-entry chunk at a time: a chunk is read into registers before anything
    // of it is written, and the write position never passes the read position
    for (uint32_t start = 0; start < total; start += BLOCK) {
        const uint32_t i = start + tid;
        uint64_t c = 0;
        bool keep = false;
        if (i < total) { c = list[i]; keep = (uint32_t)(c >> 48) <= tau; }
        const uint64_t ball = __ballot(keep);
        const uint32_t lane = tid & 63, wave = tid >> 6;
        const uint32_t before = (uint32_t)__popcll(ball & ((1ull << lane) - 1ull));
        if (lane == 0) wsum[wave] = (uint32_t)__popcll(ball);
        __syncthreads();
        uint32_t off = base;
        for (uint32_t w = 0; w < wave; ++w) off += wsum[w];
        __syncthreads();
        if (keep) list[off + before] = c;
        if (tid == 0) base += wsum[0] + wsum[1] + wsum[2] + wsum[3];
        __syncthreads();
    }
    if (tid == 0) p.cnt[(uint64_t)q * CNT_STRIDE] = base;
}

// ---------------------------------------------------------------------------------------------
// fullhist_kernel: exact hamming histogram of ONE query over a whole segment (overflow fallback)
// ---------------------------------------------------------------------------------------------
struct FullHistParams {
    const uint64_t* col[4];
    uint64_t n_rows;
    const uint64_t* query;    // [4]
    uint32_t* ghist;          // [HB] (zeroed by the host)
    uint32_t W;
    uint64_t mask_last;
};
__global__ __launch_bounds__(BLOCK) void fullhist_kernel(const FullHistParams p) {
    __shared__ uint32_t hist[320];
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid; i < 320; i += BLOCK) hist[i] = 0;
    __syncthreads();
    uint64_t qw[4];
    for (uint32_t w = 0; w < 4; ++w) qw[w] = w < p.W ? p.query[w] : 0;
    for (uint64_t r = (uint64_t)blockIdx.x * BLOCK + tid; r < p.n_rows; r += (uint64_t)gridDim.x * BLOCK) {
        uint32_t h = 0;
        for (uint32_t w = 0; w < p.W; ++w) {
            uint64_t x = p.col[w][r] ^ qw[w];
            if (w == p.W - 1) x &= p.mask_last;
            h += (uint32_t)__builtin_popcountll(x);
        }
        atomicAdd(&hist[h], 1u);
    }
    __syncthreads();
    for (uint32_t i = tid; i < NBINS; i += BLOCK)
        if (hist[i]) atomicAdd(&p.ghist[i], hist[i]);
}

}  // namespace isk
