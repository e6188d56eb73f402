// table_kernels.hip.h -- upkeep of the column store: synthetic fill, row moves, row gathers, the ingest split and mask, u32 gathers;
// the two kernels around the joins of isccsearch_join_components (row labels before them, the flatten step after them).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "scan_params.hip.h"
#include "unionfind.hip.h"

namespace isk {

__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ULL;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ULL;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBULL;
    return x ^ (x >> 31);
}

struct FillParams {
    uint64_t* col[4];
    uint64_t* keys;
    uint64_t dst_row;      // first destination row in the segment
    uint64_t n;
    uint64_t seed, first_row, key_base;
    uint32_t W, KW;
    uint64_t mask_last;    // codes shorter than W words keep zero padding
};
__global__ __launch_bounds__(BLOCK) void fill_kernel(const FillParams p) {
    for (uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; i < p.n; i += (uint64_t)gridDim.x * BLOCK) {
        const uint64_t src = p.first_row + i;
        for (uint32_t w = 0; w < p.W; ++w) {
            uint64_t v = splitmix64(p.seed + 4 * src + w);
            if (w == p.W - 1) v &= p.mask_last;
            p.col[w][p.dst_row + i] = v;
        }
        if (p.KW == 2) { p.keys[2 * (p.dst_row + i)] = 0; p.keys[2 * (p.dst_row + i) + 1] = p.key_base + src; }
        else p.keys[p.dst_row + i] = p.key_base + src;
    }
}

// sequential row moves (swap-with-last removal): lane c owns column c for every move, in order
struct MoveParams {
    uint64_t* col[4];
    uint64_t* keys;
    const uint64_t* moves;   // [n_moves][2] = (dst, src)
    uint64_t n_moves;
    uint32_t W, KW;
};
__global__ void move_rows_kernel(const MoveParams p) {
    const uint32_t c = threadIdx.x;
    if (c < p.W) {
        uint64_t* col = p.col[c];
        for (uint64_t m = 0; m < p.n_moves; ++m) col[p.moves[2 * m]] = col[p.moves[2 * m + 1]];
    } else if (c < p.W + p.KW) {
        const uint32_t kw = c - p.W;
        for (uint64_t m = 0; m < p.n_moves; ++m) p.keys[p.moves[2 * m] * p.KW + kw] = p.keys[p.moves[2 * m + 1] * p.KW + kw];
    }
}

struct GatherParams {
    const uint64_t* col[4];
    const uint64_t* rows;    // [n]
    uint64_t* out;           // [n][W]
    uint64_t n;
    uint32_t W;
};
__global__ __launch_bounds__(BLOCK) void gather_rows_kernel(const GatherParams p) {
    for (uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; i < p.n; i += (uint64_t)gridDim.x * BLOCK)
        for (uint32_t w = 0; w < p.W; ++w) p.out[i * p.W + w] = p.col[w][p.rows[i]];
}

// ingest: rows handed over row-major [n][MW] -> the segment's word columns (the last kept word masked to the code length)
struct SplitParams {
    uint64_t* col[4];
    const uint64_t* rows;    // [n][MW]
    uint64_t dst_row, n;
    uint32_t W, MW;
    uint64_t mask_last;
};
__global__ __launch_bounds__(BLOCK) void split_rows_kernel(const SplitParams p) {
    for (uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; i < p.n; i += (uint64_t)gridDim.x * BLOCK)
        for (uint32_t w = 0; w < p.W; ++w) {
            uint64_t v = p.rows[i * p.MW + w];
            if (w == p.W - 1) v &= p.mask_last;
            p.col[w][p.dst_row + i] = v;
        }
}

// add_columns: the last word column of rows handed over word-major, masked to the code length where it lies
__global__ __launch_bounds__(BLOCK) void mask_column_kernel(uint64_t* col, uint64_t n, uint64_t mask) {
    for (uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * BLOCK) col[i] &= mask;
}

// out[i] = src[rows[i]]  (document-frequency column lookups)
__global__ __launch_bounds__(BLOCK) void gather_u32_kernel(const uint32_t* src, const uint64_t* rows, uint32_t* out, uint64_t n) {
    for (uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (uint64_t)gridDim.x * BLOCK) out[i] = src[rows[i]];
}

// isccsearch_join_components: out[i] = the label of row i of a segment -- live_labels[r] where live_keys[r] (strictly ascending) is
// the row's key, 0xFFFFFFFF (no label) where the key is not listed.  64-bit keys.  isccsearch_join_degrees / _within_live: live_labels
// NULL, the label is r itself (n_live < 2^32 - 1 is checked by the host).
struct LabelParams {
    const uint64_t* keys;          // the segment's key column [n]
    const uint64_t* live_keys;     // [n_live]
    const uint32_t* live_labels;   // [n_live], or NULL: the key's index
    uint32_t* out;                 // [n]
    uint64_t n, n_live;
};
__global__ __launch_bounds__(BLOCK) void label_rows_kernel(const LabelParams p) {
    for (uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; i < p.n; i += (uint64_t)gridDim.x * BLOCK) {
        const uint64_t key = p.keys[i];
        uint64_t lo = 0, hi = p.n_live;            // the first listed key >= key lies in [lo, hi]
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (p.live_keys[mid] < key) lo = mid + 1;
            else hi = mid;
        }
        p.out[i] = lo < p.n_live && p.live_keys[lo] == key ? (p.live_labels ? p.live_labels[lo] : (uint32_t)lo) : UF_NONE;
    }
}

// isccsearch_join_overlaps: the label of row i of a simprint segment (128-bit keys: the asset is the FIRST key word) -- the rank of
// its asset in asset_keys (strictly ascending), the search of label_rows_kernel at stride 2.  0xFFFFFFFF (no label) where the asset
// is not listed, and where the row is a stop chunk: its entry in the segment's frequency column exceeds max_doc_freq (freq NULL:
// no cut).  Every LISTED row, stop chunks included, adds 1 to chunks[rank]; *live_rows counts the listed rows, *stop_chunks the
// stop chunks among them (one atomic per wave each).  Integer atomics: the result does not depend on their order.
// isccsearch_join_overlaps_between runs it once per table, each with its own two counters; side_bit (0, or LABEL_SIDE_B of join.hip.h
// for table B) is set in every label given.
// Bounds: the row loop runs ceil(n / grid size) trips, the search at most 64 (hi - lo halves; n_assets < 2^32 is checked by the host).
struct OverlapLabelParams {
    const uint64_t* keys;          // the segment's key column [n][2]
    const uint64_t* asset_keys;    // [n_assets]
    const uint32_t* freq;          // the segment's frequency column [n], or NULL
    uint32_t* out;                 // [n]
    uint32_t* chunks;              // [n_assets], zeroed
    unsigned long long* live_rows;    // this side's two counters among the call's
    unsigned long long* stop_chunks;
    uint64_t n, n_assets;
    uint32_t max_doc_freq;
    uint32_t side_bit;             // set in every label given (ranks do not reach it: the host bounds n_assets)
};
__global__ __launch_bounds__(BLOCK) void label_chunks_kernel(const OverlapLabelParams p) {
    uint32_t live = 0, stop = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; i < p.n; i += (uint64_t)gridDim.x * BLOCK) {
        const uint64_t key = p.keys[2 * i];
        uint64_t lo = 0, hi = p.n_assets;          // the first listed asset >= key lies in [lo, hi]
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (p.asset_keys[mid] < key) lo = mid + 1;
            else hi = mid;
        }
        // (the label is SELECTED at the end, not assigned inside the branches: hipcc's code for the branchy form kept the rank in the
        //  register the frequency load overwrites, and every row lost its label whenever a frequency column was given)
        const bool listed = lo < p.n_assets && p.asset_keys[lo] == key;
        const uint32_t rank = (uint32_t)lo;
        bool is_stop = false;
        if (listed) {
            atomicAdd(p.chunks + rank, 1u);
            if (p.freq) is_stop = p.freq[i] > p.max_doc_freq;
        }
        live += listed ? 1u : 0u;
        stop += is_stop ? 1u : 0u;
        p.out[i] = listed && !is_stop ? rank | p.side_bit : UF_NONE;
    }
    // every lane of the block gets here (no lane returns early): the shuffles see whole waves
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        live += (uint32_t)__shfl_xor((int)live, d, 64);
        stop += (uint32_t)__shfl_xor((int)stop, d, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        if (live) atomicAdd(p.live_rows, (unsigned long long)live);
        if (stop) atomicAdd(p.stop_chunks, (unsigned long long)stop);
    }
}

// after the last join launch of isccsearch_join_components: every label's entry becomes its component's smallest label
// (uf_flatten of unionfind.hip.h; the caller has checked parent[i] <= i, which bounds every walk)
__global__ __launch_bounds__(BLOCK) void flatten_kernel(uint32_t* parent, uint32_t n_labels) {
    for (uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; i < n_labels; i += (uint64_t)gridDim.x * BLOCK) uf_flatten(parent, (uint32_t)i);
}

}  // namespace isk
