// Segments: the chunk pairs of a self-join of a simprint table, or of the cross join of two, turned into aligned runs per pair of
// assets.  The stage has a SOURCE side and a DESTINATION side (Side of segments.h): the self-join passes its one table twice, the
// cross join passes table_a and table_b.
//
//   1. ordinals, per table: merge sort (rocPRIM) of the segment's keys (asset, offset << 32 | size) with the row numbers as values; a
//      row's ordinal is its sorted position minus the position of the first row of its asset (a lower-bound search).  Keys are unique
//      in a table, so the sorted array does not depend on the order of the rows.  Two tables: the destination side's sorted keys,
//      sorted rows and ordinals lie behind the source side's in the same buffers.
//   2. pairs: slots 2s and 2s + 1 of the hit buffer are the two directions of chunk pair s.  One table: it is oriented so that
//      src < dst.  Two tables: the hit whose src lacks isk::LABEL_SIDE_B is table_a's, whichever slot it is in (that depends on which
//      table the join held), and src is ALWAYS the label of table_a, dst that of table_b without the bit.  Keyed by {src, dst,
//      diagonal = o_dst - o_src, o_src}; an unused slot (all ones) stays all ones.
//   3. runs: merge sort by that key, unused slots last.  A pair is a run head when its predecessor is not (same src, same dst, same
//      diagonal, o_src - 1); the heads are counted into run numbers (inclusive scan) and the pairs reduced by run number: lengths and
//      distances add up, the first and the last pair are those of the smallest and the largest o_src.  All of it in integers, by an
//      operation that is commutative as well as associative: no order of additions changes a result.
//   4. records: the byte ranges are gathered from the key columns through the rows of a run's first and last pair, the _src fields
//      from the source side's column, the _dst fields from the destination side's.
//
// Nothing here waits for the device: the caller reads the segment count behind its one synchronisation.
#include <cstring>   // rocPRIM's texture iterator calls memset without including it

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include <cerrno>
#include <cstdio>

#include "segments.h"

namespace isksg {
namespace {

constexpr int BLOCK = 256;
constexpr uint32_t DIAGONAL_ZERO = 0x80000000u;

struct RowKeyLess {
    __host__ __device__ bool operator()(const RowKey& a, const RowKey& b) const {
        if (a.asset != b.asset) return a.asset < b.asset;
        return a.place < b.place;
    }
};

struct PairLess {
    __host__ __device__ bool operator()(const PairKey& a, const PairKey& b) const {
        if (a.src != b.src) return a.src < b.src;
        if (a.dst != b.dst) return a.dst < b.dst;
        if (a.diagonal != b.diagonal) return a.diagonal < b.diagonal;
        if (a.o_src != b.o_src) return a.o_src < b.o_src;
        if (a.row_src != b.row_src) return a.row_src < b.row_src;      // (no two pairs are equal so far: a row has one ordinal)
        return a.row_dst < b.row_dst;
    }
};

struct MergeRuns {
    __host__ __device__ Run operator()(const Run& a, const Run& b) const {
        Run r = a;                      // (src, dst and the diagonal: those of the run, the same in a and b)
        if (b.first_src < a.first_src) { r.first_src = b.first_src; r.first_dst = b.first_dst; r.row_first_src = b.row_first_src; r.row_first_dst = b.row_first_dst; }
        if (b.last_src > a.last_src) { r.last_src = b.last_src; r.row_last_src = b.row_last_src; r.row_last_dst = b.row_last_dst; }
        r.length = a.length + b.length;
        r.sum_hamming = a.sum_hamming + b.sum_hamming;
        return r;
    }
};

// every grid-stride loop below runs ceil(count / grid size) trips over a count the host checked
__host__ uint32_t grid_for(uint64_t count) { return (uint32_t)((count + BLOCK - 1) / BLOCK < 65536 ? (count + BLOCK - 1) / BLOCK : 65536); }

// sorted position p holds row sorted_rows[p]: its ordinal is p minus the first position of its asset
__global__ __launch_bounds__(BLOCK) void ordinals_kernel(const RowKey* sorted_keys, const uint32_t* sorted_rows, uint32_t* ordinals, uint64_t n) {
    for (uint64_t p = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; p < n; p += (uint64_t)gridDim.x * BLOCK) {
        const uint64_t asset = sorted_keys[p].asset;
        uint64_t lo = 0, hi = p;
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (sorted_keys[mid].asset < asset) lo = mid + 1;
            else hi = mid;
        }
        const uint32_t row = sorted_rows[p];
        if (row < n) ordinals[row] = (uint32_t)(p - lo);
    }
}

// chunk pair s of the hit buffer as its key; a row indexes its side's ordinals only when it is below that side's row count.
// CROSS: the source side is table_a, whose labels lack SIDE_B; else both sides are one table and the smaller label is the source.
template <bool CROSS>
__global__ __launch_bounds__(BLOCK) void pairs_kernel(const uint4* hits, const uint32_t* ordinals_src, uint64_t n_src, const uint32_t* ordinals_dst,
                                                      uint64_t n_dst, uint4* pairs, uint64_t capacity) {
    for (uint64_t s = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; s < capacity; s += (uint64_t)gridDim.x * BLOCK) {
        const uint4 a = hits[2 * s], b = hits[2 * s + 1];              // (la, lb, row_i, h) and (lb, la, row_j, h)
        uint4 key = make_uint4(~0u, ~0u, ~0u, ~0u), payload = key;
        if (a.x != iskov::NO_ASSET) {
            const bool swap = CROSS ? (a.x & SIDE_B) != 0 : a.x > a.y;
            const uint32_t row_src = swap ? b.z : a.z, row_dst = swap ? a.z : b.z;
            if (row_src < n_src && row_dst < n_dst) {
                const uint32_t o_src = ordinals_src[row_src], o_dst = ordinals_dst[row_dst];
                const uint32_t src = swap ? a.y : a.x, dst = swap ? a.x : a.y;
                key = make_uint4(src, CROSS ? dst & ~SIDE_B : dst, o_dst - o_src + DIAGONAL_ZERO, o_src);
                payload = make_uint4(row_src, row_dst, a.w, 0u);
            }
        }
        pairs[2 * s] = key;
        pairs[2 * s + 1] = payload;
    }
}

// sorted pair i as a run of its own, and whether it heads a run; the unused slots behind the pairs make ONE run
__global__ __launch_bounds__(BLOCK) void heads_kernel(const PairKey* sorted, uint32_t* heads, Run* marks, uint64_t capacity) {
    for (uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; i < capacity; i += (uint64_t)gridDim.x * BLOCK) {
        const PairKey p = sorted[i];
        bool head = true;
        if (i > 0) {
            const PairKey q = sorted[i - 1];
            if (p.src == iskov::NO_ASSET) head = q.src != iskov::NO_ASSET;
            else head = q.src != p.src || q.dst != p.dst || q.diagonal != p.diagonal || q.o_src + 1 != p.o_src;
        }
        Run r;
        r.src = p.src;
        r.dst = p.dst;
        r.first_src = r.last_src = p.o_src;
        r.first_dst = p.o_src + (p.diagonal - DIAGONAL_ZERO);
        r.length = 1;
        r.sum_hamming = p.hamming;
        r.row_first_src = r.row_last_src = p.row_src;
        r.row_first_dst = r.row_last_dst = p.row_dst;
        r.reserved = 0;
        heads[i] = head ? 1u : 0u;
        marks[i] = r;
    }
}

// reduced run i becomes its record in place: the byte ranges come from the two sides' key columns (a row indexes its side's column
// only when it is below that side's row count)
__global__ __launch_bounds__(BLOCK) void records_kernel(Run* runs, const RowKey* keys_src, uint64_t n_src, const RowKey* keys_dst, uint64_t n_dst,
                                                        const unsigned long long* n_runs, uint64_t capacity) {
    const uint64_t count = *n_runs < capacity ? *n_runs : capacity;
    for (uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; i < count; i += (uint64_t)gridDim.x * BLOCK) {
        const Run r = runs[i];
        if (r.src == iskov::NO_ASSET || r.row_first_src >= n_src || r.row_first_dst >= n_dst || r.row_last_src >= n_src || r.row_last_dst >= n_dst) continue;
        const uint64_t first_src = keys_src[r.row_first_src].place, first_dst = keys_dst[r.row_first_dst].place;
        const uint64_t last_src = keys_src[r.row_last_src].place, last_dst = keys_dst[r.row_last_dst].place;
        const uint64_t end_src = (last_src >> 32) + (uint32_t)last_src, end_dst = (last_dst >> 32) + (uint32_t)last_dst;
        uint4* const out = reinterpret_cast<uint4*>(runs + i);         // isccsearch_segment, 48 bytes
        out[0] = make_uint4(r.src, r.dst, r.first_src, r.first_dst);
        out[1] = make_uint4(r.length, r.sum_hamming, (uint32_t)(first_src >> 32), (uint32_t)(first_dst >> 32));
        out[2] = make_uint4((uint32_t)end_src, (uint32_t)(end_src >> 32), (uint32_t)end_dst, (uint32_t)(end_dst >> 32));
    }
}

int failed(std::string* err, const char* what, hipError_t e) {
    (void)hipGetLastError();   // do not leave the code behind for an unrelated later launch check
    if (err) {
        char buf[256];
        snprintf(buf, sizeof buf, "segments: %s: %s", what, hipGetErrorString(e));
        *err = buf;
    }
    return e == hipErrorOutOfMemory ? -ENOMEM : -EIO;
}

#define SGOK(expr, what)                                   \
    do {                                                   \
        hipError_t e_ = (expr);                            \
        if (e_ != hipSuccess) return failed(err, what, e_); \
    } while (0)

// rows: the larger of the two tables' key sorts (one table: its one sort)
struct Sizes { size_t rows = 0, pairs = 0, scan = 0, reduce = 0; };

int sizes(uint64_t n_src, uint64_t n_dst, uint64_t capacity, Sizes& s, std::string* err) {
    RowKey* k = nullptr;
    uint32_t* u = nullptr;
    PairKey* p = nullptr;
    Run* r = nullptr;
    unsigned long long* c = nullptr;
    size_t rows_dst = 0;
    SGOK(rocprim::merge_sort(nullptr, s.rows, k, k, rocprim::counting_iterator<uint32_t>(0), u, n_src, RowKeyLess(), (hipStream_t) nullptr), "merge_sort(rows, size)");
    if (n_dst != n_src) {
        SGOK(rocprim::merge_sort(nullptr, rows_dst, k, k, rocprim::counting_iterator<uint32_t>(0), u, n_dst, RowKeyLess(), (hipStream_t) nullptr), "merge_sort(rows, size)");
        if (rows_dst > s.rows) s.rows = rows_dst;
    }
    SGOK(rocprim::merge_sort(nullptr, s.pairs, p, p, capacity, PairLess(), (hipStream_t) nullptr), "merge_sort(pairs, size)");
    SGOK(rocprim::inclusive_scan(nullptr, s.scan, u, u, capacity, rocprim::plus<uint32_t>(), (hipStream_t) nullptr), "inclusive_scan(size)");
    SGOK(rocprim::reduce_by_key(nullptr, s.reduce, u, r, capacity, u, r, c, MergeRuns(), rocprim::equal_to<uint32_t>(), (hipStream_t) nullptr),
         "reduce_by_key(size)");
    return 0;
}

// one table's ordinals: sorted_keys[n], sorted_rows[n] and ordinals[n] are that table's part of the scratch
int ordinals_of(const Side& side, RowKey* sorted_keys, uint32_t* sorted_rows, uint32_t* ordinals, void* temp, size_t temp_bytes, hipStream_t stream,
                std::string* err) {
    SGOK(rocprim::merge_sort(temp, temp_bytes, side.keys, sorted_keys, rocprim::counting_iterator<uint32_t>(0), sorted_rows, side.n, RowKeyLess(), stream),
         "merge_sort(rows)");
    hipLaunchKernelGGL(ordinals_kernel, dim3(grid_for(side.n)), dim3(BLOCK), 0, stream, sorted_keys, sorted_rows, ordinals, side.n);
    SGOK(hipGetLastError(), "kernel launch");
    return 0;
}

}  // namespace

int locate_temp_bytes(uint64_t n_src, uint64_t n_dst, uint64_t capacity, size_t* bytes, std::string* err) {
    Sizes s;
    const int rc = sizes(n_src, n_dst, capacity, s, err);
    if (rc) return rc;
    size_t most = s.rows;
    if (s.pairs > most) most = s.pairs;
    if (s.scan > most) most = s.scan;
    if (s.reduce > most) most = s.reduce;
    *bytes = most;
    return 0;
}

int locate(const Side& src, const Side& dst, const iskov::Hit* hits, uint64_t capacity, RowKey* sorted_keys, uint32_t* sorted_rows,
           uint32_t* ordinals, PairKey* pairs, Run* runs, unsigned long long* n_segments, void* temp, size_t temp_bytes,
           hipStream_t stream, std::string* err) {
    if (src.n == 0 || dst.n == 0 || capacity == 0) return 0;
    const bool cross = src.keys != dst.keys;
    if (!cross && src.n != dst.n) {
        if (err) *err = "segments: one key column given with two row counts";
        return -EINVAL;
    }
    Sizes s;
    int rc = sizes(src.n, dst.n, capacity, s, err);
    if (rc) return rc;
    if (s.rows > temp_bytes || s.pairs > temp_bytes || s.scan > temp_bytes || s.reduce > temp_bytes) {
        if (err) *err = "segments: the temporary storage is smaller than locate_temp_bytes() asked for";
        return -EINVAL;
    }
    // 1. ordinals: one sort per table, the destination side's scratch behind the source side's (one table: the one part serves both)
    uint32_t* const ordinals_dst = cross ? ordinals + src.n : ordinals;
    if ((rc = ordinals_of(src, sorted_keys, sorted_rows, ordinals, temp, s.rows, stream, err))) return rc;
    if (cross && (rc = ordinals_of(dst, sorted_keys + src.n, sorted_rows + src.n, ordinals_dst, temp, s.rows, stream, err))) return rc;
    // 2. pairs
    PairKey* const sorted = pairs + capacity;
    if (cross)
        hipLaunchKernelGGL(pairs_kernel<true>, dim3(grid_for(capacity)), dim3(BLOCK), 0, stream, reinterpret_cast<const uint4*>(hits), ordinals, src.n,
                           ordinals_dst, dst.n, reinterpret_cast<uint4*>(pairs), capacity);
    else
        hipLaunchKernelGGL(pairs_kernel<false>, dim3(grid_for(capacity)), dim3(BLOCK), 0, stream, reinterpret_cast<const uint4*>(hits), ordinals, src.n,
                           ordinals_dst, dst.n, reinterpret_cast<uint4*>(pairs), capacity);
    SGOK(hipGetLastError(), "kernel launch");
    // 3. runs.  Once sorted, the keyed pairs are dead: their buffer (32 bytes per pair) takes the head flags, the run numbers and the
    // unique run numbers of the reduction, which nothing reads (4 bytes per pair each)
    SGOK(rocprim::merge_sort(temp, s.pairs, pairs, sorted, capacity, PairLess(), stream), "merge_sort(pairs)");
    uint32_t* const heads = reinterpret_cast<uint32_t*>(pairs);
    uint32_t* const numbers = heads + capacity;
    uint32_t* const unique = numbers + capacity;
    Run* const reduced = runs + capacity;
    hipLaunchKernelGGL(heads_kernel, dim3(grid_for(capacity)), dim3(BLOCK), 0, stream, sorted, heads, runs, capacity);
    SGOK(hipGetLastError(), "kernel launch");
    SGOK(rocprim::inclusive_scan(temp, s.scan, heads, numbers, capacity, rocprim::plus<uint32_t>(), stream), "inclusive_scan");
    SGOK(rocprim::reduce_by_key(temp, s.reduce, numbers, runs, capacity, unique, reduced, n_segments, MergeRuns(), rocprim::equal_to<uint32_t>(), stream),
         "reduce_by_key");
    // 4. records
    hipLaunchKernelGGL(records_kernel, dim3(grid_for(capacity)), dim3(BLOCK), 0, stream, reduced, src.keys, src.n, dst.keys, dst.n, n_segments, capacity);
    SGOK(hipGetLastError(), "kernel launch");
    return 0;
}

}  // namespace isksg
