// Overlap records: sort the directed hits of a self-join of a simprint table, then reduce them per ordered pair of assets.
//
//   1. merge sort (rocPRIM) of the hits by (src, dst, row, hamming), unused slots (all ones) last.  Equal hits are equal in every
//      field, so the sorted array does not depend on the order in which the join kernels appended.
//   2. mark: hit i becomes a one-hit record {src, dst, matched, 0, sum_hamming, chunk_pairs = 1}; the FIRST hit of its
//      (src, dst, row) -- the one with the smallest distance -- has matched = 1 and sum_hamming = its distance, the others 0 and 0.
//   3. reduce by (src, dst) (rocPRIM): the fields add up.  All of them are integers: no order of additions changes a result.
//
// Nothing here waits for the device: the caller reads the record count behind its one synchronisation.
#include <cstring>   // rocPRIM's texture iterator calls memset without including it

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include <cerrno>
#include <cstdio>

#include "overlap.h"

namespace iskov {
namespace {

constexpr int BLOCK = 256;

struct HitLess {
    __host__ __device__ bool operator()(const Hit& a, const Hit& b) const {
        if (a.src != b.src) return a.src < b.src;
        if (a.dst != b.dst) return a.dst < b.dst;
        if (a.row != b.row) return a.row < b.row;
        return a.hamming < b.hamming;
    }
};

struct AddRecords {
    __host__ __device__ isccsearch_overlap operator()(const isccsearch_overlap& a, const isccsearch_overlap& b) const {
        isccsearch_overlap r = a;       // (src, dst: those of the run, the same in a and b)
        r.matched += b.matched;
        r.sum_hamming += b.sum_hamming;
        r.chunk_pairs += b.chunk_pairs;
        return r;
    }
};

// the grid-stride loop runs ceil(m / grid size) trips
__global__ __launch_bounds__(BLOCK) void mark_kernel(const Hit* sorted, uint64_t* keys, isccsearch_overlap* marks, uint64_t m) {
    for (uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; i < m; i += (uint64_t)gridDim.x * BLOCK) {
        const Hit h = sorted[i];
        bool first = true;
        if (i > 0) {
            const Hit g = sorted[i - 1];
            first = g.src != h.src || g.dst != h.dst || g.row != h.row;
        }
        isccsearch_overlap r;
        r.src = h.src;
        r.dst = h.dst;
        r.matched = first ? 1u : 0u;
        r.reserved = 0;
        r.sum_hamming = first ? h.hamming : 0u;
        r.chunk_pairs = 1;
        keys[i] = (uint64_t)h.src << 32 | h.dst;
        marks[i] = r;
    }
}

int failed(std::string* err, const char* what, hipError_t e) {
    (void)hipGetLastError();   // do not leave the code behind for an unrelated later launch check
    if (err) {
        char buf[256];
        snprintf(buf, sizeof buf, "overlap records: %s: %s", what, hipGetErrorString(e));
        *err = buf;
    }
    return e == hipErrorOutOfMemory ? -ENOMEM : -EIO;
}

#define OVOK(expr, what)                                   \
    do {                                                   \
        hipError_t e_ = (expr);                            \
        if (e_ != hipSuccess) return failed(err, what, e_); \
    } while (0)

int sizes(uint64_t m, size_t& sort_bytes, size_t& reduce_bytes, std::string* err) {
    Hit* h = nullptr;
    uint64_t* k = nullptr;
    isccsearch_overlap* r = nullptr;
    unsigned long long* c = nullptr;
    OVOK(rocprim::merge_sort(nullptr, sort_bytes, h, h, m, HitLess(), (hipStream_t) nullptr), "merge_sort(size)");
    OVOK(rocprim::reduce_by_key(nullptr, reduce_bytes, k, r, m, k, r, c, AddRecords(), rocprim::equal_to<uint64_t>(), (hipStream_t) nullptr),
         "reduce_by_key(size)");
    return 0;
}

}  // namespace

int aggregate_temp_bytes(uint64_t m, size_t* bytes, std::string* err) {
    size_t a = 0, b = 0;
    const int rc = sizes(m, a, b, err);
    if (rc) return rc;
    *bytes = a > b ? a : b;
    return 0;
}

int aggregate(Hit* hits, Hit* sorted, isccsearch_overlap* marks, isccsearch_overlap* records, unsigned long long* n_records, uint64_t m,
              void* temp, size_t temp_bytes, hipStream_t stream, std::string* err) {
    if (m == 0) return 0;
    size_t sort_bytes = 0, reduce_bytes = 0;
    const int rc = sizes(m, sort_bytes, reduce_bytes, err);
    if (rc) return rc;
    if (sort_bytes > temp_bytes || reduce_bytes > temp_bytes) {
        if (err) *err = "overlap records: the temporary storage is smaller than aggregate_temp_bytes() asked for";
        return -EINVAL;
    }
    OVOK(rocprim::merge_sort(temp, sort_bytes, hits, sorted, m, HitLess(), stream), "merge_sort");
    // once sorted, the unsorted hits are dead: their buffer takes the reduction's keys (8 of its 16 bytes per hit)
    uint64_t* const keys = reinterpret_cast<uint64_t*>(hits);
    const uint32_t grid = (uint32_t)((m + BLOCK - 1) / BLOCK < 65536 ? (m + BLOCK - 1) / BLOCK : 65536);
    hipLaunchKernelGGL(mark_kernel, dim3(grid), dim3(BLOCK), 0, stream, sorted, keys, marks, m);
    OVOK(hipGetLastError(), "kernel launch");
    // the unique keys are not needed (a record carries its src and dst): they overwrite the sorted hits, which nothing reads any more
    OVOK(rocprim::reduce_by_key(temp, reduce_bytes, keys, marks, m, reinterpret_cast<uint64_t*>(sorted), records, n_records, AddRecords(),
                                rocprim::equal_to<uint64_t>(), stream),
         "reduce_by_key");
    return 0;
}

}  // namespace iskov
