// mfma_common.hip.h -- what the three matrix-core scan kernels of mfma_scan.hip share: vector types, the block size, the
// accumulator pair of a query group, the layout of the candidate ring, the live-threshold loads and the bit map of the operands.
#pragma once

#include "mfma_scan.h"

#include <hip/hip_runtime.h>

namespace isk {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef int v8i __attribute__((ext_vector_type(8)));
typedef float v16f __attribute__((ext_vector_type(16)));
typedef const __attribute__((address_space(3))) v4i* lds_frag_ptr;
typedef const __attribute__((address_space(3))) float* lds_thr_ptr;

constexpr int MBLOCK = 256;           // 4 waves; a chunk's LDS image is <= 40 KB, so LDS admits four blocks per CU
struct Acc { v16f t[2]; };            // a lane's results of one query group: two accumulators of 16 registers

__device__ __forceinline__ float min3f(float a, float b, float c) { return fminf(fminf(a, b), c); }
// a live threshold as other CUs last wrote it: device-scope load, past this CU's vector cache
__device__ __forceinline__ float live_threshold(const float* addr) {
    return __int_as_float(__hip_atomic_load(reinterpret_cast<const int*>(addr), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}
// ... of the packed kernels (pack_threshold, scan_params.hip.h)
__device__ __forceinline__ uint32_t live_packed(const float* addr) {
    return (uint32_t)__hip_atomic_load(reinterpret_cast<const int*>(addr), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Dword j (0..3) of a 32-bit half: nibble t holds bit j + 4 t.  Rows (A) and queries (B) use the same map, so the k order
// inside the instruction does not matter; lanes 0..31 carry the low half of a word and lanes 32..63 the high half on both sides.
__device__ __forceinline__ uint32_t nibbles(uint32_t x, int j) { return (x >> j) & 0x11111111u; }

// The candidate ring: per wave, the saved result blocks of lanes that hold a hit.  A block, in dwords: the lane's 32 accumulator
// registers | query in chunk + lane half << 16 | the threshold word the fold ran under | pad (144 B).  Every kernel keeps its own
// save_hits / process_ring / pend_complete over it: as shared functions they compiled to different code in kernels that sit at
// their register limit (per-function optimisation before inlining sees through a struct, not through a lambda's captures).
constexpr uint32_t PK_RING_ENTRIES = 8, PK_RING_ENTRY_DWORDS = 36;

}  // namespace isk
