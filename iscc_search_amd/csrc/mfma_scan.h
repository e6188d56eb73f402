// mfma_scan.h -- host interface of mfma_scan.hip (the matrix-core form of the collect scan: FP4 products, f32 sums).
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "scan_params.hip.h"

namespace isk {

constexpr int MFMA_MAX_LDS = 48 * 1024;   // a chunk needs <= 40 KB of dynamic LDS: within the default limit, nothing to configure

// query groups (32 queries each; an even number unless `pack`) one block keeps in LDS for W compared words
uint32_t mfma_groups_per_chunk(int W, uint32_t nq_pad, bool pack);
size_t mfma_lds_bytes(int W, uint32_t groups);
uint32_t mfma_waves_per_block();
// pack: 64-bit codes on mfma_pack_kernel (two row tiles per accumulator, packed f16 fold); the batch must not hold an all-zero query
// pack3: 64-bit codes on mfma_pack3_kernel (three row tiles per accumulator, OR fold of indicator bits) -- chunks of more than
// four groups only (mfma_pack3_fits); smaller chunks keep mfma_pack_kernel
bool mfma_pack3_fits(uint32_t groups);
uint32_t mfma_rows_per_wave_step(int W, bool pack, bool pack3 = false);   // rows a wave takes per step (192 pack3, 128 packed, else 64)
uint32_t mfma_blocks_per_cu(int W, uint32_t groups, bool pack);   // resident blocks per CU (LDS and register limits)
// grid = (blocks_x, chunks of groups * 32 queries); returns 0 or a hipError_t when the chunk would not fit (check
// hipGetLastError() for the launch itself, as with every other kernel)
int launch_mfma_scan(int W, int mode, bool pack, uint32_t blocks_x, uint32_t groups, hipStream_t st, const ScanParams& p, bool pack3 = false);

// ---- the joins on the matrix cores (mfma_join_kernel.hip.h): a block HOLDS a chunk of `groups` * 32 rows of one segment in LDS and
// streams the other segment, 64 rows per wave and step
struct JoinEmit;                  // join.hip.h: what only the emit path reads
enum class JoinForm : int;        // join.hip.h: what a join leaves behind for its pairs (PAIRS, LINK, OVERLAP, DEGREE, LIVE)
struct MfmaJoinParams {
    const uint64_t* col_q[4];     // the held segment's columns (word-major); JoinEmit::keys_a are its keys
    const uint64_t* col_s[4];     // the streamed segment's; JoinEmit::keys_b
    const JoinEmit* e;
    uint64_t n_q, n_s;            // rows of the two segments
    uint64_t chunk_base;          // blockIdx.y counts chunks from this one (a launch takes at most MFMA_JOIN_MAX_CHUNKS)
    uint32_t mask_lo, mask_hi;    // mask of the last compared word
    uint32_t tau, same;           // same: both are ONE segment -- only streamed row > held row is a pair
};
constexpr uint32_t MFMA_JOIN_WAVES = 4;             // waves per block (MBLOCK / 64)
constexpr uint32_t MFMA_JOIN_STEP_ROWS = 64;        // streamed rows per wave and step
constexpr uint32_t MFMA_JOIN_STEPS_PER_WAVE = 16;   // steps a wave runs per chunk, so that the chunk's expansion in the prologue amortises
constexpr uint32_t MFMA_JOIN_MAX_BLOCKS_X = 1024;   // ... more, once the streamed segment needs more blocks than this (from 1 Mi rows)
constexpr uint32_t MFMA_JOIN_MAX_CHUNKS = 8192;     // chunks per launch (grid.y); longer segments take several launches
// blocks of a chunk that run steps when `steps` of them are left to it (the self-join: fewer for a chunk late in the segment);
// with blocks_x = the grid's width, also the grid rule itself
__host__ __device__ inline uint32_t mfma_join_live_blocks(uint64_t steps, uint32_t blocks_x) {
    const uint64_t per_block = (uint64_t)MFMA_JOIN_WAVES * MFMA_JOIN_STEPS_PER_WAVE;
    const uint64_t want = (steps + per_block - 1) / per_block;
    return want < blocks_x ? (uint32_t)want : blocks_x;
}
inline uint32_t mfma_join_blocks_x(uint64_t n_streamed) {
    return mfma_join_live_blocks((n_streamed + MFMA_JOIN_STEP_ROWS - 1) / MFMA_JOIN_STEP_ROWS, MFMA_JOIN_MAX_BLOCKS_X);
}
// groups of the held segment (n_held rows) per chunk, and the chunk's LDS image: those of mfma_groups_per_chunk(W, n_held, false) and
// mfma_lds_bytes for every form but DEGREE, whose image carries 4 bytes more per held row (its LDS counters) and whose chunk is as many
// groups fewer as that takes to fit MFMA_MAX_LDS (64-bit codes: 30 groups for 32)
uint32_t mfma_join_groups_per_chunk(int W, uint64_t n_held, JoinForm form);
size_t mfma_join_lds_bytes(int W, uint32_t groups, JoinForm form);
// grid = (blocks_x, chunks of `groups` = mfma_join_groups_per_chunk groups); p.chunk_base names the first of them.  Returns 0 or a hipError_t as launch_mfma_scan does
// (form, cross): the emit path of join.hip.h; a combination that join_form_exists does not list is refused like a chunk that does not fit
int launch_mfma_join(int W, JoinForm form, bool cross, uint32_t blocks_x, uint32_t chunks, uint32_t groups, hipStream_t st, const MfmaJoinParams& p);

}  // namespace isk
