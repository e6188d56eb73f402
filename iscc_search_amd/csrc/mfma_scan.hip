// mfma_scan.hip -- the collect scan for LARGE query batches on the matrix cores of gfx950 (MI355X).
//
// Same contract as scan_kernel (valu_scan_kernel.hip.h): for every row of [row_begin, n_rows) and every query, append
// (hamming, row) to the query's candidate list when hamming over the compared prefix <= tau_q
// (reference call sites: iscc_search/indexes/usearch/index.py:2037, iscc_search/indexes/simprint/usearch_core.py:165;
// metric: docs/explanation/similarity-search.md:24-29).  What differs is the arithmetic:
//
//   hamming(row, q) = popc(q) + dot(row bits as 0/1, query bits as +1/-1)            (exact small integers)
//
// so the (rows x queries x bits) work is a dense contraction.  The XOR + popcount kernel needs 4.5 VALU instructions per
// (row, query, 64-bit word), each issuing at one wave64 per ~4 cycles per SIMD, and is VALU-bound from ~11 queries per
// pass on.  Here the products run on the matrix pipe in its cheapest format: FP4 (e2m1: 0x2 = +1,
// 0xA = -1, 0x0 = 0) through v_mfma_f32_32x32x64_f8f6f4 (the unscaled form: block scales 2^0) -- ONE instruction (32 cycles)
// per 32 rows x 32 queries x 64 bits, f32 accumulation, exact because every partial sum is an integer of magnitude
// <= 256.  (The int8 form, v_mfma_i32_32x32x32_i8, needs two instructions of the same length per word and measured 1.44x
// slower: profiles/r02_proto_mfma_scan.txt.)
//
// A wave owns T = 2 tiles of 32 rows: each lane expands ITS 32 bits of one row per word into 32 nibbles (4 VGPRs, the A
// operand), once per step, and then walks every query group of the block's chunk.  A group is 32 queries pre-expanded to
// +1/-1 nibbles in LDS (one ds_read_b128 per lane and word); W MFMAs per tile give the 32 x 32 dot products; a lane's 16
// results per tile all belong to ONE query (C/D column = lane & 31), so 16 v_min3_f32 fold the two tiles and one compare
// against thr_q = tau_q - popc(q) decides whether the lane enters the rare emit path.  Masked prefixes (NPHD between codes
// of different lengths) cost nothing: the query nibbles beyond the prefix are 0.
//
// What bounds it is vector ISSUE: the fold (16 values per lane per 1 024 pairs, two per v_min3) and the MFMAs share the
// SIMD's issue port (~50 cycles per 1 024 pairs and word against 32 of matrix-pipe time); the XOR + popcount kernel needs
// ~290.  Rows cross the memory system once per chunk of up to 1 024 queries.  Measured numbers: DESIGN.md section 4.
//
// Modes (scan_params.hip.h): MODE_COLLECT (range-limited searches: a given threshold), MODE_BOTH / MODE_STRETCH (the threshold
// levels and the collect pass of the level design: append + histogram, picks between launches) and MODE_SELF -- ONE launch
// over all rows whose thresholds tighten themselves: the live thresholds are re-read from global memory once per step, every
// candidate is counted per distance, and the lane that proves "k rows within t" lowers the threshold (see Pending, emit_self,
// lower_threshold).  The default for k <= 512.
//
// The joins (isccsearch_join_within / _between) run the same arithmetic under ONE fixed threshold, with a chunk of a table's own rows
// where the queries are: mfma_join_kernel.hip.h, launch_mfma_join.
//
// Built with -mllvm -amdgpu-mfma-vgpr-form=1 -ffinite-math-only: hipcc otherwise puts the accumulators in AGPRs and pays one
// v_accvgpr_read per result before the fold (16 extra VALU instructions per tile and group), and canonicalises the inputs of
// every 2-input fminf (two v_max per group: the values are small integers, never NaN).
#include "mfma_scan.h"

#include "mfma_common.hip.h"
#include "mfma_scan_kernel.hip.h"
#include "mfma_pack_kernel.hip.h"
#include "mfma_pack3_kernel.hip.h"
#include "mfma_join_kernel.hip.h"

namespace isk {

template <int DEPTH, int G>
static void launch_pack_depth(int mode, dim3 grid, size_t lds, hipStream_t st, const ScanParams& p, uint32_t groups) {
    with_mode(mode, [&](auto m) { hipLaunchKernelGGL((mfma_pack_kernel<decltype(m)::value, DEPTH, G>), grid, dim3(MBLOCK), lds, st, p, groups); });
}

static int launch_pack(int mode, dim3 grid, size_t lds, hipStream_t st, const ScanParams& p, uint32_t groups, bool pack3) {
    if (pack3 && mfma_pack3_fits(groups)) {
        lds += P3_LDS_EXTRA;
        if (lds > (size_t)MFMA_MAX_LDS) return (int)hipErrorInvalidValue;
        with_mode(mode, [&](auto m) {
            if (groups & 1) hipLaunchKernelGGL((mfma_pack3_kernel<decltype(m)::value, true>), grid, dim3(MBLOCK), lds, st, p, groups);
            else hipLaunchKernelGGL((mfma_pack3_kernel<decltype(m)::value, false>), grid, dim3(MBLOCK), lds, st, p, groups);
        });
        return 0;
    }
    if (lds > (size_t)MFMA_MAX_LDS) return (int)hipErrorInvalidValue;
    static_assert(PK_DEEP_GROUPS == 4, "one case per count");
    switch (groups) {           // up to PK_DEEP_GROUPS groups: one instantiation per count (a step's stages are straight-line code)
        case 1: launch_pack_depth<4, 1>(mode, grid, lds, st, p, groups); break;
        case 2: launch_pack_depth<4, 2>(mode, grid, lds, st, p, groups); break;
        case 3: launch_pack_depth<4, 3>(mode, grid, lds, st, p, groups); break;
        case 4: launch_pack_depth<4, 4>(mode, grid, lds, st, p, groups); break;
        default: launch_pack_depth<1, 0>(mode, grid, lds, st, p, groups);
    }
    return 0;
}

uint32_t mfma_groups_per_chunk(int W, uint32_t nq_pad, bool pack) {
    // LDS per group: 32 queries x (32 * W bytes of +1/-1 nibbles + thr + popc); at most 40 KB per block, four blocks per CU
    static const uint32_t max_groups[5] = {0, 32, 16, 10, 8};
    uint32_t need = (nq_pad + 31) / 32;
    if (pack) return need < 1 ? 1 : (need < max_groups[1] ? need : max_groups[1]);      // mfma_pack_kernel takes any number of groups
    need += need & 1;                         // the pipeline of mfma_scan_kernel walks the groups in pairs
    if (need < 2) need = 2;
    if (need <= max_groups[W]) return need;
    // several chunks: as many as the LDS limit asks for, each as SMALL as that number of chunks allows -- 1 024 queries of 192-bit
    // codes are 32 groups: four chunks of 10 multiplied 40 groups' worth (a fifth of the MFMAs on padding queries: the matrix pipe
    // 0.75 busy for 0.53 of the peak, profiles/r04_pmc_sq_widths.txt), four chunks of 8 multiply 32
    const uint32_t chunks = (need + max_groups[W] - 1) / max_groups[W];
    uint32_t g = (need + chunks - 1) / chunks;
    g += g & 1;
    return g < max_groups[W] ? g : max_groups[W];
}

// B fragments | thresholds | popcounts | the four waves' rings of saved result blocks
size_t mfma_lds_bytes(int W, uint32_t groups) { return (size_t)groups * W * 64 * 16 + (size_t)groups * 32 * 8 + MBLOCK / 64 * PK_RING_ENTRIES * PK_RING_ENTRY_DWORDS * sizeof(uint32_t); }

uint32_t mfma_waves_per_block() { return MBLOCK / 64; }
uint32_t mfma_rows_per_wave_step(int W, bool pack, bool pack3) { return pack3 ? 32u * P3_TILES : pack ? 32u * PK_TILES : 64u; }
bool mfma_pack3_fits(uint32_t groups) { return groups > PK_DEEP_GROUPS; }

uint32_t mfma_blocks_per_cu(int W, uint32_t groups, bool pack) {
    const uint32_t by_lds = (uint32_t)((160u * 1024u) / mfma_lds_bytes(W, groups));
    const uint32_t by_regs = pack || W <= 3 ? 3u : 2u;       // mfma_min_waves, the packed kernels' launch bounds
    return by_lds < by_regs ? (by_lds ? by_lds : 1u) : by_regs;
}

int launch_mfma_scan(int W, int mode, bool pack, uint32_t blocks_x, uint32_t groups, hipStream_t st, const ScanParams& p, bool pack3) {
    const uint32_t chunks = (p.nq_pad + groups * 32 - 1) / (groups * 32);
    const dim3 grid(blocks_x, chunks);
    const size_t lds = mfma_lds_bytes(W, groups);
    if (pack) return W == 1 ? launch_pack(mode, grid, lds, st, p, groups, pack3) : (int)hipErrorInvalidValue;
    // a chunk's LDS image is <= 40 KB: inside the default dynamic-LDS limit, no per-device function attribute to set
    if (lds > (size_t)MFMA_MAX_LDS) return (int)hipErrorInvalidValue;
    with_words(W, [&](auto w) { with_mode(mode, [&](auto m) {
        hipLaunchKernelGGL((mfma_scan_kernel<decltype(w)::value, decltype(m)::value>), grid, dim3(MBLOCK), lds, st, p, groups);
    }); });
    return 0;
}

// the joins' chunk: the scan's image; DEGREE adds a counter per held row behind the rings and gives up pairs of groups until that fits
size_t mfma_join_lds_bytes(int W, uint32_t groups, JoinForm form) {
    return mfma_lds_bytes(W, groups) + (form == JoinForm::DEGREE ? (size_t)groups * 32 * sizeof(uint32_t) : 0);
}
uint32_t mfma_join_groups_per_chunk(int W, uint64_t n_held, JoinForm form) {
    // (any count from 2^20 rows on sizes the chunk alike: as many groups as 40 KB of LDS hold)
    uint32_t g = mfma_groups_per_chunk(W, (uint32_t)(n_held < (1u << 20) ? n_held : 1u << 20), false);
    while (g > 2 && mfma_join_lds_bytes(W, g, form) > (size_t)MFMA_MAX_LDS) g -= 2;
    return g;
}

int launch_mfma_join(int W, JoinForm form, bool cross, uint32_t blocks_x, uint32_t chunks, uint32_t groups, hipStream_t st, const MfmaJoinParams& p) {
    static_assert(MFMA_JOIN_WAVES == MBLOCK / 64, "the grid rule counts the kernel's waves");
    const size_t lds = mfma_join_lds_bytes(W, groups, form);
    // the group pipeline walks pairs of groups; grid.y is 16 bits
    if (W < 1 || W > 4 || lds > (size_t)MFMA_MAX_LDS || groups < 2 || (groups & 1) || !blocks_x || !chunks || chunks > MFMA_JOIN_MAX_CHUNKS) return (int)hipErrorInvalidValue;
    const bool exists = with_join_form(form, cross, [&](auto f) { with_words(W, [&](auto w) {
        hipLaunchKernelGGL((mfma_join_kernel<decltype(w)::value, decltype(f)::form, decltype(f)::cross>), dim3(blocks_x, chunks), dim3(MBLOCK), lds, st, p, groups);
    }); });
    return exists ? 0 : (int)hipErrorInvalidValue;
}

}  // namespace isk
