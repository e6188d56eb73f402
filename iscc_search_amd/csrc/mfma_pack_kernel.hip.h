// mfma_pack_kernel.hip.h -- mfma_pack_kernel, 64-bit codes (W = 1): TWO row tiles share ONE accumulator, folded as packed f16
// (included by mfma_scan.hip).
//
// mfma_scan_kernel looks at every (row, query) result once: 15 v_min3_f32 + v_min_f32 + v_cmp per 32 queries x 64 rows,
// 17 vector instructions beside 64 cycles of matrix-pipe time -- vector ISSUE bound it (pipe 0.485 busy, round 2).  Here the
// first MFMA of a tile pair adds its dot products (|d| <= 64) to a constant block C = 2^23 + 0x402000 and the second one is
// the block-SCALED form with scale 2^16 accumulating into the same registers:
//
//     bits(acc) = 0x4B402000 + d1 + 65536 * d2        (an f32 in [2^23, 2^24): ulp = 1, every partial sum an exact integer)
//
// so the LOW half of every register is 0x2000 + d1 and the HIGH half 0x4B40 + d2: positive, normal f16 bit patterns, whose
// order as f16 is their order as integers.  v_pk_minimum3_f16 (new in gfx950) folds FOUR results per instruction, and the
// query's packed threshold T = (first NON-hit pattern of each half) rides in the same fold: "some result <= thr" <=> fold != T.
// A wave owns FOUR tiles (128 rows, two accumulators): 16 fold instructions + 1 compare + 2 scale loads beside four MFMAs
// (128 cycles) -- the matrix pipe is the bound again (prototype: tools/proto_pack_scan.hip, profiles/r03_proto_pack_scan.txt).
//
// The stage (MFMAs of group g + 1 around the fold of group g) is inline assembly in ISSUE ORDER -- MFMA, four fold
// instructions, MFMA, ... -- because hipcc moved the builtin MFMAs across the fold and the hit branch whatever
// sched_barrier said.  hipcc inserts NO hazard nops for assembly, so the distances are kept by construction and counted in
// INSTRUCTIONS (one wait state each, the rule hipcc itself applies; an 8-pass MFMA result may be read by the VALU 11 wait
// states after the MFMA): the first eight fold instructions touch accumulator 0 of the old group only (last written by the
// THIRD MFMA of the previous stage, >= 20 instructions back), accumulator 1 comes after that (>= 20 back as well); a
// v_pk_minimum3_f16 is never followed directly by a consumer of its result (two interleaved chains; s_nop 0 before the join
// and the compare); the first and the last group of a step, whose MFMAs / fold stand alone, are padded with s_nop.
//
// d2 = +64 (query == 0 against a row of all ones) would carry into the exponent and halve the resolution of the low half:
// the host routes a batch holding an all-zero 64-bit query to mfma_scan_kernel (Batch::plan, batch.hip.h).
#pragma once

#include "mfma_common.hip.h"

namespace isk {

constexpr int PK_TILES = 4;                                             // row tiles per wave and step
constexpr uint32_t PK_DEEP_GROUPS = 4;                                  // chunks of up to this many groups (128 queries): one instantiation per count,
                                                                        // four steps of rows in flight, accumulators carried across steps (five and six fit 168 registers no more)
__device__ __forceinline__ uint32_t pkmin3(uint32_t a, uint32_t b, uint32_t c) {
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    const h2 x = __builtin_bit_cast(h2, a), y = __builtin_bit_cast(h2, b), z = __builtin_bit_cast(h2, c);
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_minimum(__builtin_elementwise_minimum(x, y), z));
}
// The A operand of 32 bits of a row (mfma_pack_kernel): nibble t of dword j stands for bit j + 4 t, kept IN PLACE -- the codes
// 0x1, 0x2, 0x4 are e2m1 1/2, 1, 2 (bit 3 would be the sign: that dword moves down one bit) -- and the query fragments carry the
// reciprocal magnitudes (prologue).  5 vector instructions instead of the 7 of "(x >> j) & 0x11111111, << 1".
__device__ __forceinline__ v4i pk_rows(uint32_t x) {
    return v4i{(int)(x & 0x11111111u), (int)(x & 0x22222222u), (int)(x & 0x44444444u), (int)((x & 0x88888888u) >> 1)};
}

// The instructions of a stage (`stage`, `first_group`, `last_fold`).  What each part of a step costs was measured once by leaving
// it out (no fold, rows expanded once, no looks, the second tile unscaled): the fold is 16 % of the launch and sits on the vector
// issue port, the looks cost nothing -- profiles/r04_pack_step_accounting.txt.
#define ISK_PKM "v_pk_minimum3_f16 "
#define ISK_CMP "v_cmp_ne_u32_e64 %[mask], %[t], %[mA]\n"
#define ISK_MF1(n, av) "v_mfma_f32_32x32x64_f8f6f4 %[" #n "], %[" #av "], %[b], %[mg] cbsz:4 blgp:4\n"
#define ISK_MF2(n, av) "v_mfma_scale_f32_32x32x64_f8f6f4 %[" #n "], %[" #av "], %[b], %[" #n "], %[sh], %[so] op_sel_hi:[0,0,0] cbsz:4 blgp:4\n"

// DEPTH: steps whose rows a wave keeps in flight.  A chunk of 32 groups works ~5 000 cycles on a step's 1 KB of rows and one
// step ahead hides any latency; a chunk of one or two groups is done in ~400, and with one step (3 waves x 4 SIMDs x 1 KB =
// 12 KB per CU) in flight the scan crawled at 2.5 TB/s, bound by memory latency (32 queries: 0.33 ms per 100 M rows,
// profiles/r03_step_timelines.txt).  Small chunks run the DEPTH = 4 instantiation: the step body four times per loop trip,
// each on its own row registers.
// G: 0 = any number of groups, fragments from LDS, a step's groups pipelined among themselves; 1 / 2 = a chunk of exactly that
// many groups (<= 64 queries), fragments in registers, pipelined ACROSS steps (`few_step` below)
template <int MODE, int DEPTH, int G>
__global__ __launch_bounds__(MBLOCK, 3) void mfma_pack_kernel(const ScanParams p, const uint32_t groups) {
    constexpr int MT = PK_TILES;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    v4i* lb = reinterpret_cast<v4i*>(smem);
    uint32_t* lthr = reinterpret_cast<uint32_t*>(smem + (size_t)groups * 64 * 16);      // packed thresholds
    int* lpop = reinterpret_cast<int*>(lthr + groups * 32);
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t r = lane & 31, h = lane >> 5;
    const uint32_t q0 = blockIdx.y * groups * 32;

    // prologue: as mfma_scan_kernel<1>, thresholds packed
    for (uint32_t i = tid; i < groups * 32 * 2; i += MBLOCK) {
        const uint32_t ql = i >> 1, hh = i & 1;
        const uint32_t q = q0 + ql;
        // padding queries (bias BIAS_NEVER: beyond the batch's real queries) are all-zero words: as live queries they would score
        // +64 against a row of all ones, the one value the packed high half cannot hold -- their fragment is ZERO (every dot 0)
        const bool live = q < p.nq_pad && p.bias[q] != BIAS_NEVER;
        const uint64_t qw = live ? p.queries[(uint64_t)q * 4] : 0;
        const uint32_t x = hh ? (uint32_t)(qw >> 32) : (uint32_t)qw;
        const uint32_t m = live ? (hh ? p.mask_hi : p.mask_lo) : 0u;
        const uint32_t g = ql >> 5, c = ql & 31;
        v4i frag;
#pragma unroll
        // +-v with v = 2, 1, 1/2, 1/2 for the four dwords (e2m1 0x4, 0x2, 0x1, 0x1; sign = bit 3): the ROW nibbles of dword j are
        // 1/2, 1, 2, 2 (pk_rows), so that every product is +-1 and three of a row's four dwords cost ONE v_and each
        for (int j = 0; j < 4; ++j) frag[j] = (int)(((j == 0 ? 0x44444444u : j == 1 ? 0x22222222u : 0x11111111u) | (nibbles(x, j) << 3)) & (nibbles(m, j) * 0xFu));
        lb[(size_t)g * 64 + hh * 32 + c] = frag;
    }
    for (uint32_t ql = tid; ql < groups * 32; ql += MBLOCK) {
        const uint32_t q = q0 + ql;
        int pc = 0, tau = -1;
        if (q < p.nq_pad) {
            pc = __popcll(p.queries[(uint64_t)q * 4] & (((uint64_t)p.mask_hi << 32) | p.mask_lo));
            tau = (int)(0x7FFFFFFFu - p.bias[q]);
        }
        lpop[ql] = pc;
        if constexpr (MODE == MODE_SELF) lthr[ql] = q < p.nq_pad ? live_packed(p.thr_live + q) : 0u;     // the boot kernel wrote them packed
        else lthr[ql] = pack_threshold(tau - pc);
    }
    __syncthreads();

    const uint64_t first = p.row_begin / (32 * MT);                         // row_begin is a multiple of the XOR kernel's tile (>= 512 rows)
    const uint64_t nsteps = (p.n_rows + 32 * MT - 1) / (32 * MT);
    const uint64_t stride = (uint64_t)gridDim.x * (MBLOCK / 64);
    // the wave number as a SCALAR: step number and row addresses then live on the scalar unit (scalar-base loads)
    // (DEPTH > 1: a wave owns DEPTH consecutive steps at a time -- its loads in flight are DEPTH KB of ONE stretch of rows; DEPTH
    //  steps a grid stride apart measured slower, profiles/r03_ab_row_prefetch.txt)
    uint64_t step = first + ((uint64_t)blockIdx.x * (MBLOCK / 64) + (uint32_t)__builtin_amdgcn_readfirstlane((int)wave)) * DEPTH;
    if (step >= nsteps) return;
    const uint64_t last_row = p.n_rows - 1;
    const uint32_t* const col32 = reinterpret_cast<const uint32_t*>(p.col[0]);

    // ---- candidates ------------------------------------------------------------------------------------------------------------
    // A stage whose fold differs from T in some lane costs the hot loop NO global memory operation and no unrolled search: the
    // lanes that hold a hit copy their 32 accumulator registers (+ query, threshold) into their wave's LDS ring -- slots from
    // the compare's own lane mask, so the count stays wave-uniform -- and the stage loop goes on.  At the end of the step (or
    // when the ring is full) `process_ring` walks the saved blocks with a REAL loop: lane v looks at result v of a block (64
    // results: 32 registers x 2 halves), so the search for the hit is one compare per lane instead of 64 unrolled compares
    // with a branch each, and every hit of a block is appended by its own lane with all atomics in flight together.  Their
    // results are consumed by `Pending` at the lane's next hit or at the end of the NEXT step, when they (and the row prefetch,
    // which shares the in-order vmcnt) have long arrived.  Before: the 64 compares and two returned atomics per candidate sat in
    // the stage loop behind a vmcnt(0) that also waited for the row prefetch -- ~1.9 us of wave time per candidate (k = 100:
    // 3.5 ms per 100 M x 1 024 pass against 2.3 for k = 1, profiles/r03_ab_self.txt).
    constexpr uint32_t RING_E = PK_RING_ENTRIES, ENTRY = PK_RING_ENTRY_DWORDS;       // dwords: 32 registers | query, lane half | T | pad
    uint32_t* const ring = reinterpret_cast<uint32_t*>(lpop + groups * 32) + wave * (RING_E * ENTRY);
    uint32_t rcount = 0;                        // saved blocks in the ring (wave-uniform)
    // MODE_SELF: a candidate's list slot is requested here and its word stored once the slot is known -- at the lane's next
    // candidate or at the end of the next step.  Its distance counts are NO-RETURN atomics (count[q][t] += 1 for every t in
    // [hamming, threshold the compare ran under)): nobody waits for them; "k rows within t" is noticed by the CHECKER lanes
    // below, which read one counter per step each and lower the live threshold with one atomicMin on the packed word.
    // (The lane whose own increment crossed k used to do that: two returned atomics and a dependent chain of further ones per
    //  candidate, ~3.6 us of wave time each -- the level design beat the single pass by 10 % at 100 M rows and by 40 % at 12.5 M.)
    uint32_t pend_slot = 0, pend_lo = 0, pend_hi = 0x80000000u;        // pend_hi bit 31: nothing pending
    auto pend_complete = [&]() __attribute__((always_inline)) {
        if (!(pend_hi & 0x80000000u)) {
            const uint32_t qi = q0 + (pend_hi >> 20);                   // query in chunk : 11 | hamming : 7 | row >> 32 : 12
            if (pend_slot < p.cap) p.cand[(uint64_t)qi * p.cap + pend_slot] = ((uint64_t)((pend_hi >> 12) & 0x7Fu) << 48) | ((uint64_t)(pend_hi & 0xFFFu) << 32) | pend_lo;
            pend_hi = 0x80000000u;
        }
    };
    auto process_ring = [&](uint64_t st) __attribute__((always_inline)) {
        const uint32_t reg = lane >> 1, hf = lane & 1;
        // result `reg` of half `hf` is tile 2 (reg >> 4) + hf, matrix row (reg & 3) + 8 ((reg & 15) >> 2) + 4 (lane >> 5 of the
        // saving lane); tile t, matrix row m is row 64 (t & 1) + (t >> 1) + 2 m of the step (`expand`)
        const uint32_t off0 = 64 * hf + (reg >> 4) + 2 * ((reg & 3) + 8 * ((reg & 15) >> 2));
        for (uint32_t e = 0; e < rcount; ++e) {
            const uint32_t* const blk = ring + e * ENTRY;
            const uint32_t bits = blk[reg], head = blk[32], tpk = blk[33];
            const uint32_t ql = head & 0xFFFFu, off = off0 + 8 * (head >> 16);
            const bool below = hf ? bits < (tpk & 0xFFFF0000u) : (bits & 0xFFFFu) < (tpk & 0xFFFFu);
            const int d = hf ? (int)(bits >> 16) - (int)PK_HI0 : (int)(bits & 0xFFFFu) - (int)PK_LO0;
            const uint64_t row = st * (32 * MT) + off;
            // (d < -64 is no dot product of 64 bits: never turned into an index)
            if (below && d >= -64 && row <= last_row) {
                const int pc = lpop[ql];
                if constexpr (MODE == MODE_SELF) {
                    pend_complete();
                    const uint32_t qi = q0 + ql, hd = (uint32_t)(d + pc);
                    const int tau_seen = unpack_threshold(tpk) + pc;
                    pend_slot = atomicAdd(&p.cnt[(uint64_t)qi * CNT_STRIDE], 1u);
                    uint32_t* const counts = p.ghist + (uint64_t)qi * HB;
                    for (int t = (int)hd; t < tau_seen; ++t) __hip_atomic_fetch_add(&counts[t], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // result unused: no-return form
                    pend_lo = (uint32_t)row;
                    pend_hi = (ql << 20) | (hd << 12) | (uint32_t)(row >> 32);       // rows < 2^44
                } else {
                    emit<MODE>(p, q0 + ql, (uint32_t)(d + pc), row);
                }
            }
        }
        rcount = 0;
    };
    // `mask`: the lanes whose fold differs from T (query g * 32 + (lane & 31), rows 4 * (lane >> 5) + ... of the step's tiles)
    auto save_hits = [&](const Acc& acc, uint64_t mask, uint32_t tpk, uint32_t g, uint64_t st) __attribute__((always_inline)) {
        while (mask) {                              // wave-uniform; more than one trip only when the ring fills up
            const uint32_t room = RING_E - rcount;
            if (room == 0) { process_ring(st); continue; }
            const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
            const bool mine = ((mask >> lane) & 1) != 0 && rank < room;
            if (mine) {
                uint32_t* const blk = ring + (rcount + rank) * ENTRY;
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int i = 0; i < 16; i += 4)
                        *reinterpret_cast<float4*>(blk + 16 * j + i) = make_float4(acc.t[j][i], acc.t[j][i + 1], acc.t[j][i + 2], acc.t[j][i + 3]);
                *reinterpret_cast<uint2*>(blk + 32) = make_uint2((g * 32 + r) | (h << 16), tpk);
            }
            const uint64_t taken = __builtin_amdgcn_ballot_w64(mine);
            rcount += (uint32_t)__builtin_popcountll(taken);
            mask &= ~taken;
        }
    };

    const float mgf = __uint_as_float(PK_MAGIC);
    v16f magic = {mgf, mgf, mgf, mgf, mgf, mgf, mgf, mgf, mgf, mgf, mgf, mgf, mgf, mgf, mgf, mgf};
    asm volatile("" : "+v"(magic));                        // ONE register block for the whole kernel
    int sc_hi = (int)0x8F8F8F8F, sc_one = 0x7F7F7F7F;      // E8M0 block scales 2^16 and 2^0
    asm volatile("" : "+v"(sc_hi), "+v"(sc_one));
    v4i a[MT];

    // stage: MFMAs of the NEW group into `nw`, fold of the OLD group `od` with its packed threshold; returns the lanes whose
    // fold differs from T as a wave mask and the fold in `m`
    auto stage = [&](Acc& nw, const Acc& od, const v4i& b, uint32_t tpk, uint32_t& m) __attribute__((always_inline)) -> uint64_t {
        uint32_t mA, mB;
        uint64_t mask;
        const v16f& o0 = od.t[0];
        const v16f& o1 = od.t[1];
        asm volatile(ISK_MF1(n0, a0)
                     ISK_PKM "%[mA], %[t], %[u0], %[u1]\n" ISK_PKM "%[mB], %[u8], %[u9], %[u10]\n"
                     ISK_PKM "%[mA], %[mA], %[u2], %[u3]\n" ISK_PKM "%[mB], %[mB], %[u11], %[u12]\n"
                     : [n0] "=&v"(nw.t[0]), [mA] "=&v"(mA), [mB] "=&v"(mB)
                     : [a0] "v"(a[0]), [b] "v"(b), [mg] "v"(magic), [t] "v"(tpk), [u0] "v"(o0[0]), [u1] "v"(o0[1]), [u2] "v"(o0[2]), [u3] "v"(o0[3]),
                       [u8] "v"(o0[8]), [u9] "v"(o0[9]), [u10] "v"(o0[10]), [u11] "v"(o0[11]), [u12] "v"(o0[12]));
        asm volatile(ISK_MF1(n1, a2)
                     ISK_PKM "%[mA], %[mA], %[u4], %[u5]\n" ISK_PKM "%[mB], %[mB], %[u13], %[u14]\n"
                     ISK_PKM "%[mA], %[mA], %[u6], %[u7]\n" ISK_PKM "%[mB], %[mB], %[u15], %[w8]\n"
                     : [n1] "=&v"(nw.t[1]), [mA] "+v"(mA), [mB] "+v"(mB)
                     : [a2] "v"(a[2]), [b] "v"(b), [mg] "v"(magic), [u4] "v"(o0[4]), [u5] "v"(o0[5]), [u6] "v"(o0[6]), [u7] "v"(o0[7]),
                       [u13] "v"(o0[13]), [u14] "v"(o0[14]), [u15] "v"(o0[15]), [w8] "v"(o1[8]));
        asm volatile(ISK_MF2(n0, a1)
                     ISK_PKM "%[mA], %[mA], %[w0], %[w1]\n" ISK_PKM "%[mB], %[mB], %[w9], %[w10]\n"
                     ISK_PKM "%[mA], %[mA], %[w2], %[w3]\n" ISK_PKM "%[mB], %[mB], %[w11], %[w12]\n"
                     : [n0] "+v"(nw.t[0]), [mA] "+v"(mA), [mB] "+v"(mB)
                     : [a1] "v"(a[1]), [b] "v"(b), [sh] "v"(sc_hi), [so] "v"(sc_one), [w0] "v"(o1[0]), [w1] "v"(o1[1]), [w2] "v"(o1[2]), [w3] "v"(o1[3]),
                       [w9] "v"(o1[9]), [w10] "v"(o1[10]), [w11] "v"(o1[11]), [w12] "v"(o1[12]));
        asm volatile(ISK_MF2(n1, a3)
                     ISK_PKM "%[mA], %[mA], %[w4], %[w5]\n" ISK_PKM "%[mB], %[mB], %[w13], %[w14]\n"
                     ISK_PKM "%[mA], %[mA], %[w6], %[w7]\n"
                     "s_nop 0\n"
                     ISK_PKM "%[mA], %[mA], %[mB], %[w15]\n"
                     "s_nop 0\n"
                     ISK_CMP
                     : [n1] "+v"(nw.t[1]), [mA] "+v"(mA), [mB] "+v"(mB), [mask] "=s"(mask)
                     : [a3] "v"(a[3]), [b] "v"(b), [sh] "v"(sc_hi), [so] "v"(sc_one), [t] "v"(tpk), [w4] "v"(o1[4]), [w5] "v"(o1[5]), [w6] "v"(o1[6]), [w7] "v"(o1[7]),
                       [w13] "v"(o1[13]), [w14] "v"(o1[14]), [w15] "v"(o1[15]));
        m = mA;
        return mask;
    };
    // the four MFMAs of a step's FIRST group (nothing to fold beside them), padded so that the first stage may read them
    auto first_group = [&](Acc& nw, const v4i& b) __attribute__((always_inline)) {
        asm volatile(ISK_MF1(n0, a0) ISK_MF1(n1, a2) ISK_MF2(n0, a1) ISK_MF2(n1, a3) "s_nop 7\ns_nop 3\n"
                     : [n0] "=&v"(nw.t[0]), [n1] "=&v"(nw.t[1])
                     : [a0] "v"(a[0]), [a1] "v"(a[1]), [a2] "v"(a[2]), [a3] "v"(a[3]), [b] "v"(b), [mg] "v"(magic), [sh] "v"(sc_hi), [so] "v"(sc_one));
    };
    // the fold of a step's LAST group: same order as in a stage, no MFMA beside it
    auto last_fold = [&](const Acc& od, uint32_t tpk, uint32_t& m) __attribute__((always_inline)) -> uint64_t {
        uint32_t mA, mB;
        uint64_t mask;
        const v16f& o0 = od.t[0];
        const v16f& o1 = od.t[1];
        asm volatile("s_nop 3\n"
                     ISK_PKM "%[mA], %[t], %[u0], %[u1]\n" ISK_PKM "%[mB], %[u8], %[u9], %[u10]\n"
                     ISK_PKM "%[mA], %[mA], %[u2], %[u3]\n" ISK_PKM "%[mB], %[mB], %[u11], %[u12]\n"
                     ISK_PKM "%[mA], %[mA], %[u4], %[u5]\n" ISK_PKM "%[mB], %[mB], %[u13], %[u14]\n"
                     ISK_PKM "%[mA], %[mA], %[u6], %[u7]\n"
                     : [mA] "=&v"(mA), [mB] "=&v"(mB)
                     : [t] "v"(tpk), [u0] "v"(o0[0]), [u1] "v"(o0[1]), [u2] "v"(o0[2]), [u3] "v"(o0[3]), [u4] "v"(o0[4]), [u5] "v"(o0[5]), [u6] "v"(o0[6]), [u7] "v"(o0[7]),
                       [u8] "v"(o0[8]), [u9] "v"(o0[9]), [u10] "v"(o0[10]), [u11] "v"(o0[11]), [u12] "v"(o0[12]), [u13] "v"(o0[13]), [u14] "v"(o0[14]));
        asm volatile(ISK_PKM "%[mB], %[mB], %[u15], %[w8]\n"
                     ISK_PKM "%[mA], %[mA], %[w0], %[w1]\n" ISK_PKM "%[mB], %[mB], %[w9], %[w10]\n"
                     ISK_PKM "%[mA], %[mA], %[w2], %[w3]\n" ISK_PKM "%[mB], %[mB], %[w11], %[w12]\n"
                     ISK_PKM "%[mA], %[mA], %[w4], %[w5]\n" ISK_PKM "%[mB], %[mB], %[w13], %[w14]\n"
                     ISK_PKM "%[mA], %[mA], %[w6], %[w7]\n"
                     "s_nop 0\n"
                     ISK_PKM "%[mA], %[mA], %[mB], %[w15]\n"
                     "s_nop 0\n"
                     ISK_CMP
                     : [mA] "+v"(mA), [mB] "+v"(mB), [mask] "=s"(mask)
                     : [t] "v"(tpk), [u15] "v"(o0[15]), [w0] "v"(o1[0]), [w1] "v"(o1[1]), [w2] "v"(o1[2]), [w3] "v"(o1[3]), [w4] "v"(o1[4]), [w5] "v"(o1[5]), [w6] "v"(o1[6]),
                       [w7] "v"(o1[7]), [w8] "v"(o1[8]), [w9] "v"(o1[9]), [w10] "v"(o1[10]), [w11] "v"(o1[11]), [w12] "v"(o1[12]), [w13] "v"(o1[13]), [w14] "v"(o1[14]), [w15] "v"(o1[15]));
        m = mA;
        return mask;
    };

    const v4i* const lbl = lb + lane;
    const uint32_t* const lt = lthr + r;
    // A step is 128 rows = 1 KB, ONE 16-byte load per lane: lane L holds rows 2 L and 2 L + 1 of the step (x, y | z, w).  The
    // matrix-core operand wants a row's two dwords in lanes m and m + 32: v_permlane32_swap (gfx950) trades the upper half of
    // one register with the lower half of another, so swap(x, y) yields TWO tiles at once -- rows 2 m (lanes < 32 kept their x,
    // lanes >= 32 received y of lane m) and rows 2 m + 64 -- and swap(z, w) the tiles of rows 2 m + 1 and 2 m + 65.  Before:
    // four 4-byte loads per lane and step, four times the address work of the texture path for the same bytes.
    auto load_rows = [&](uint64_t st) __attribute__((always_inline)) -> u32x4 {          // compiler-scheduled: DEPTH == 1, and the table's partial last step
        if ((st + 1) * (32 * MT) <= p.n_rows) return __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(col32 + st * (64 * MT)) + lane);
        const uint64_t r0 = st * (32 * MT) + 2 * lane, r1 = r0 + 1;
        const uint2 lo = *reinterpret_cast<const uint2*>(col32 + (r0 <= last_row ? r0 : last_row) * 2);
        const uint2 hi = *reinterpret_cast<const uint2*>(col32 + (r1 <= last_row ? r1 : last_row) * 2);
        return u32x4{lo.x, lo.y, hi.x, hi.y};
    };
    auto expand = [&](const u32x4& v) __attribute__((always_inline)) {
        const auto e = __builtin_amdgcn_permlane32_swap(v[0], v[1], false, false);
        const auto o = __builtin_amdgcn_permlane32_swap(v[2], v[3], false, false);
        a[0] = pk_rows(e[0]);
        a[1] = pk_rows(e[1]);
        a[2] = pk_rows(o[0]);
        a[3] = pk_rows(o[1]);
    };
    // DEPTH > 1: the loads are issued from inline asm and retired by COUNTED waits, so that DEPTH steps of rows stay in flight.
    // (Left to hipcc, every step began with s_waitcnt vmcnt(0) and a copy of the whole row-register array: nothing was in flight
    //  while a step computed, and 17..64 queries scanned at 3.4 TB/s.)  Same discipline as load_tile_asm (valu_scan_kernel.hip.h), checked
    // at build time by tools/audit_kernels.py: nothing touches a destination between its load and its wait; `s_nop 4` in front
    // (a VALU-written SGPR base needs 5 wait states before a VMEM instruction reads it); no spills in this kernel.
    const uint32_t lane_bytes = lane * 16;
    auto issue_rows = [&](u32x4& dst, uint64_t st) __attribute__((always_inline)) {
        const uint64_t addr = reinterpret_cast<uint64_t>(col32) + st * (256 * MT);
        // (the step number is wave-uniform by construction; pinned to SGPRs here in case hipcc moved its arithmetic to the VALU)
        const unsigned char* const base = reinterpret_cast<const unsigned char*>(
            ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(addr >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)addr));
        // ("+v": a slot is ONE register quadruple for the whole kernel, updated in place -- as a fresh output per load, hipcc gave
        //  some instantiations' slots different registers in the loop and rotated them with copies at the back edge, in flight)
        // (`nt`: the rows are read once -- 9..32 queries scanned at 5.2 TB/s without the hint, 5.8 with it: 0.153 -> 0.139 ms per 100 M rows,
        //  profiles/r04_pmc_sq_small_chunks.txt; the XOR + popcount kernel's loads carry it too)
        asm volatile("s_nop 4\n\tglobal_load_dwordx4 %0, %1, %2 nt\n\t" : "+v"(dst) : "v"(lane_bytes), "s"(base) : "memory");
    };
    auto await_rows = [&](u32x4& v) __attribute__((always_inline)) {                     // DEPTH - 1 younger row loads are outstanding at every wait
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(DEPTH - 1) : "memory");
        asm volatile("" : "+v"(v));
    };
    const uint32_t wave_s = (uint32_t)__builtin_amdgcn_readfirstlane((int)wave);
    // thresholds [256 wave, 256 wave + 256) are this wave's to keep fresh, four per lane.  The lane number is RECOMPUTED at
    // each use (mbcnt of a laundered zero), or hipcc keeps a 64-bit global address and an LDS address alive through the
    // group loop for two instructions per look -- registers the rare path needs (168 with them: one spilled)
    auto fresh_index = [&]() __attribute__((always_inline)) {
        uint32_t z = 0;
        asm volatile("" : "+v"(z));
        return wave_s * 256 + __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, z)) * 4;
    };
    const bool refresh = MODE == MODE_SELF && wave * 256 + lane * 4 < groups * 32 && q0 + wave * 256 + lane * 4 < p.nq_pad;
    // a step is 128 rows here (64 in mfma_scan_kernel): look half as many steps apart for the same rows per look
    const uint32_t refresh_mask = (groups >= 32 ? 1u : groups >= 16 ? 2u : groups >= 8 ? 4u : groups >= 4 ? 8u : 16u) * ((p.refresh_steps + 1) / 2) - 1u;
    // CHECKERS (MODE_SELF): task (query, j) asks "do k appended rows lie within tau_q - j?", j = 1..4, by reading count[q][tau_q - j]
    // at the start of a look step and lowering the live threshold at its end.  64 tasks per wave and look: the first
    // `slices` waves of the grid take one slice each; a grid with fewer waves rotates through the slices step by step.
    const uint32_t slices = groups * 32 * 4 / 64, nwaves = gridDim.x * (MBLOCK / 64);
    const uint32_t gw = blockIdx.x * (MBLOCK / 64) + wave_s;
    uint32_t trip = 0;
    Acc accX, accY;
    auto all_groups = [&]() __attribute__((always_inline)) {
        // two B buffers and two accumulator sets: the fragment of group g + 2 is requested while group g + 1 multiplies
        // (any number of groups: pairs of stages while at least three groups remain, then one stage + the last fold for an even
        //  rest or the last fold alone for an odd one -- 17..32 queries are ONE group, not one and a padding group)
        v4i by = lbl[0], bx = lbl[groups > 1 ? 64 : 0];
        uint32_t thrY = lt[0], thrX = lt[groups > 1 ? 32 : 0];
        uint32_t mY, mX;
        first_group(accY, by);
        uint32_t g = 0;
#pragma unroll 1
        for (; g + 2 < groups; g += 2) {
            by = lbl[(g + 2) * 64];                       // consumed by the stage before
            const uint32_t thrYn = lt[(g + 2) * 32];
            if (const uint64_t mk = stage(accX, accY, bx, thrY, mY); __builtin_expect(mk != 0, 0)) save_hits(accY, mk, thrY, g, step);
            thrY = thrYn;
            const uint32_t g3 = g + 3 < groups ? g + 3 : g + 2;       // (an odd count has no group g + 3: nothing is multiplied with it)
            bx = lbl[g3 * 64];
            const uint32_t thrXn = lt[g3 * 32];
            if (const uint64_t mk = stage(accY, accX, by, thrX, mX); __builtin_expect(mk != 0, 0)) save_hits(accX, mk, thrX, g + 1, step);
            thrX = thrXn;
        }
        if (g + 1 < groups) {
            if (const uint64_t mk = stage(accX, accY, bx, thrY, mY); mk != 0) save_hits(accY, mk, thrY, g, step);
            if (const uint64_t mk = last_fold(accX, thrX, mX); mk != 0) save_hits(accX, mk, thrX, g + 1, step);
        } else {
            if (const uint64_t mk = last_fold(accY, thrY, mY); mk != 0) save_hits(accY, mk, thrY, g, step);
        }
    };
    // The general loop with the same carry across steps, for EVEN group counts (an odd count would trade the roles of the two
    // accumulator sets from step to step: two copies of the loop, which do not fit 168 registers): the step's first stage
    // multiplies group 0 into accY while it folds what the PREVIOUS step left in accX (its last group) -- `first_group` and
    // `last_fold` stood alone for 128 + 12 and ~80 cycles per step and wave, 5 % of a 32-group step (A/B: profiles/r03_ab_carry.txt).
    bool carried = false;                                 // accX holds the previous step's last group
    auto even_groups = [&](uint64_t prev) __attribute__((always_inline)) {
        v4i by = lbl[0], bx = lbl[64];
        uint32_t thrY = lt[0], thrX = lt[32];
        const uint32_t thrL = lt[(groups - 1) * 32];
        uint32_t mY, mX;
        if (const uint64_t mk = stage(accY, accX, by, thrL, mX); __builtin_expect(carried && mk != 0, 0)) { save_hits(accX, mk, thrL, groups - 1, prev); process_ring(prev); }
        uint32_t g = 0;
#pragma unroll 1
        for (; g + 2 < groups; g += 2) {
            by = lbl[(g + 2) * 64];                       // consumed by the stage before
            const uint32_t thrYn = lt[(g + 2) * 32];
            if (const uint64_t mk = stage(accX, accY, bx, thrY, mY); __builtin_expect(mk != 0, 0)) save_hits(accY, mk, thrY, g, step);
            thrY = thrYn;
            bx = lbl[(g + 3) * 64];
            const uint32_t thrXn = lt[(g + 3) * 32];
            if (const uint64_t mk = stage(accY, accX, by, thrX, mX); __builtin_expect(mk != 0, 0)) save_hits(accX, mk, thrX, g + 1, step);
            thrX = thrXn;
        }
        if (const uint64_t mk = stage(accX, accY, bx, thrY, mY); __builtin_expect(mk != 0, 0)) save_hits(accY, mk, thrY, g, step);
        carried = true;
    };
    auto even_flush = [&](uint64_t prev) __attribute__((always_inline)) {
        if (carried) {
            uint32_t m;
            const uint32_t t = lt[(groups - 1) * 32];
            if (const uint64_t mk = last_fold(accX, t, m); mk != 0) { save_hits(accX, mk, t, groups - 1, prev); process_ring(prev); }
            carried = false;
        }
    };
    // FEW GROUPS.  With one or two groups a step has nothing of its own to hide behind: the first group's MFMAs and the last
    // group's fold stood alone (128 + 12 idle cycles and ~80 per 1 KB of rows and wave).  Here the accumulators live ACROSS
    // steps: a stage multiplies this step's rows while it folds what the previous stage left -- for one group the previous
    // STEP's products (the two accumulator sets trade roles from step to step: the unrolled DEPTH loop makes that static), for
    // two groups (s, g0) beside the fold of (s - 1, g1) and (s, g1) beside the fold of (s, g0).  The fragments stay in
    // registers.  A stage's candidates are processed at once (the ring then never mixes steps); `have`: something to fold.
    constexpr int FB = G == 1 || G == 2 ? G : 1;          // one or two groups keep their fragments in registers
    v4i fb[FB];
    bool have = false;
    if constexpr (G == 1 || G == 2) {
#pragma unroll
        for (int g = 0; g < G; ++g) fb[g] = lbl[g * 64];
    }
    // P receives the even groups, Q the odd ones; on entry Q holds the previous step's last group.  An even G leaves its last
    // group in Q again; an odd G leaves it in P: the caller swaps the sets from step to step.
    auto few_step = [&](Acc& P, Acc& Q, uint64_t prev) __attribute__((always_inline)) {      // prev: the step before `step`
        uint32_t m;
        v4i bcur;
        if constexpr (G == 1 || G == 2) bcur = fb[0];
        else bcur = lbl[0];
#pragma unroll
        for (int g = 0; g < (G > 0 ? G : 1); ++g) {
            v4i bnext = bcur;
            if (g + 1 < G) {
                if constexpr (G == 2) bnext = fb[FB - 1];
                else bnext = lbl[(g + 1) * 64];                             // requested while group g multiplies
            }
            Acc& nw = (g & 1) ? Q : P;
            Acc& od = (g & 1) ? P : Q;
            const uint32_t t = lt[(g == 0 ? G - 1 : g - 1) * 32];            // the threshold of the group being FOLDED
            const uint64_t mk = stage(nw, od, bcur, t, m);
            if (g == 0) {
                if (__builtin_expect(have && mk != 0, 0)) { save_hits(od, mk, t, G - 1, prev); process_ring(prev); }
            } else {
                if (__builtin_expect(mk != 0, 0)) { save_hits(od, mk, t, g - 1, step); process_ring(step); }
            }
            bcur = bnext;
        }
        have = true;
    };
    auto few_flush = [&](Acc& od, uint64_t prev) __attribute__((always_inline)) {        // the fold of the last products: those of step `prev`
        if (have) {
            uint32_t m;
            const uint32_t t = lt[(G > 0 ? G - 1 : 0) * 32];
            if (const uint64_t mk = last_fold(od, t, m); mk != 0) { save_hits(od, mk, t, G > 0 ? G - 1 : 0, prev); process_ring(prev); }
            have = false;
        }
    };
    // one step over the rows expanded in a[]: `body` multiplies and folds
    auto one_step = [&](auto&& body) __attribute__((always_inline)) {
        uint32_t fresh[4] = {0u, 0u, 0u, 0u};
        const bool look = trip < 4 || (trip & refresh_mask) == 0;
        const bool refresh_now = refresh && look;
        uint32_t chk_count = 0, chk_what = ~0u;       // chk_what: query in chunk | hamming level << 16, ~0: no task
        if constexpr (MODE == MODE_SELF) {
            if (refresh_now) {
                const float* const src = p.thr_live + q0 + fresh_index();
#pragma unroll
                for (int i = 0; i < 4; ++i) fresh[i] = live_packed(src + i);
            }
            const uint32_t slice = nwaves >= slices ? gw : (gw + trip * nwaves) % slices;
            if (look && slice < slices) {
                uint32_t z = 0;
                asm volatile("" : "+v"(z));
                const uint32_t task = slice * 64 + __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, z));
                const uint32_t ql = task >> 2, tpk = lthr[ql];
                const int level = unpack_threshold(tpk) + lpop[ql] - 1 - (int)(task & 3);
                if (tpk != 0 && level >= 0 && q0 + ql < p.nq_pad) {
                    chk_what = ql | ((uint32_t)level << 16);
                    chk_count = (uint32_t)__hip_atomic_load(reinterpret_cast<const int*>(p.ghist + (uint64_t)(q0 + ql) * HB + level), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
        }
        body();
        // what the PREVIOUS step's appends returned (issued a whole step ago: no wait), then this step's blocks
        if constexpr (MODE == MODE_SELF) pend_complete();
        if (rcount) process_ring(step);
        if constexpr (MODE == MODE_SELF) {
            if (chk_what != ~0u && chk_count >= p.k) {
                const uint32_t ql = chk_what & 0xFFFFu;
                atomicMin(reinterpret_cast<uint32_t*>(p.thr_live) + q0 + ql, pack_threshold((int)(chk_what >> 16) - lpop[ql]));
            }
            if (refresh_now) *reinterpret_cast<uint4*>(lthr + fresh_index()) = make_uint4(fresh[0], fresh[1], fresh[2], fresh[3]);
        }
    };
    if constexpr (DEPTH == 1) {
        u32x4 x = load_rows(step);
        if (groups & 1) {
            while (step < nsteps) {
                expand(x);
                x = load_rows(step + stride < nsteps ? step + stride : step);    // in flight during this step
                one_step(all_groups);
                step += stride;
                ++trip;
            }
        } else {
            while (step < nsteps) {
                expand(x);
                x = load_rows(step + stride < nsteps ? step + stride : step);
                one_step([&]() __attribute__((always_inline)) { even_groups(step - stride); });
                step += stride;
                ++trip;
            }
            even_flush(step - stride);
        }
    } else {
        const uint64_t nfull = p.n_rows / (32 * MT);          // whole steps: [first, nfull); a partial last step is loaded the slow way
        const uint64_t leap = stride * DEPTH;                 // from a wave's stretch of DEPTH steps to its next one
        u32x4 x[DEPTH];
#pragma unroll
        for (int d = 0; d < DEPTH; ++d) x[d] = u32x4{0u, 0u, 0u, 0u};
        if (step < nfull) {
            uint64_t base = step, last = step;
            uint32_t last_d = 0;
            bool more = true;
#pragma unroll
            for (int d = 0; d < DEPTH; ++d) issue_rows(x[d], base + d < nfull ? base + d : base);
            while (more) {
#pragma unroll
                for (int d = 0; d < DEPTH; ++d) {
                    step = base + d;
                    if (step >= nfull) { more = false; break; }
                    const uint64_t prev = d ? step - 1 : step - leap + (DEPTH - 1);
                    await_rows(x[d]);
                    expand(x[d]);
                    issue_rows(x[d], step + leap < nfull ? step + leap : base);   // (past the end: a re-read nobody uses)
                    if constexpr (G == 0) one_step(all_groups);
                    else if constexpr ((G & 1) != 0) {
                        static_assert((DEPTH & 1) == 0, "the accumulator roles of an odd group count alternate with d");
                        if (d & 1) one_step([&]() __attribute__((always_inline)) { few_step(accY, accX, prev); });
                        else one_step([&]() __attribute__((always_inline)) { few_step(accX, accY, prev); });
                        last_d = d;
                    } else one_step([&]() __attribute__((always_inline)) { few_step(accX, accY, prev); });
                    last = step;
                    ++trip;
                }
                if (more) { base += leap; step = base; }
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            if constexpr ((G & 1) != 0) {                     // the last group waits in P of the last call
                if (last_d & 1) few_flush(accY, last);
                else few_flush(accX, last);
            } else if constexpr (G > 1) few_flush(accY, last);   // ... in Q
        }
        if (step < nsteps) {                                  // == nfull: this wave owns the partial step
            expand(load_rows(step));
            one_step(all_groups);
        }
    }
    if constexpr (MODE == MODE_SELF) pend_complete();
}

#undef ISK_MF1
#undef ISK_MF2
#undef ISK_PKM
#undef ISK_CMP

}  // namespace isk
