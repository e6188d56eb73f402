// mfma_pack3_kernel.hip.h -- mfma_pack3_kernel, 64-bit codes (W = 1): THREE row tiles per accumulator, folded by a bitwise OR of
// indicator bits (included by mfma_scan.hip).
//
// mfma_pack_kernel folds two dot products per register with min: 16 v_pk_minimum3_f16 + v_cmp per four MFMAs, at its
// instruction minimum (profiles/r04_pack_step_accounting.txt).  Here a register holds THREE results and the fold is an OR:
//
//   * rows AND queries are +1 / -1 (e2m1 0x2 / 0xA; masked query bits 0), so an MFMA computes sum s(r) s(q) = m - 2 d over the
//     m compared bits: no per-query popcount is left in the product;
//   * tile t of an accumulator is multiplied with block scale 2^(7 t) (t = 0: the unscaled form) into ONE f32 whose start value
//     is 2^23 + sum_t 2^(7 t + 1) (63 + T - m / 2):  field t, bits 1 + 7 t .. 7 + 7 t, then holds 63 + T - d_t, in 0..127 for
//     every d in 0..64 and T in 1..64 -- no carry between fields, the value stays in [2^23, 2^24) (ulp 1, every sum exact; bit 0
//     stays 0: m is even, the products are +-1), and bit 6 of a field (P3_IND) is set exactly when d_t < T;
//   * T is ONE value per wave (the start value is one register block shared by every group): the largest live hamming
//     threshold of the chunk's queries + 1.  A set indicator only says d < T: the candidate path tests every field against its
//     own query's threshold (process_ring), as mfma_pack_kernel does;
//   * the fold of a stage (six tiles, two accumulators, 32 registers) is 15 v_or3_b32 + one v_bitop3_b32 ((A | B) & P3_IND)
//     + one v_cmp: 17 instructions per SIX MFMAs instead of 17 per four.
//
// T is derived from the per-wave maxima in LDS (`lmax`: each wave reduces its slice of the thresholds when it refreshes them)
// and only ever drops; a drop rewrites the start block (16 v_mov) between steps.  A query whose threshold admits every row
// (>= 64) cannot be expressed by an indicator bit (65 values): the wave then runs with T = 64 and a fold mask that includes
// bit 30, which every accumulator holds, so every lane takes the candidate path until the threshold drops.
//
// Same hazard rules as mfma_pack_kernel (stage in issue order, distances kept by construction, checked by tools/audit_kernels.py):
// an accumulator's three MFMAs are one chain (a chain of one instruction needs no interleaving for throughput), so the old
// group's accumulator 0 is complete three MFMAs before the end of the previous stage and is folded first; accumulator 1 is
// read from the stage's third MFMA on, >= 12 instructions after the MFMA that completed it.
#pragma once

#include "mfma_common.hip.h"

namespace isk {

constexpr int P3_TILES = 6;                                             // row tiles per wave and step: 192 rows
constexpr uint32_t P3_IND = 0x00204080u;                                // bit 6 of the fields at bits 1, 8, 15
constexpr uint32_t P3_LDS_EXTRA = 16;                                   // lmax: one int per wave behind the rings

// start value (bit pattern) for block threshold T (1..64) and m compared bits (even)
__host__ __device__ __forceinline__ uint32_t p3_start(uint32_t T, uint32_t m) {
    const uint32_t bias = 63 + T - m / 2;
    return 0x4B000000u | (bias << 1) | (bias << 8) | (bias << 15);
}
// The A operand of 32 bits of a row: nibble t of dword j holds bit 4 t + 3 - j as the SIGN of +-1 (the query fragments use the
// same map).  7 vector instructions per 32 bits (one v_and_or for dword 0, a shift + v_and_or for the others).
__device__ __forceinline__ v4i p3_rows(uint32_t x) {
    return v4i{(int)((x & 0x88888888u) | 0x22222222u), (int)(((x << 1) & 0x88888888u) | 0x22222222u),
               (int)(((x << 2) & 0x88888888u) | 0x22222222u), (int)(((x << 3) & 0x88888888u) | 0x22222222u)};
}
// a packed live threshold (pack_threshold) as a hamming threshold clamped to -1..64, plus 1 (0: no row can hit)
__device__ __forceinline__ int p3_tau1(uint32_t tpk, int pc) {
    const int t = unpack_threshold(tpk) + pc;
    return (t < -1 ? -1 : t > 64 ? 64 : t) + 1;
}
// maximum over the wave of non-negative values (DPP row shifts, then the row broadcasts; lane 63 ends with it), wave-uniform
__device__ __forceinline__ int p3_wave_max(int v) {
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x111, 0xF, 0xF, false));      // row_shr:1
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x112, 0xF, 0xF, false));      // row_shr:2
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x114, 0xF, 0xF, false));      // row_shr:4
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x118, 0xF, 0xF, false));      // row_shr:8
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x142, 0xF, 0xF, false));      // row_bcast:15
    v = max(v, __builtin_amdgcn_update_dpp(0, v, 0x143, 0xF, 0xF, false));      // row_bcast:31
    return __builtin_amdgcn_readlane(v, 63);
}

#define ISK_P3A(n, av) "v_mfma_f32_32x32x64_f8f6f4 %[" #n "], %[" #av "], %[b], %[st] cbsz:4 blgp:4\n"
#define ISK_P3B(n, av) "v_mfma_scale_f32_32x32x64_f8f6f4 %[" #n "], %[" #av "], %[b], %[" #n "], %[s7], %[so] op_sel_hi:[0,0,0] cbsz:4 blgp:4\n"
#define ISK_P3C(n, av) "v_mfma_scale_f32_32x32x64_f8f6f4 %[" #n "], %[" #av "], %[b], %[" #n "], %[s14], %[so] op_sel_hi:[0,0,0] cbsz:4 blgp:4\n"
#define ISK_OR3(d, x, y, z) "v_or3_b32 %[" #d "], %[" #x "], %[" #y "], %[" #z "]\n"

// Chunks of more than PK_DEEP_GROUPS groups only (the one-step-deep loop of mfma_pack_kernel<MODE, 1, 0>).  ODD: the group count
// is odd -- a step's first group and last fold stand alone; even counts carry the last group into the next step (one kernel with
// both loops does not fit 168 registers in MODE_SELF).
template <int MODE, bool ODD>
__global__ __launch_bounds__(MBLOCK, 3) void mfma_pack3_kernel(const ScanParams p, const uint32_t groups) {
    constexpr uint32_t ROWS = 32 * P3_TILES;
    constexpr uint32_t RING_E = PK_RING_ENTRIES, ENTRY = PK_RING_ENTRY_DWORDS;    // dwords: 32 registers | query, lane half | T | pad
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    v4i* lb = reinterpret_cast<v4i*>(smem);
    uint32_t* lthr = reinterpret_cast<uint32_t*>(smem + (size_t)groups * 64 * 16);      // packed thresholds (as mfma_pack_kernel)
    int* lpop = reinterpret_cast<int*>(lthr + groups * 32);
    uint32_t* const rings = reinterpret_cast<uint32_t*>(lpop + groups * 32);
    int* const lmax = reinterpret_cast<int*>(rings + (MBLOCK / 64) * RING_E * ENTRY);    // per wave: max p3_tau1 of its slice
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t q0 = blockIdx.y * groups * 32;
    const uint32_t mbits = (uint32_t)(__popc(p.mask_lo) + __popc(p.mask_hi));         // compared bits: whole bytes, even

    // prologue: +-1 query fragments (0 beyond the compared prefix and for padding queries: every dot 0, d reads m / 2)
    for (uint32_t i = tid; i < groups * 32 * 2; i += MBLOCK) {
        const uint32_t ql = i >> 1, hh = i & 1;
        const uint32_t q = q0 + ql;
        const bool live = q < p.nq_pad && p.bias[q] != BIAS_NEVER;
        const uint64_t qw = live ? p.queries[(uint64_t)q * 4] : 0;
        const uint32_t x = hh ? (uint32_t)(qw >> 32) : (uint32_t)qw;
        const uint32_t m = live ? (hh ? p.mask_hi : p.mask_lo) : 0u;
        const uint32_t g = ql >> 5, c = ql & 31;
        v4i frag;
#pragma unroll
        for (int j = 0; j < 4; ++j) frag[j] = (int)((((x << j) & 0x88888888u) | 0x22222222u) & ((((m << j) & 0x88888888u) >> 3) * 0xFu));
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
        if constexpr (MODE == MODE_SELF) lthr[ql] = q < p.nq_pad ? live_packed(p.thr_live + q) : 0u;
        else lthr[ql] = pack_threshold(tau - pc);
    }
    __syncthreads();

    const uint32_t wave_s = (uint32_t)__builtin_amdgcn_readfirstlane((int)wave);
    auto fresh_index = [&]() __attribute__((always_inline)) {
        uint32_t z = 0;
        asm volatile("" : "+v"(z));
        return wave_s * 256 + __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, z)) * 4;
    };
    const bool mine4 = wave * 256 + lane * 4 < groups * 32;         // this lane's four thresholds of the wave's slice exist
    // the wave's slice maximum of p3_tau1 over four packed thresholds per lane -> lmax[wave]
    auto publish_max = [&](const uint32_t (&t4)[4], bool valid) __attribute__((always_inline)) {
        int v = 0;
        if (valid) {
            const int4 pc = *reinterpret_cast<const int4*>(lpop + fresh_index());
            v = max(max(p3_tau1(t4[0], pc.x), p3_tau1(t4[1], pc.y)), max(p3_tau1(t4[2], pc.z), p3_tau1(t4[3], pc.w)));
        }
        v = p3_wave_max(v);
        if (lane == 0) lmax[wave] = v;
    };
    {
        uint32_t t4[4] = {0u, 0u, 0u, 0u};
        if (mine4) {
            const uint4 v = *reinterpret_cast<const uint4*>(lthr + fresh_index());
            t4[0] = v.x; t4[1] = v.y; t4[2] = v.z; t4[3] = v.w;
        }
        publish_max(t4, mine4);
    }
    __syncthreads();

    const uint64_t nsteps = (p.n_rows - p.row_begin + ROWS - 1) / ROWS;    // steps from row_begin; the last may be partial
    const uint64_t stride = (uint64_t)gridDim.x * (MBLOCK / 64);
    uint64_t step = (uint64_t)blockIdx.x * (MBLOCK / 64) + wave_s;
    if (step >= nsteps) return;
    const uint64_t last_row = p.n_rows - 1;
    const uint32_t* const col32 = reinterpret_cast<const uint32_t*>(p.col[0]);

    // ---- the block threshold T and the start value -------------------------------------------------------------------------
    // tcur: T in force, 1..65 (65: some query admits every row -- the products are made with T = 64 and every lane is a candidate)
    uint32_t tcur = 65;
    const float s0 = __uint_as_float(p3_start(64, mbits));
    v16f start = {s0, s0, s0, s0, s0, s0, s0, s0, s0, s0, s0, s0, s0, s0, s0, s0};
    auto update_t = [&]() __attribute__((always_inline)) {
        const int4 mx = *reinterpret_cast<const int4*>(lmax);
        const uint32_t t1 = (uint32_t)__builtin_amdgcn_readfirstlane(max(max(mx.x, mx.y), max(mx.z, mx.w)));   // max tau + 1: 0..65
        const uint32_t tn = t1 < 1 ? 1u : t1;
        if (tn < tcur) {
            tcur = tn;
            const float sv = __uint_as_float(p3_start(tn > 64 ? 64u : tn, mbits));
            start = v16f{sv, sv, sv, sv, sv, sv, sv, sv, sv, sv, sv, sv, sv, sv, sv, sv};
        }
        asm volatile("" : "+v"(start));                   // ONE register block for the whole kernel
    };
    update_t();
    auto t_of = [](uint32_t t) { return t > 64 ? 64u : t; };   // the T the products were made with
    // the mask of the fold: the indicator bits, and with T = 65 also bit 30, which every accumulator has set (2^23 <= value < 2^24)
    auto ind_of = [](uint32_t t) { return t > 64 ? P3_IND | 0x40000000u : P3_IND; };

    // ---- candidates: as in mfma_pack_kernel, three fields per saved register ---------------------------------------------------
    uint32_t rcount = 0;
    uint32_t pend_slot = 0, pend_lo = 0, pend_hi = 0x80000000u;        // pend_hi bit 31: nothing pending
    auto pend_complete = [&]() __attribute__((always_inline)) {
        if (!(pend_hi & 0x80000000u)) {
            const uint32_t qi = q0 + (pend_hi >> 20);                   // query in chunk : 11 | hamming : 7 | row >> 32 : 12
            if (pend_slot < p.cap) p.cand[(uint64_t)qi * p.cap + pend_slot] = ((uint64_t)((pend_hi >> 12) & 0x7Fu) << 48) | ((uint64_t)(pend_hi & 0xFFFu) << 32) | pend_lo;
            pend_hi = 0x80000000u;
        }
    };
    // TWO saved blocks per trip: lane v takes register v & 31 of block e + (v >> 5) and tests its three fields
    // (lane numbers in the candidate path are RECOMPUTED -- mbcnt of a laundered zero -- so that hipcc keeps none of them alive
    //  through the stage loop: the rare path inside it peaks at the register limit)
    auto lane_now = [&]() __attribute__((always_inline)) {
        uint32_t z = 0;
        asm volatile("" : "+v"(z));
        return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, z));
    };
    auto process_ring = [&](uint64_t st) __attribute__((always_inline)) {
        const uint32_t ln = lane_now(), sub = ln >> 5, reg = ln & 31, i = reg & 15, acc = reg >> 4;
        const uint32_t m0 = (i & 3) + 8 * (i >> 2);                    // matrix row of result i (+ 4 for the upper lane half)
        const uint64_t row0 = p.row_begin + st * ROWS;
        for (uint32_t e = 0; e < rcount; e += 2) {
            if (e + sub < rcount) {
                const uint32_t* const blk = rings + wave_s * (RING_E * ENTRY) + (e + sub) * ENTRY;
                const uint32_t bits = blk[reg], head = blk[32], tb = blk[33];
                const uint32_t ql = head & 0xFFFFu, mm = m0 + 4 * (head >> 16);
                const int pc = lpop[ql];
                const int tau = unpack_threshold(lthr[ql]) + pc;          // the query's own live threshold (<= the one T came from)
#pragma unroll 1
                for (int f = 0; f < 3; ++f) {
                    const int d = 63 + (int)tb - (int)((bits >> (1 + 7 * f)) & 0x7Fu);
                    const uint32_t t = 3 * acc + f;                       // tile: a[t] of `expand`
                    const uint64_t row = row0 + (t < 4 ? 2 * mm + 64 * (t & 1) + (t >> 1) : 128 + 32 * (t - 4) + mm);
                    // (d < 0 is no distance of 64 bits: never turned into an index)
                    if (d <= tau && d >= 0 && row <= last_row) {
                        if constexpr (MODE == MODE_SELF) {
                            pend_complete();
                            const uint32_t qi = q0 + ql, hd = (uint32_t)d;
                            pend_slot = atomicAdd(&p.cnt[(uint64_t)qi * CNT_STRIDE], 1u);
                            uint32_t* const counts = p.ghist + (uint64_t)qi * HB;
                            for (int tt = d; tt < tau; ++tt) __hip_atomic_fetch_add(&counts[tt], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            pend_lo = (uint32_t)row;
                            pend_hi = (ql << 20) | (hd << 12) | (uint32_t)(row >> 32);
                        } else {
                            emit<MODE>(p, q0 + ql, (uint32_t)d, row);
                        }
                    }
                }
            }
        }
        rcount = 0;
    };
    auto save_hits = [&](const Acc& a2, uint64_t mask, uint32_t tb, uint32_t g, uint64_t st) __attribute__((always_inline)) {
        while (mask) {                              // wave-uniform; more than one trip only when the ring fills up
            const uint32_t room = RING_E - rcount;
            if (room == 0) { process_ring(st); continue; }
            const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
            const uint32_t ln = lane_now();
            const bool mine = ((mask >> ln) & 1) != 0 && rank < room;
            if (mine) {
                uint32_t* const blk = rings + wave_s * (RING_E * ENTRY) + (rcount + rank) * ENTRY;
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int i = 0; i < 16; i += 4)
                        *reinterpret_cast<float4*>(blk + 16 * j + i) = make_float4(a2.t[j][i], a2.t[j][i + 1], a2.t[j][i + 2], a2.t[j][i + 3]);
                *reinterpret_cast<uint2*>(blk + 32) = make_uint2((g * 32 + (ln & 31)) | ((ln >> 5) << 16), tb);
            }
            const uint64_t taken = __builtin_amdgcn_ballot_w64(mine);
            rcount += (uint32_t)__builtin_popcountll(taken);
            mask &= ~taken;
        }
    };

    // E8M0 block scales 2^7, 2^14 and 2^0 (VGPRs), the fold's mask in an SGPR
    int sc7 = (int)0x86868686, sc14 = (int)0x8D8D8D8D, sc_one = 0x7F7F7F7F;
    asm volatile("" : "+v"(sc7), "+v"(sc14), "+v"(sc_one));
    v4i a[P3_TILES];

    // stage: the six MFMAs of the NEW group into `nw` (accumulator 0: tiles 0..2, then accumulator 1: tiles 3..5), the fold of
    // the OLD group `od`: returns the lanes with some bit of `ind` set (ind_of)
    auto stage = [&](Acc& nw, const Acc& od, const v4i& b, uint32_t ind) __attribute__((always_inline)) -> uint64_t {
        uint32_t oA, oB, rr;
        uint64_t mask;
        const v16f& u = od.t[0];
        const v16f& w = od.t[1];
        asm volatile(ISK_P3A(n0, a0)
                     ISK_OR3(A, u0, u1, u2) ISK_OR3(B, u3, u4, u5) ISK_OR3(A, A, u6, u7)
                     : [n0] "=&v"(nw.t[0]), [A] "=&v"(oA), [B] "=&v"(oB)
                     : [a0] "v"(a[0]), [b] "v"(b), [st] "v"(start), [u0] "v"(u[0]), [u1] "v"(u[1]), [u2] "v"(u[2]), [u3] "v"(u[3]), [u4] "v"(u[4]),
                       [u5] "v"(u[5]), [u6] "v"(u[6]), [u7] "v"(u[7]));
        asm volatile(ISK_P3B(n0, a1)
                     ISK_OR3(B, B, u8, u9) ISK_OR3(A, A, u10, u11) ISK_OR3(B, B, u12, u13)
                     : [n0] "+v"(nw.t[0]), [A] "+v"(oA), [B] "+v"(oB)
                     : [a1] "v"(a[1]), [b] "v"(b), [s7] "v"(sc7), [so] "v"(sc_one), [u8] "v"(u[8]), [u9] "v"(u[9]), [u10] "v"(u[10]), [u11] "v"(u[11]),
                       [u12] "v"(u[12]), [u13] "v"(u[13]));
        asm volatile(ISK_P3C(n0, a2)
                     ISK_OR3(A, A, u14, u15) ISK_OR3(B, B, w0, w1) ISK_OR3(A, A, w2, w3)
                     : [n0] "+v"(nw.t[0]), [A] "+v"(oA), [B] "+v"(oB)
                     : [a2] "v"(a[2]), [b] "v"(b), [s14] "v"(sc14), [so] "v"(sc_one), [u14] "v"(u[14]), [u15] "v"(u[15]), [w0] "v"(w[0]), [w1] "v"(w[1]),
                       [w2] "v"(w[2]), [w3] "v"(w[3]));
        asm volatile(ISK_P3A(n1, a3)
                     ISK_OR3(B, B, w4, w5) ISK_OR3(A, A, w6, w7) ISK_OR3(B, B, w8, w9)
                     : [n1] "=&v"(nw.t[1]), [A] "+v"(oA), [B] "+v"(oB)
                     : [a3] "v"(a[3]), [b] "v"(b), [st] "v"(start), [w4] "v"(w[4]), [w5] "v"(w[5]), [w6] "v"(w[6]), [w7] "v"(w[7]),
                       [w8] "v"(w[8]), [w9] "v"(w[9]));
        asm volatile(ISK_P3B(n1, a4)
                     ISK_OR3(A, A, w10, w11) ISK_OR3(B, B, w12, w13) ISK_OR3(A, A, w14, w15)
                     : [n1] "+v"(nw.t[1]), [A] "+v"(oA), [B] "+v"(oB)
                     : [a4] "v"(a[4]), [b] "v"(b), [s7] "v"(sc7), [so] "v"(sc_one), [w10] "v"(w[10]), [w11] "v"(w[11]), [w12] "v"(w[12]), [w13] "v"(w[13]),
                       [w14] "v"(w[14]), [w15] "v"(w[15]));
        asm volatile(ISK_P3C(n1, a5)
                     "v_bitop3_b32 %[R], %[A], %[B], %[ind] bitop3:0xa8\n"        // (A | B) & ind
                     "v_cmp_ne_u32_e64 %[mask], %[R], 0\n"
                     : [n1] "+v"(nw.t[1]), [R] "=&v"(rr), [mask] "=s"(mask)
                     : [a5] "v"(a[5]), [b] "v"(b), [s14] "v"(sc14), [so] "v"(sc_one), [A] "v"(oA), [B] "v"(oB), [ind] "s"(ind));
        return mask;
    };
    // the six MFMAs of a step's FIRST group (nothing to fold beside them), padded so that the first stage may read them
    auto first_group = [&](Acc& nw, const v4i& b) __attribute__((always_inline)) {
        asm volatile(ISK_P3A(n0, a0) ISK_P3B(n0, a1) ISK_P3C(n0, a2) ISK_P3A(n1, a3) ISK_P3B(n1, a4) ISK_P3C(n1, a5) "s_nop 7\ns_nop 3\n"
                     : [n0] "=&v"(nw.t[0]), [n1] "=&v"(nw.t[1])
                     : [a0] "v"(a[0]), [a1] "v"(a[1]), [a2] "v"(a[2]), [a3] "v"(a[3]), [a4] "v"(a[4]), [a5] "v"(a[5]), [b] "v"(b), [st] "v"(start),
                       [s7] "v"(sc7), [s14] "v"(sc14), [so] "v"(sc_one));
    };
    // the fold of a step's LAST group, no MFMA beside it (padded: the last stage's MFMAs may be just behind)
    auto last_fold = [&](const Acc& od, uint32_t ind) __attribute__((always_inline)) -> uint64_t {
        uint32_t oA, oB, rr;
        uint64_t mask;
        const v16f& u = od.t[0];
        const v16f& w = od.t[1];
        asm volatile("s_nop 7\ns_nop 3\n"
                     ISK_OR3(A, u0, u1, u2) ISK_OR3(B, u3, u4, u5) ISK_OR3(A, A, u6, u7) ISK_OR3(B, B, u8, u9)
                     ISK_OR3(A, A, u10, u11) ISK_OR3(B, B, u12, u13) ISK_OR3(A, A, u14, u15)
                     : [A] "=&v"(oA), [B] "=&v"(oB)
                     : [u0] "v"(u[0]), [u1] "v"(u[1]), [u2] "v"(u[2]), [u3] "v"(u[3]), [u4] "v"(u[4]), [u5] "v"(u[5]), [u6] "v"(u[6]), [u7] "v"(u[7]),
                       [u8] "v"(u[8]), [u9] "v"(u[9]), [u10] "v"(u[10]), [u11] "v"(u[11]), [u12] "v"(u[12]), [u13] "v"(u[13]), [u14] "v"(u[14]), [u15] "v"(u[15]));
        asm volatile(ISK_OR3(B, B, w0, w1) ISK_OR3(A, A, w2, w3) ISK_OR3(B, B, w4, w5) ISK_OR3(A, A, w6, w7)
                     ISK_OR3(B, B, w8, w9) ISK_OR3(A, A, w10, w11) ISK_OR3(B, B, w12, w13) ISK_OR3(A, A, w14, w15)
                     "v_bitop3_b32 %[R], %[A], %[B], %[ind] bitop3:0xa8\n"
                     "v_cmp_ne_u32_e64 %[mask], %[R], 0\n"
                     : [A] "+v"(oA), [B] "+v"(oB), [R] "=&v"(rr), [mask] "=s"(mask)
                     : [w0] "v"(w[0]), [w1] "v"(w[1]), [w2] "v"(w[2]), [w3] "v"(w[3]), [w4] "v"(w[4]), [w5] "v"(w[5]), [w6] "v"(w[6]), [w7] "v"(w[7]),
                       [w8] "v"(w[8]), [w9] "v"(w[9]), [w10] "v"(w[10]), [w11] "v"(w[11]), [w12] "v"(w[12]), [w13] "v"(w[13]), [w14] "v"(w[14]), [w15] "v"(w[15]),
                       [ind] "s"(ind));
        return mask;
    };

    const v4i* const lbl = lb + lane;
    // A step is 192 rows = 1.5 KB: lane L loads rows 2 L and 2 L + 1 (16 bytes, as mfma_pack_kernel) and row 128 + L (8 bytes);
    // v_permlane32_swap turns each pair of dwords into two tiles (see mfma_pack_kernel's load_rows):
    //   a[0]: rows 2 m, a[1]: 2 m + 64, a[2]: 2 m + 1, a[3]: 2 m + 65, a[4]: 128 + m, a[5]: 160 + m     (m = matrix row)
    struct Rows { u32x4 x; u32x2 y; };
    auto load_rows = [&](uint64_t st) __attribute__((always_inline)) -> Rows {
        const uint64_t row0 = p.row_begin + st * ROWS;
        if (row0 + ROWS <= p.n_rows)
            return Rows{__builtin_nontemporal_load(reinterpret_cast<const u32x4*>(col32 + row0 * 2) + lane),
                        __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(col32 + (row0 + 128) * 2) + lane)};
        const uint64_t r0 = row0 + 2 * lane, r1 = r0 + 1, r2 = row0 + 128 + lane;
        const uint2 lo = *reinterpret_cast<const uint2*>(col32 + (r0 <= last_row ? r0 : last_row) * 2);
        const uint2 hi = *reinterpret_cast<const uint2*>(col32 + (r1 <= last_row ? r1 : last_row) * 2);
        const uint2 th = *reinterpret_cast<const uint2*>(col32 + (r2 <= last_row ? r2 : last_row) * 2);
        return Rows{u32x4{lo.x, lo.y, hi.x, hi.y}, u32x2{th.x, th.y}};
    };
    auto expand = [&](const Rows& v) __attribute__((always_inline)) {
        const auto e = __builtin_amdgcn_permlane32_swap(v.x[0], v.x[1], false, false);
        const auto o = __builtin_amdgcn_permlane32_swap(v.x[2], v.x[3], false, false);
        const auto f = __builtin_amdgcn_permlane32_swap(v.y[0], v.y[1], false, false);
        a[0] = p3_rows(e[0]);
        a[1] = p3_rows(e[1]);
        a[2] = p3_rows(o[0]);
        a[3] = p3_rows(o[1]);
        a[4] = p3_rows(f[0]);
        a[5] = p3_rows(f[1]);
    };

    const bool refresh = MODE == MODE_SELF && mine4 && q0 + wave * 256 + lane * 4 < p.nq_pad;
    // the same number of steps between looks as mfma_pack_kernel (a step is 192 rows here, 128 there)
    const uint32_t refresh_mask = (groups >= 32 ? 1u : groups >= 16 ? 2u : groups >= 8 ? 4u : 8u) * ((p.refresh_steps + 1) / 2) - 1u;
    const uint32_t slices = groups * 32 * 4 / 64, nwaves = gridDim.x * (MBLOCK / 64);
    const uint32_t gw = blockIdx.x * (MBLOCK / 64) + wave_s;
    uint32_t trip = 0;
    Acc accX, accY;
    // odd group counts: a step's first group and last fold stand alone
    auto all_groups = [&]() __attribute__((always_inline)) {
        v4i by = lbl[0], bx = lbl[64];                    // groups > PK_DEEP_GROUPS
        const uint32_t tb = t_of(tcur), ind = ind_of(tcur);
        first_group(accY, by);
        uint32_t g = 0;
#pragma unroll 1
        for (; g + 2 < groups; g += 2) {
            by = lbl[(g + 2) * 64];
            if (const uint64_t mk = stage(accX, accY, bx, ind); __builtin_expect(mk != 0, 0)) save_hits(accY, mk, tb, g, step);
            const uint32_t g3 = g + 3 < groups ? g + 3 : g + 2;
            bx = lbl[g3 * 64];
            if (const uint64_t mk = stage(accY, accX, by, ind); __builtin_expect(mk != 0, 0)) save_hits(accX, mk, tb, g + 1, step);
        }
        if (g + 1 < groups) {
            if (const uint64_t mk = stage(accX, accY, bx, ind); mk != 0) save_hits(accY, mk, tb, g, step);
            if (const uint64_t mk = last_fold(accX, ind); mk != 0) save_hits(accX, mk, tb, g + 1, step);
        } else {
            if (const uint64_t mk = last_fold(accY, ind); mk != 0) save_hits(accY, mk, tb, g, step);
        }
    };
    // even group counts: the step's first stage folds the previous step's last group (carried in accX, made under tcar)
    bool carried = false;
    uint32_t tcar = 64;
    auto even_groups = [&](uint64_t prev) __attribute__((always_inline)) {
        v4i by = lbl[0], bx = lbl[64];
        const uint32_t tb = t_of(tcur), ind = ind_of(tcur);
        if (const uint64_t mk = stage(accY, accX, by, ind_of(tcar)); __builtin_expect(carried && mk != 0, 0)) { save_hits(accX, mk, t_of(tcar), groups - 1, prev); process_ring(prev); }
        uint32_t g = 0;
#pragma unroll 1
        for (; g + 2 < groups; g += 2) {
            by = lbl[(g + 2) * 64];
            if (const uint64_t mk = stage(accX, accY, bx, ind); __builtin_expect(mk != 0, 0)) save_hits(accY, mk, tb, g, step);
            bx = lbl[(g + 3) * 64];
            if (const uint64_t mk = stage(accY, accX, by, ind); __builtin_expect(mk != 0, 0)) save_hits(accX, mk, tb, g + 1, step);
        }
        if (const uint64_t mk = stage(accX, accY, bx, ind); __builtin_expect(mk != 0, 0)) save_hits(accY, mk, tb, g, step);
        carried = true;
        tcar = tcur;
    };
    auto even_flush = [&](uint64_t prev) __attribute__((always_inline)) {
        if (carried) {
            if (const uint64_t mk = last_fold(accX, ind_of(tcar)); mk != 0) { save_hits(accX, mk, t_of(tcar), groups - 1, prev); process_ring(prev); }
            carried = false;
        }
    };
    auto one_step = [&](auto&& body) __attribute__((always_inline)) {
        uint32_t fresh[4] = {0u, 0u, 0u, 0u};
        const bool look = trip < 4 || (trip & refresh_mask) == 0;
        const bool refresh_now = refresh && look;
        if constexpr (MODE == MODE_SELF) {
            if (look) update_t();                     // what the waves published at their last looks
        }
        body();
        if constexpr (MODE == MODE_SELF) pend_complete();
        if (rcount) process_ring(step);
        if constexpr (MODE == MODE_SELF) {
            // (the checkers' counters and the live thresholds are read HERE, not in flight during the step as in mfma_pack_kernel:
            //  registers through the stage loop are what the rare path inside it lacks; the other waves of the SIMD cover the wait)
            uint32_t chk_count = 0, chk_what = ~0u;   // chk_what: query in chunk | hamming level << 16, ~0: no task
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
            if (refresh_now) {
                const float* const src = p.thr_live + q0 + fresh_index();
#pragma unroll
                for (int i = 0; i < 4; ++i) fresh[i] = live_packed(src + i);
            }
            if (chk_what != ~0u && chk_count >= p.k) {
                const uint32_t ql = chk_what & 0xFFFFu;
                atomicMin(reinterpret_cast<uint32_t*>(p.thr_live) + q0 + ql, pack_threshold((int)(chk_what >> 16) - lpop[ql]));
            }
            if (refresh_now) *reinterpret_cast<uint4*>(lthr + fresh_index()) = make_uint4(fresh[0], fresh[1], fresh[2], fresh[3]);
            if (look) publish_max(fresh, refresh_now);
        }
    };
    Rows x = load_rows(step);
    if constexpr (ODD) {
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
    if constexpr (MODE == MODE_SELF) pend_complete();
}

#undef ISK_P3A
#undef ISK_P3B
#undef ISK_P3C
#undef ISK_OR3

}  // namespace isk
