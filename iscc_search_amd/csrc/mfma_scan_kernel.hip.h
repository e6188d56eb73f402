// mfma_scan_kernel.hip.h -- mfma_scan_kernel: the matrix-core scan for codes of one to four words, one dot product per f32
// accumulator register, folded with v_min3_f32 (included by mfma_scan.hip, whose file comment describes the method).
#pragma once

#include "mfma_common.hip.h"

namespace isk {

// Registers decide: the rare emit path (both accumulator sets live + 64-bit row numbers) peaks at 130-175 VGPRs, i.e. three
// waves per SIMD for W <= 3 and two for W = 4.  Forcing four (128 VGPRs) spilled to scratch; the prototype measured
// 3.22 ms with three resident blocks against 3.15 ms with four (profiles/r02_proto_mfma_scan.txt) -- not worth a spill.
template <int W> constexpr int mfma_min_waves() { return W <= 3 ? 3 : 2; }
constexpr int FP4 = 4;                // cbsz / blgp format code of e2m1
// Both scale operands constant 0: hipcc then selects the UNSCALED encoding, v_mfma_f32_32x32x64_f8f6f4 (no
// v_mfma_ld_scale prefix, no scale VGPRs), which multiplies as with block scales 2^0.  Same bits as the scaled form with
// E8M0 scales 0x7F (both checked against a brute-force kernel: tools/proto_mfma_scan.hip, -DPROTO_SCALE=0) and 6 % faster
// (3.10 vs 3.30 ms per 100 M x 1 024 pass): one instruction less to issue per MFMA.
constexpr int SCALE_ONE = 0;

// LDS image of a chunk: B fragments [groups][W][64] v4i | thr[groups * 32] (float) | popc[groups * 32]
template <int W, int MODE>
__global__ __launch_bounds__(MBLOCK, mfma_min_waves<W>()) void mfma_scan_kernel(const ScanParams p, const uint32_t groups) {
    constexpr int MT = 2;       // row tiles (32 rows) per wave and step: the two share every B fragment, threshold read and compare
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    v4i* lb = reinterpret_cast<v4i*>(smem);
    float* lthr = reinterpret_cast<float*>(smem + (size_t)groups * W * 64 * 16);
    int* lpop = reinterpret_cast<int*>(lthr + groups * 32);
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t r = lane & 31, h = lane >> 5;
    const uint32_t q0 = blockIdx.y * groups * 32;       // first query of this block's chunk

    // prologue: expand the chunk's queries to +1 / -1 nibbles (0 beyond the compared prefix and for padding queries)
    for (uint32_t i = tid; i < groups * 32 * 2 * W; i += MBLOCK) {
        const uint32_t ql = i / (2 * W), rest = i % (2 * W), w = rest >> 1, hh = rest & 1;
        const uint32_t q = q0 + ql;
        const bool live = q < p.nq_pad;
        const uint64_t qw = live ? p.queries[(uint64_t)q * 4 + w] : 0;
        const uint32_t x = hh ? (uint32_t)(qw >> 32) : (uint32_t)qw;
        uint32_t m = live ? 0xFFFFFFFFu : 0u;
        if (w == W - 1) m &= hh ? p.mask_hi : p.mask_lo;
        const uint32_t g = ql >> 5, c = ql & 31;
        v4i frag;
#pragma unroll
        for (int j = 0; j < 4; ++j) frag[j] = (int)((0x22222222u | (nibbles(x, j) << 3)) & (nibbles(m, j) * 0xFu));   // bit ? -1 : +1, masked: 0
        lb[((size_t)g * W + w) * 64 + hh * 32 + c] = frag;
    }
    for (uint32_t ql = tid; ql < groups * 32; ql += MBLOCK) {
        const uint32_t q = q0 + ql;
        int pc = 0, tau = -1;
        if (q < p.nq_pad) {
#pragma unroll
            for (int w = 0; w < W; ++w) {
                uint64_t qw = p.queries[(uint64_t)q * 4 + w];
                if (w == W - 1) qw &= ((uint64_t)p.mask_hi << 32) | p.mask_lo;
                pc += __popcll(qw);
            }
            tau = (int)(0x7FFFFFFFu - p.bias[q]);       // BIAS_NEVER -> -1: no row can be a candidate
        }
        lpop[ql] = pc;
        if constexpr (MODE == MODE_SELF) lthr[ql] = q < p.nq_pad ? live_threshold(p.thr_live + q) : -1.0e9f;
        else lthr[ql] = (float)(tau - pc);              // hamming <= tau  <=>  dot <= tau - popc(q)
    }
    __syncthreads();

    const uint64_t first = p.row_begin / (32 * MT);                         // row_begin is a multiple of 64
    const uint64_t nsteps = (p.n_rows + 32 * MT - 1) / (32 * MT);           // the last step may be partial
    const uint64_t stride = (uint64_t)gridDim.x * (MBLOCK / 64);
    // W >= 2: the wave number is read as a SCALAR, so that the step number and the row addresses live on the scalar unit
    // (scalar-base loads) instead of ~14 vector instructions of 64-bit address arithmetic per step.  Same box, A/B: 128-bit
    // 4.586 against 4.605 ms per 1 024 queries and 0.57-0.59 against 0.615 ms per 64; 256-bit 9.20 against 9.36 and no change
    // at 64 queries.  Not for 64-bit codes: nothing at 1 024 queries and 17-64 queries measured 15-20 % slower.
    constexpr bool SCALAR_STEPS = W >= 2;
    const uint32_t wave_u = SCALAR_STEPS ? (uint32_t)__builtin_amdgcn_readfirstlane((int)wave) : wave;
    uint64_t step = first + (uint64_t)blockIdx.x * (MBLOCK / 64) + wave_u;
    if (step >= nsteps) return;
    const uint64_t last_row = p.n_rows - 1;

    const uint32_t* col32[W];
#pragma unroll
    for (int w = 0; w < W; ++w) col32[w] = reinterpret_cast<const uint32_t*>(p.col[w]);

    static_assert(MT == 2, "the candidate ring holds the two tiles' 32 results of a lane");
    // ---- candidates: as in mfma_pack_kernel -- the lanes that hold a result within their query's threshold copy their
    // 32 results (+ query, threshold) into their wave's LDS ring and the stage loop goes on; at the end of the step the ring is
    // walked with a real loop, TWO saved blocks per trip, lane v on result v & 31 of block v >> 5.  MODE_SELF: the list slot is
    // consumed at the lane's next candidate or at the end of the next step, the distance counts are no-return atomics, and
    // CHECKER lanes notice "k rows within t" (one counter read per look) and lower the live threshold.  (Round 2: 32 unrolled
    // compares and two returned atomics + a dependent chain per candidate inside the stage loop: config 5's table -- 10 M x
    // 128-bit, 512 queries, k = 400 -- scanned at 0.94 ms against 0.22 ms of matrix-pipe time.)
    constexpr uint32_t RING_E = PK_RING_ENTRIES, ENTRY = PK_RING_ENTRY_DWORDS;
    uint32_t* const ring = reinterpret_cast<uint32_t*>(lpop + groups * 32) + wave * (RING_E * ENTRY);
    uint32_t rcount = 0;
    uint32_t pend_slot = 0, pend_lo = 0, pend_hi = 0x80000000u;        // pend_hi bit 31: nothing pending
    auto pend_complete = [&]() {
        if (!(pend_hi & 0x80000000u)) {
            const uint32_t qi = q0 + (pend_hi >> 21);                   // query in chunk : 10 | hamming : 9 | row >> 32 : 12
            if (pend_slot < p.cap) p.cand[(uint64_t)qi * p.cap + pend_slot] = ((uint64_t)((pend_hi >> 12) & 0x1FFu) << 48) | ((uint64_t)(pend_hi & 0xFFFu) << 32) | pend_lo;
            pend_hi = 0x80000000u;
        }
    };
    auto process_ring = [&](uint64_t st) {
        const uint32_t sub = lane >> 5, ri = lane & 31;
        const uint32_t off0 = (ri >> 4) * 32 + (ri & 3) + 8 * ((ri & 15) >> 2);
        for (uint32_t e = 0; e < rcount; e += 2) {
            if (e + sub < rcount) {
                const uint32_t* const blk = ring + (e + sub) * ENTRY;
                const float v = __uint_as_float(blk[ri]), thr = __uint_as_float(blk[33]);
                const uint32_t head = blk[32], ql = head & 0xFFFFu;
                const uint64_t row = st * (32 * MT) + off0 + 4 * (head >> 16);
                if (v <= thr && row <= last_row) {
                    const int pc = lpop[ql];
                    const uint32_t hd = (uint32_t)((int)v + pc);
                    if constexpr (MODE == MODE_SELF) {
                        pend_complete();
                        const uint32_t qi = q0 + ql;
                        const int tau_seen = (int)thr + pc;
                        pend_slot = atomicAdd(&p.cnt[(uint64_t)qi * CNT_STRIDE], 1u);
                        uint32_t* const counts = p.ghist + (uint64_t)qi * HB;
                        for (int t = (int)hd; t < tau_seen; ++t) __hip_atomic_fetch_add(&counts[t], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        pend_lo = (uint32_t)row;
                        pend_hi = (ql << 21) | (hd << 12) | (uint32_t)(row >> 32);       // rows < 2^44
                    } else {
                        emit<MODE>(p, q0 + ql, hd, row);
                    }
                }
            }
        }
        rcount = 0;
    };
    // `mask`: the lanes whose minimum is within their threshold (query g * 32 + (lane & 31), rows 4 * (lane >> 5) + ... of the tiles)
    auto save_hits = [&](const Acc& acc, uint64_t mask, float thr, uint32_t g, uint64_t st) {
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
                *reinterpret_cast<uint2*>(blk + 32) = make_uint2((g * 32 + r) | (h << 16), __float_as_uint(thr));
            }
            const uint64_t taken = __builtin_amdgcn_ballot_w64(mine);
            rcount += (uint32_t)__builtin_popcountll(taken);
            mask &= ~taken;
        }
    };
    // The fold is builtins that hipcc schedules around the MFMAs.  (The stage of two to four words as single asm statements in
    // issue order, as in mfma_pack_kernel, measured 2-4 % slower: with 2 W MFMAs per 17 fold instructions the matrix pipe, not
    // the issue order, is the bound -- profiles/r03_ab_ordered_stage.txt.)
    auto rare = [&](const Acc& acc, float thr, uint32_t g, uint64_t st, float mall) {
        const uint64_t mask = __builtin_amdgcn_ballot_w64(mall <= thr);
        if (__builtin_expect(mask != 0, 0)) save_hits(acc, mask, thr, g, st);
    };
    auto reduce = [&](const Acc& acc, float thr, uint32_t g, uint64_t st) {
        float m[MT];
#pragma unroll
        for (int t = 0; t < MT; ++t) m[t] = min3f(acc.t[t][0], acc.t[t][1], acc.t[t][2]);
#pragma unroll
        for (int i = 3; i < 15; i += 2)
#pragma unroll
            for (int t = 0; t < MT; ++t) m[t] = min3f(m[t], acc.t[t][i], acc.t[t][i + 1]);
        rare(acc, thr, g, st, fminf(min3f(m[0], acc.t[0][15], acc.t[1][15]), m[1]));
    };

    const v16f zero = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    v8i a[MT][W];     // only the first four dwords carry FP4 data; the instruction ignores the rest
    // one word of one group: one MFMA per tile into the group's accumulators
    auto mm = [&](Acc& acc, int w, const v4i& b) {
        const v8i b8 = {b[0], b[1], b[2], b[3], 0, 0, 0, 0};
#pragma unroll
        for (int t = 0; t < MT; ++t)
            acc.t[t] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a[t][w], b8, w == 0 ? zero : acc.t[t], FP4, FP4, 0, SCALE_ONE, 0, SCALE_ONE);
    };
    // An empty asm naming BOTH accumulator sets right after the first MFMAs of the next group: the fold of the previous
    // group then depends on it, so hipcc can neither hoist that fold above the MFMAs nor give the two sets the same
    // registers (it did both in the prototype and serialised MFMA -> s_nop 10 -> fold).
    auto pin2 = [&](Acc& x, Acc& y) { asm volatile("" : "+v"(x.t[0]), "+v"(x.t[1]), "+v"(y.t[0]), "+v"(y.t[1])); };
    const v4i* lbl = lb + lane;
    const float* lt = lthr + r;
    auto row_of = [&](uint64_t st, int t) { const uint64_t row = (st * MT + t) * 32 + r; return row <= last_row ? row : last_row; };

    // the rows of step `st`: lane (r, h) of tile t reads dword h of row st * 32 MT + 32 t + r.  SCALAR_STEPS: a uniform base plus a
    // constant per-lane offset; only the table's last step can be partial and clamps per lane as the general form does
    const uint32_t lane_dword = r * 2 + h;
    auto load_rows = [&](uint64_t st, uint32_t (&dst)[MT][W]) {
        if (SCALAR_STEPS && (st + 1) * (32 * MT) <= p.n_rows) {
#pragma unroll
            for (int t = 0; t < MT; ++t)
#pragma unroll
                for (int w = 0; w < W; ++w) dst[t][w] = (col32[w] + st * (64 * MT) + t * 64)[lane_dword];
        } else {
#pragma unroll
            for (int t = 0; t < MT; ++t)
#pragma unroll
                for (int w = 0; w < W; ++w) dst[t][w] = col32[w][row_of(st, t) * 2 + h];
        }
    };
    uint32_t x[MT][W], xn[MT][W];
    load_rows(step, x);
    // MODE_SELF: wave w keeps the block's copy of thresholds [256 w, 256 w + 256) fresh -- requested here, written to LDS
    // after the group loop, picked up by all four waves from their next step on (a stale threshold is only a looser one)
    // (the lane's slice of the thresholds is RECOMPUTED at each use -- mbcnt of a laundered zero -- or hipcc keeps a 64-bit global
    //  address and an LDS address alive through the group loop: registers the 192-bit kernel does not have)
    const uint32_t wave_sc = (uint32_t)__builtin_amdgcn_readfirstlane((int)wave);
    auto fresh_index = [&]() {
        uint32_t z = 0;
        asm volatile("" : "+v"(z));
        return wave_sc * 256 + __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, z)) * 4;
    };
    const bool refresh = MODE == MODE_SELF && wave * 256 + lane * 4 < groups * 32 && q0 + wave * 256 + lane * 4 < p.nq_pad;   // nq_pad is a multiple of 8
    // ... every `refresh_steps` steps when the chunk is full (32 groups), proportionally less often for smaller chunks
    const uint32_t refresh_mask = (groups >= 32 ? 1u : groups >= 16 ? 2u : groups >= 8 ? 4u : groups >= 4 ? 8u : 16u) * p.refresh_steps - 1u;
    uint32_t trip = 0;
    for (; step < nsteps; step += stride, ++trip) {
        const uint64_t ns = step + stride < nsteps ? step + stride : step;
        float fresh[4] = {0.f, 0.f, 0.f, 0.f};
        // (a wave's first steps always look: all waves start under the bootstrap threshold at once, and until the first update
        //  arrives every row within it is appended -- a 4 M-row table would be scanned whole under it at 16 steps per look)
        const bool look = trip < 8 || (trip & refresh_mask) == 0;
        const bool refresh_now = refresh && look;                             // (MODE_SELF only: `refresh` is false otherwise)
        uint32_t chk_count = 0, chk_what = ~0u;       // chk_what: query in chunk | hamming level << 16, ~0: no task
        if constexpr (MODE == MODE_SELF) {
            if (refresh_now) {
                const float* const src = p.thr_live + q0 + fresh_index();
#pragma unroll
                for (int i = 0; i < 4; ++i) fresh[i] = live_threshold(src + i);
            }
            // checkers: task (query, j) reads count[q][tau_q - j], j = 1..4 (see mfma_pack_kernel)
            const uint32_t slices = groups * 32 * 4 / 64, nwaves = gridDim.x * (MBLOCK / 64);
            const uint32_t gw = blockIdx.x * (MBLOCK / 64) + wave_sc;
            const uint32_t slice = nwaves >= slices ? gw : (gw + trip * nwaves) % slices;
            if (look && slice < slices) {
                const uint32_t task = slice * 64 + lane, ql = task >> 2;
                const float thr = lthr[ql];
                const int level = (int)thr + lpop[ql] - 1 - (int)(task & 3);
                if (thr > -1.0e8f && level >= 0 && q0 + ql < p.nq_pad) {
                    chk_what = ql | ((uint32_t)level << 16);
                    chk_count = (uint32_t)__hip_atomic_load(reinterpret_cast<const int*>(p.ghist + (uint64_t)(q0 + ql) * HB + level), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
        }
        load_rows(ns, xn);                                                          // next step's rows, in flight during this one
#pragma unroll
        for (int t = 0; t < MT; ++t)
#pragma unroll
            for (int w = 0; w < W; ++w)
                a[t][w] = v8i{(int)(nibbles(x[t][w], 0) << 1), (int)(nibbles(x[t][w], 1) << 1), (int)(nibbles(x[t][w], 2) << 1),
                              (int)(nibbles(x[t][w], 3) << 1), 0, 0, 0, 0};                      // bit ? 1.0 (0x2) : 0

        // Software pipeline over the (group, word) sequence: two B buffers (one word each) and two accumulator sets.
        // The fragment of the NEXT word is requested right after the MFMAs of the current one are issued (its buffer
        // was consumed one stage earlier), and the results of group g are folded while the MFMAs of group g + 1 run.
        v4i bx = lbl[0], by = lbl[0];
        Acc accX, accY;
        float thrX = 0.f, thrY = lt[0];
        // stage(w): consume one buffer, prefetch fragment `nxt` (counted from the pair's base pointer, so that the offsets
        // are immediates of the ds_read and one pointer increment serves two groups) into the other one
        auto stage = [&](Acc& acc, lds_frag_ptr base, int nxt, int w, bool y_buf, bool more) {
            if (y_buf) {
                mm(acc, w, by);
                if (more) bx = base[nxt * 64];
            } else {
                mm(acc, w, bx);
                if (more) by = base[nxt * 64];
            }
        };
        // group 0
#pragma unroll
        for (int w = 0; w < W; ++w) stage(accY, (lds_frag_ptr)lbl, w + 1, w, (w & 1) == 0, true);
        // LDS addresses of the pair (g, g + 1): 32-bit pointers advanced by hand and laundered, or hipcc rebuilds both
        // from g with a shift-add per group (two more vector instructions per pair in a loop that is issue-bound)
        lds_frag_ptr lg = (lds_frag_ptr)lbl + W * 64;
        lds_thr_ptr ltg = (lds_thr_ptr)lt + 32;
#pragma unroll 1
        for (uint32_t g = 1; g + 1 < groups; g += 2, lg += 2 * W * 64, ltg += 64) {
            asm volatile("" : "+v"(lg), "+v"(ltg));
            // odd group g -> accX; its first word sits in buffer parity (W & 1): Y when W is even
            thrX = ltg[0];
#pragma unroll
            for (int w = 0; w < W; ++w) {
                stage(accX, lg, w + 1, w, ((W + w) & 1) == 0, true);
                if (w == 0) { pin2(accX, accY); reduce(accY, thrY, g - 1, step); }
            }
            // even group g + 1 -> accY; (2 * W + w) & 1 == w & 1
            thrY = ltg[32];
#pragma unroll
            for (int w = 0; w < W; ++w) {
                stage(accY, lg, W + w + 1, w, (w & 1) == 0, true);
                if (w == 0) { pin2(accY, accX); reduce(accX, thrX, g, step); }
            }
        }
        // last (odd) group: nothing further to prefetch after its last word
        {
            const uint32_t g = groups - 1;
            thrX = ltg[0];
#pragma unroll
            for (int w = 0; w < W; ++w) {
                stage(accX, lg, w + 1, w, ((W + w) & 1) == 0, w + 1 < W);
                if (w == 0) { pin2(accX, accY); reduce(accY, thrY, g - 1, step); }
            }
            reduce(accX, thrX, g, step);
        }
#pragma unroll
        for (int t = 0; t < MT; ++t)
#pragma unroll
            for (int w = 0; w < W; ++w) x[t][w] = xn[t][w];
        // what the PREVIOUS step's appends returned (issued a whole step ago: no wait), then this step's saved blocks
        if constexpr (MODE == MODE_SELF) pend_complete();
        if (rcount) process_ring(step);
        if constexpr (MODE == MODE_SELF) {
            if (chk_what != ~0u && chk_count >= p.k) {
                const uint32_t ql = chk_what & 0xFFFFu;
                lower_threshold(p.thr_live + q0 + ql, (float)((int)(chk_what >> 16) - lpop[ql]));
            }
            if (refresh_now) *reinterpret_cast<float4*>(lthr + fresh_index()) = make_float4(fresh[0], fresh[1], fresh[2], fresh[3]);
        }
    }
    if constexpr (MODE == MODE_SELF) pend_complete();
}

}  // namespace isk
