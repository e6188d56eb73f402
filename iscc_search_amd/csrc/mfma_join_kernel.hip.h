// mfma_join_kernel.hip.h -- mfma_join_kernel: the index joins (isccsearch_join_within / isccsearch_join_between) on the matrix
// cores (included by mfma_scan.hip, whose file comment describes the arithmetic).
//
// mfma_scan_kernel with a fixed threshold, its queries taken from a table: a block HOLDS a chunk of rows of one segment in LDS
// (B fragments, +1 / -1 nibbles, 0 past the compared prefix; per row tau - popc(row) and popc(row)) and its waves STREAM the other
// segment, two 32-row tiles per wave and step, the next step's rows in flight.  One tau per launch: no k, no live thresholds,
// no checkers, no select.
//   grid = (blocks of streamed steps, chunks of this launch); chunk = p.chunk_base + blockIdx.y, so that a segment of more
//   than 65 535 chunks takes several launches.
//   The prologue reads the held rows straight from the segment's word-major columns.  Held rows past the segment's count get zero
//   fragments and a threshold no sum reaches; the last streamed step is clamped to the last row and its repeats are dropped
//   in the emit path: nothing stored behind a segment's end becomes a pair.
//   Within one segment (p.same) chunk c streams from the 64-row step that contains its first row and the emit path keeps only
//   row_streamed > row_held: every unordered pair exactly once.  A chunk late in the segment has few steps left; the blocks
//   that would run none return before the prologue (mfma_join_live_blocks: JOIN_STEPS_PER_WAVE steps per wave).
//   Hits go through the per-wave LDS ring of saved accumulator blocks as in mfma_scan_kernel.  The ring walk (`process_ring`) is this
//   kernel's emit path; join.hip.h's file comment describes the forms F and CROSS once for both kernels.  The held side takes the part
//   the SGPR side has in join_scan_kernel (JoinEmit::keys_a, labels_a, sgpr_side_is_b).  PAIRS and OVERLAP walk the ring twice (count,
//   ONE returned atomic on JoinEmit::total for the walk, write; each walk rcount / 2 <= RING_E / 2 trips; LIVE is PAIRS with live_pair
//   asked in both walks), LINK once.
//   DEGREE walks once too and issues no global atomic per pair: the held rows of the chunk are counted in an LDS array of groups * 32
//   counters behind the rings (one LDS add per saved block: its 32 results belong to one held row), flushed to JoinEmit::degree
//   when the block has streamed its last step -- so no wave of a DEGREE block returns before that barrier --, and the streamed rows
//   of the step in two registers per lane, folded across the wave's halves: at most one global atomic per streamed row and walk.
#pragma once

#include "join.hip.h"
#include "mfma_common.hip.h"
#include "mfma_scan_kernel.hip.h"

namespace isk {

// LDS image of a chunk: B fragments [groups][W][64] v4i | thr[groups * 32] (float) | popc[groups * 32] | the waves' rings
// | DEGREE only: degree[groups * 32] (mfma_join_lds_bytes)
template <int W, JoinForm F, bool CROSS>
__global__ __launch_bounds__(MBLOCK, mfma_min_waves<W>()) void mfma_join_kernel(const MfmaJoinParams p, const uint32_t groups) {
    static_assert(join_form_exists(F, CROSS), "no such join form");
    constexpr bool LINK = F == JoinForm::LINK, OVERLAP = F == JoinForm::OVERLAP, DEGREE = F == JoinForm::DEGREE, LIVE = F == JoinForm::LIVE;
    constexpr int MT = 2;       // row tiles (32 rows) per wave and step
    constexpr uint32_t WAVES = MBLOCK / 64;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    v4i* lb = reinterpret_cast<v4i*>(smem);
    float* lthr = reinterpret_cast<float*>(smem + (size_t)groups * W * 64 * 16);
    int* lpop = reinterpret_cast<int*>(lthr + groups * 32);
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t r = lane & 31, h = lane >> 5;
    const uint64_t q0 = (p.chunk_base + blockIdx.y) * (uint64_t)(groups * 32);       // first held row of this block's chunk

    // the steps of this chunk, and the blocks that share them: a block without a step returns before the prologue
    const uint64_t nsteps = (p.n_s + 32 * MT - 1) / (32 * MT);           // the last step may be partial
    const uint64_t first = p.same ? q0 / (32 * MT) : 0;                  // (a chunk is a multiple of 64 rows)
    if (q0 >= p.n_q || first >= nsteps) return;
    const uint32_t live_blocks = mfma_join_live_blocks(nsteps - first, gridDim.x);
    if (blockIdx.x >= live_blocks) return;

    // prologue: expand the chunk's rows to +1 / -1 nibbles (0 beyond the compared prefix and for rows past the segment's count)
    for (uint32_t i = tid; i < groups * 32 * 2 * W; i += MBLOCK) {
        const uint32_t ql = i / (2 * W), rest = i % (2 * W), w = rest >> 1, hh = rest & 1;
        const uint64_t q = q0 + ql;
        const bool live = q < p.n_q;
        const uint64_t qw = live ? p.col_q[w][q] : 0;
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
        const uint64_t q = q0 + ql;
        int pc = 0;
        float thr = -1.0e9f;                             // rows past the count: no sum reaches it
        if (q < p.n_q) {
#pragma unroll
            for (int w = 0; w < W; ++w) {
                uint64_t qw = p.col_q[w][q];
                if (w == W - 1) qw &= ((uint64_t)p.mask_hi << 32) | p.mask_lo;
                pc += __popcll(qw);
            }
            thr = (float)((int)p.tau - pc);              // hamming <= tau  <=>  dot <= tau - popc(held row)
        }
        lpop[ql] = pc;
        lthr[ql] = thr;
    }
    // DEGREE: the chunk's counters, behind the rings
    uint32_t* const ldeg = DEGREE ? reinterpret_cast<uint32_t*>(lpop + groups * 32) + WAVES * (PK_RING_ENTRIES * PK_RING_ENTRY_DWORDS) : nullptr;
    if (DEGREE)
        for (uint32_t ql = tid; ql < groups * 32; ql += MBLOCK) ldeg[ql] = 0;
    __syncthreads();

    const uint64_t stride = (uint64_t)live_blocks * WAVES;
    // W >= 2: the step number and the row addresses on the scalar unit, as in mfma_scan_kernel
    constexpr bool SCALAR_STEPS = W >= 2;
    const uint32_t wave_u = SCALAR_STEPS ? (uint32_t)__builtin_amdgcn_readfirstlane((int)wave) : wave;
    uint64_t step = first + (uint64_t)blockIdx.x * WAVES + wave_u;
    if (!DEGREE && step >= nsteps) return;      // (DEGREE: a wave without a step runs no trip of the step loop and waits at the flush)
    const uint64_t last_row = p.n_s - 1;

    const uint32_t* col32[W];
#pragma unroll
    for (int w = 0; w < W; ++w) col32[w] = reinterpret_cast<const uint32_t*>(p.col_s[w]);

    static_assert(MT == 2, "the ring holds the two tiles' 32 results of a lane");
    // ---- pairs: the lanes that hold a result within their held row's threshold copy their 32 results (+ held row, threshold)
    // into their wave's LDS ring and the stage loop goes on; at the end of the step (or when the ring is full) the ring is walked
    // TWICE, two saved blocks per trip, lane v on result v & 31 of block v >> 5: count, one atomic for the wave, write.
    constexpr uint32_t RING_E = PK_RING_ENTRIES, ENTRY = PK_RING_ENTRY_DWORDS;
    uint32_t* const ring = reinterpret_cast<uint32_t*>(lpop + groups * 32) + wave * (RING_E * ENTRY);
    uint32_t rcount = 0;
    auto process_ring = [&](uint64_t st) {
        const uint32_t sub = lane >> 5, ri = lane & 31;
        const uint32_t off0 = (ri >> 4) * 32 + (ri & 3) + 8 * ((ri & 15) >> 2);
        // result `ri` of saved block `en`: is it a pair?  (i: held row, j: streamed row, hd: distance)
        auto pair_at = [&](uint32_t en, uint64_t& i, uint64_t& j, uint32_t& hd) {
            if (en >= rcount) return false;
            const uint32_t* const blk = ring + en * ENTRY;
            const float v = __uint_as_float(blk[ri]), thr = __uint_as_float(blk[33]);
            const uint32_t head = blk[32], ql = head & 0xFFFFu;
            i = q0 + ql;
            j = st * (32 * MT) + off0 + 4 * (head >> 16);
            hd = (uint32_t)((int)v + lpop[ql]);
            return v <= thr && j <= last_row && (CROSS || !p.same || j > i);
        };
        uint32_t c = 0;
        if (DEGREE) {                              // one walk, nothing written: LDS adds for the held rows, two registers for the streamed rows
            const JoinEmit& e = *p.e;
            // the lane's two streamed rows of this step (pair_at: head >> 16 is 0 or 1) and their labels
            const uint64_t j0 = st * (32 * MT) + off0;
            const uint32_t lb0 = j0 <= last_row ? e.labels_b[j0] : UF_NONE, lb1 = j0 + 4 <= last_row ? e.labels_b[j0 + 4] : UF_NONE;
            uint32_t c0 = 0, c1 = 0;
            for (uint32_t en = 0; en < rcount; en += 2) {
                uint64_t i = q0, j = j0;            // (pair_at leaves them alone past the ring's count)
                uint32_t hd;
                const bool pair = pair_at(en + sub, i, j, hd);
                const bool upper = j != j0;
                const bool both = pair && (upper ? lb1 : lb0) != UF_NONE && e.labels_a[i] != UF_NONE;
                // the 32 results of a saved block are of ONE held row: one LDS add per block, by the first lane of its half
                const uint64_t hits = __builtin_amdgcn_ballot_w64(both);
                const uint32_t of_block = (uint32_t)__builtin_popcount((uint32_t)(hits >> (32 * sub)));
                if (ri == 0 && of_block != 0) atomicAdd(ldeg + (uint32_t)(i - q0), of_block);
                c0 += both && !upper ? 1u : 0u;
                c1 += both && upper ? 1u : 0u;
            }
            c = c0 + c1;
            // lanes v and v + 32 hold the same two streamed rows: fold, the lower half adds
            c0 += (uint32_t)__shfl_xor((int)c0, 32, 64);
            c1 += (uint32_t)__shfl_xor((int)c1, 32, 64);
            if (sub == 0) {
                if (c0 != 0) atomicAdd(e.degree + lb0, c0);
                if (c1 != 0) atomicAdd(e.degree + lb1, c1);
            }
            const uint32_t counted = wave_sum(c);
            if (counted != 0 && lane == 0) atomicAdd(e.total, (unsigned long long)counted);
            rcount = 0;
            return;
        }
        if (LINK) {                                // one walk: the labelled pairs are united as they are counted, nothing is written
            const JoinEmit& e = *p.e;
            for (uint32_t en = 0; en < rcount; en += 2) {
                uint64_t i, j;
                uint32_t hd;
                if (pair_at(en + sub, i, j, hd)) c += link_pair(e, i, j);
            }
            const uint32_t linked = wave_sum(c);
            if (linked != 0 && lane == 0) atomicAdd(e.total, (unsigned long long)linked);
            rcount = 0;
            return;
        }
        if (OVERLAP) {                             // two walks (each rcount / 2 <= RING_E / 2 trips): count the pairs of two different labels, one atomic, write their hits
            const JoinEmit& e = *p.e;
            for (uint32_t en = 0; en < rcount; en += 2) {
                uint64_t i, j;
                uint32_t hd, la, lb;
                c += pair_at(en + sub, i, j, hd) && overlap_pair<CROSS>(e, i, j, la, lb) ? 1u : 0u;
            }
            uint64_t slot;
            if (overlap_slots(e, c, lane, slot)) {
                for (uint32_t en = 0; c != 0 && en < rcount; en += 2) {
                    uint64_t i, j;
                    uint32_t hd, la, lb;
                    if (!pair_at(en + sub, i, j, hd) || !overlap_pair<CROSS>(e, i, j, la, lb)) continue;
                    overlap_write(e, slot, la, lb, i, j, hd);
                    ++slot;
                }
            }
            rcount = 0;
            return;
        }
        for (uint32_t en = 0; en < rcount; en += 2) {
            uint64_t i, j;
            uint32_t hd;
            c += pair_at(en + sub, i, j, hd) && (!LIVE || live_pair(*p.e, i, j)) ? 1u : 0u;
        }
        // wave-inclusive prefix of the counts; lane 63 holds the walk's total
        uint32_t incl = c;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t t = (uint32_t)__shfl_up((int)incl, d, 64);
            if (lane >= (uint32_t)d) incl += t;
        }
        const uint32_t walk_total = (uint32_t)__shfl((int)incl, 63, 64);
        if (walk_total != 0) {                     // (0: only non-pairs passed -- the diagonal, the clamped last step)
            const JoinEmit& e = *p.e;
            uint32_t lo = 0, hi = 0;
            if (lane == 0) {
                const unsigned long long b = atomicAdd(e.total, (unsigned long long)walk_total);
                lo = (uint32_t)b; hi = (uint32_t)(b >> 32);
            }
            uint64_t slot = ((uint64_t)(uint32_t)__shfl((int)hi, 0, 64) << 32 | (uint32_t)__shfl((int)lo, 0, 64)) + (incl - c);
            const uint32_t kw = e.kw;
            for (uint32_t en = 0; c != 0 && en < rcount; en += 2) {
                uint64_t i, j;
                uint32_t hd;
                if (!pair_at(en + sub, i, j, hd)) continue;
                if (LIVE && !live_pair(e, i, j)) continue;
                if (slot < e.capacity) {
                    uint64_t ka_hi = kw == 2 ? e.keys_a[i * 2] : 0, ka_lo = e.keys_a[i * kw + kw - 1];
                    uint64_t kb_hi = kw == 2 ? e.keys_b[j * 2] : 0, kb_lo = e.keys_b[j * kw + kw - 1];
                    if (CROSS ? e.sgpr_side_is_b != 0 : kb_hi < ka_hi || (kb_hi == ka_hi && kb_lo < ka_lo)) {
                        uint64_t t = ka_hi; ka_hi = kb_hi; kb_hi = t;
                        t = ka_lo; ka_lo = kb_lo; kb_lo = t;
                    }
                    if (kw == 2) { e.out_keys_a[slot * 2] = ka_hi; e.out_keys_b[slot * 2] = kb_hi; }
                    e.out_keys_a[slot * kw + kw - 1] = ka_lo;
                    e.out_keys_b[slot * kw + kw - 1] = kb_lo;
                    e.out_hamming[slot] = hd;
                    e.out_prefix_bits[slot] = (uint16_t)e.prefix_bits;
                }
                ++slot;
            }
        }
        rcount = 0;
    };
    // `mask`: the lanes whose minimum is within their threshold (held row g * 32 + (lane & 31), rows 4 * (lane >> 5) + ... of the tiles)
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
    // the fold is builtins that hipcc schedules around the MFMAs (and whose hazards it places), as in mfma_scan_kernel
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
    auto mm = [&](Acc& acc, int w, const v4i& b) {
        const v8i b8 = {b[0], b[1], b[2], b[3], 0, 0, 0, 0};
#pragma unroll
        for (int t = 0; t < MT; ++t)
            acc.t[t] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a[t][w], b8, w == 0 ? zero : acc.t[t], FP4, FP4, 0, SCALE_ONE, 0, SCALE_ONE);
    };
    // (an empty asm naming both accumulator sets: keeps the fold of the previous group behind the first MFMAs of the next one
    //  and the two sets in different registers -- see mfma_scan_kernel)
    auto pin2 = [&](Acc& x, Acc& y) { asm volatile("" : "+v"(x.t[0]), "+v"(x.t[1]), "+v"(y.t[0]), "+v"(y.t[1])); };
    const v4i* lbl = lb + lane;
    const float* lt = lthr + r;
    auto row_of = [&](uint64_t st, int t) { const uint64_t row = (st * MT + t) * 32 + r; return row <= last_row ? row : last_row; };

    // the rows of step `st`: lane (r, h) of tile t reads dword h of row st * 32 MT + 32 t + r
    const uint32_t lane_dword = r * 2 + h;
    auto load_rows = [&](uint64_t st, uint32_t (&dst)[MT][W]) {
        if (SCALAR_STEPS && (st + 1) * (32 * MT) <= p.n_s) {
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
    for (; step < nsteps; step += stride) {
        const uint64_t ns = step + stride < nsteps ? step + stride : step;
        load_rows(ns, xn);                                                          // next step's rows, in flight during this one
#pragma unroll
        for (int t = 0; t < MT; ++t)
#pragma unroll
            for (int w = 0; w < W; ++w)
                a[t][w] = v8i{(int)(nibbles(x[t][w], 0) << 1), (int)(nibbles(x[t][w], 1) << 1), (int)(nibbles(x[t][w], 2) << 1),
                              (int)(nibbles(x[t][w], 3) << 1), 0, 0, 0, 0};                      // bit ? 1.0 (0x2) : 0

        // the software pipeline of mfma_scan_kernel over the (group, word) sequence: two B buffers, two accumulator sets
        v4i bx = lbl[0], by = lbl[0];
        Acc accX, accY;
        float thrX = 0.f, thrY = lt[0];
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
            // even group g + 1 -> accY
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
        if (rcount) process_ring(step);
    }
    if (DEGREE) {                                   // the block has streamed its last step: one global atomic per counted held row
        __syncthreads();
        const JoinEmit& e = *p.e;
        for (uint32_t ql = tid; ql < groups * 32; ql += MBLOCK) {
            const uint32_t d = ldeg[ql];
            if (d != 0) atomicAdd(e.degree + e.labels_a[q0 + ql], d);      // (counted: the row exists and has a label)
        }
    }
}

}  // namespace isk
