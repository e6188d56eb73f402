// valu_scan_kernel.hip.h -- the XOR + popcount streaming scan on the VALU: scan_kernel and scan_adapt_kernel, the pinned
// popcount chain and the inline-asm tile loads they are built from (join.hip.h streams with the same helpers).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "scan_params.hip.h"

namespace isk {

// rows per thread per tile: every thread issues U 16-byte loads per column (2 rows each)
template <int W> struct TileCfg { static constexpr int U = (W == 1) ? 4 : (W == 2 ? 2 : 1); };
template <int W> constexpr int tile_rows() { return BLOCK * 2 * TileCfg<W>::U; }
// Where the TQ queries of a group live while a block scans.
//   SGPRs (scalar operands of v_xor, nothing to load in the loop) as long as they FIT: TQ*W*2 query dwords + TQ
//   biases + the loop's own scalars must stay under ~100 registers, beyond that hipcc spills them into VGPR lanes
//   and every use costs a v_readlane -- a VALU instruction, the very resource the kernel is short of (W=4, TQ=8:
//   52 spilled SGPRs = +19 % VALU work per tile; TQ=16: 211).
//   VGPRs (wave-uniform words pinned into vector registers) were measured and bring nothing.  In ISOLATION gfx950 issues the
//   plain two-operand ops (v_xor, v_and, v_add, shifts, v_mov, v_fma_f32) of a wave64 in ~2.4 cycles when their sources are
//   VGPRs, inline constants or literals, and in ~4.1 when one source is an SGPR; v_bcnt, v_min3 and the other VOP3 integer ops
//   take ~4.1-4.4 either way (profiles/r02_micro_valu2.txt).  MIXED with those 4-cycle ops, as in this kernel's inner loop,
//   the fast forms gain nothing: 4 v_xor + 4 v_bcnt + 1 v_min3 take 35 cycles with the query words in VGPRs and 35 with them
//   in SGPRs (profiles/r02_micro_valu3.txt), and the kernel measured 78.8 k queries/s either way -- so the queries stay in
//   SGPRs, which leaves the VGPRs to the tiles in flight (7 instead of 6 waves per SIMD) and streams 2 % faster (0.84 vs
//   0.82 of HBM).
//   LDS otherwise: one broadcast ds_read_b128 per four query dwords per tile, on the LDS pipe, into VGPR operands.
template <int W, int TQ> constexpr bool queries_in_lds() { return TQ * W >= 24; }
template <int W> constexpr int query_vecs() { return (2 * W + 3) / 4; }   // u32x4 slots per query in LDS

__device__ __forceinline__ uint32_t bcnt(uint32_t x, uint32_t acc) {
    return (uint32_t)__builtin_popcount(x) + acc;   // cold paths: let the compiler pick the form
}
// Hot-path forms.  Left alone hipcc reassociates popc(x)+popc(y)+bias into 2 x v_bcnt(.., 0) +
// v_add3 and splits the row-pair minimum into v_min + v_min3 (5.75 VALU ops per (row, query) pair
// instead of 4.5).  An EMPTY asm statement on the running value stops the reassociation while
// instruction selection still folds popc(x)+acc into one v_bcnt_u32_b32 and the two mins into one
// v_min3_u32 (a non-empty asm makes the hazard recogniser pad with s_nop).
__device__ __forceinline__ uint32_t pin(uint32_t v) { asm("" : "+v"(v)); return v; }
__device__ __forceinline__ uint32_t bcnt_s(uint32_t x, uint32_t acc_sgpr) { return pin((uint32_t)__builtin_popcount(x) + acc_sgpr); }
__device__ __forceinline__ uint32_t bcnt_v(uint32_t x, uint32_t acc) { return (uint32_t)__builtin_popcount(x) + acc; }
__device__ __forceinline__ uint32_t min3u(uint32_t a, uint32_t b, uint32_t c) { return pin(min(min(a, b), c)); }
__device__ __forceinline__ uint32_t sgpr(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));   // one 16-byte global load: .x/.y = row r (lo, hi), .z/.w = row r+1

// Streaming loads of the scan kernel, issued from inline asm so that the PREFETCH stays in flight:
// hipcc's own s_waitcnt insertion drained it at the loop head (vmcnt(0) in front of the next
// prefetch's address arithmetic).  hipcc neither counts nor pads what is inside an asm statement
// (cdna_hip_programming.md section 5.7), so:
//   * every use of a destination goes through wait_tile() first (counted s_waitcnt vmcnt + "+v" ties);
//   * the string opens with `s_nop 4`: the scalar bases may come straight from v_readfirstlane /
//     v_readlane (SGPR spill reloads), and a VALU-written SGPR needs 5 wait states before a VMEM
//     instruction reads it -- without the pad the load used a stale base (wrong rows, or a fault);
//   * outputs are early-clobber: a destination must not share a register with a later load's operand;
//   * kernels using these loads must have NO scratch and NO VGPR spills (a compiler copy of a
//     destination between load and wait would read garbage): tools/kernel_resources.py checks it.
// All U*W loads of a tile are ONE statement.  saddr form: 64-bit scalar column base + one 32-bit per-lane
// byte offset + immediate u*1024 (each wave reads U KiB contiguous per column).
// Every load carries `nt`: the rows are read once per pass, and a read-only stream with this access pattern reaches
// 7.05 TB/s non-temporal against 6.25 TB/s plain (profiles/r01_micro_read.txt; the scope bits change nothing).
#define ISK_LD(dst, off, base, imm) "global_load_dwordx4 " dst ", " off ", " base " offset:" imm " nt\n\t"
template <int U, int W>
__device__ __forceinline__ void load_tile_asm(u32x4 (&v)[U][W], const void* const (&tb)[W], uint32_t voff) {
    if constexpr (W == 1) {
        static_assert(U == 4, "tile shape");
        asm volatile("s_nop 4\n\t" ISK_LD("%0", "%4", "%5", "0") ISK_LD("%1", "%4", "%5", "1024")
                     ISK_LD("%2", "%4", "%5", "2048") ISK_LD("%3", "%4", "%5", "3072")
                     : "=&v"(v[0][0]), "=&v"(v[1][0]), "=&v"(v[2][0]), "=&v"(v[3][0]) : "v"(voff), "s"(tb[0]) : "memory");
    } else if constexpr (W == 2) {
        static_assert(U == 2, "tile shape");
        asm volatile("s_nop 4\n\t" ISK_LD("%0", "%4", "%5", "0") ISK_LD("%1", "%4", "%6", "0")
                     ISK_LD("%2", "%4", "%5", "1024") ISK_LD("%3", "%4", "%6", "1024")
                     : "=&v"(v[0][0]), "=&v"(v[0][1]), "=&v"(v[1][0]), "=&v"(v[1][1]) : "v"(voff), "s"(tb[0]), "s"(tb[1]) : "memory");
    } else if constexpr (W == 3) {
        static_assert(U == 1, "tile shape");
        asm volatile("s_nop 4\n\t" ISK_LD("%0", "%3", "%4", "0") ISK_LD("%1", "%3", "%5", "0") ISK_LD("%2", "%3", "%6", "0")
                     : "=&v"(v[0][0]), "=&v"(v[0][1]), "=&v"(v[0][2]) : "v"(voff), "s"(tb[0]), "s"(tb[1]), "s"(tb[2]) : "memory");
    } else {
        static_assert(W == 4 && U == 1, "tile shape");
        asm volatile("s_nop 4\n\t" ISK_LD("%0", "%4", "%5", "0") ISK_LD("%1", "%4", "%6", "0")
                     ISK_LD("%2", "%4", "%7", "0") ISK_LD("%3", "%4", "%8", "0")
                     : "=&v"(v[0][0]), "=&v"(v[0][1]), "=&v"(v[0][2]), "=&v"(v[0][3])
                     : "v"(voff), "s"(tb[0]), "s"(tb[1]), "s"(tb[2]), "s"(tb[3]) : "memory");
    }
}
// wait until at most N vector-memory operations of this wave are outstanding, then tie the tile's
// registers to the wait so that no use can be scheduled above it
template <int N, int U, int W>
__device__ __forceinline__ void wait_tile(u32x4 (&v)[U][W]) {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
        for (int w = 0; w < W; ++w) asm volatile("" : "+v"(v[u][w]));
}

// A copy of a tile's row registers that the compiler cannot see through, for the rare emit paths: without it the compiler
// merges their rescoring with the fast path (common subexpressions) and keeps every accumulator of the tile alive.
template <int U, int W>
__device__ __forceinline__ void launder_rows(u32x4 (&r)[U][W], const u32x4 (&v)[U][W]) {
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
        for (int w = 0; w < W; ++w) { r[u][w] = v[u][w]; asm volatile("" : "+v"(r[u][w])); }
}

// ---------------------------------------------------------------------------------------------
// scan_kernel<W, MASK, TQ, MODE>
//   grid = (blocks_x, query_groups); block = 256.  Group g holds queries [g*TQ, (g+1)*TQ).
//   Fast path per tile: U*W coalesced 16-byte loads per lane, then for every query
//       acc = bias_q; acc = bcnt(row_lo ^ q_lo, acc); acc = bcnt(row_hi ^ q_hi, acc)   (per word)
//   so acc < 2^31  <=>  hamming <= tau_q, and one v_min3 folds two rows into the lane's running
//   minimum.  Only lanes whose minimum has bit 31 clear enter the (rare) emit path.
// ---------------------------------------------------------------------------------------------
//   FOLD: the fast path tests popc((lo^q_lo)|(hi^q_hi)) <= tau, a NECESSARY condition, for 3.5 instead of 4.5 ops
//         per pair; the emit path computes the exact distance.  Only pays under a tight threshold: chosen at run
//         time by scan_adapt_kernel.
template <int W, bool MASK, int TQ, int MODE, bool FOLD = false>
__device__ __forceinline__ void scan_body(const ScanParams& p) {
    static_assert(!FOLD || (W == 1 && !MASK), "the OR-fold filter is for whole 64-bit codes");
    constexpr int U = TileCfg<W>::U;
    constexpr int TILE = BLOCK * 2 * U;
    constexpr bool QL = queries_in_lds<W, TQ>() && !FOLD;
    constexpr int NV = query_vecs<W>();
    const uint32_t tid = threadIdx.x;
    const uint32_t q0 = blockIdx.y * TQ;

    // biases -> SGPRs; queries -> SGPRs (uniform addresses: scalar loads) or LDS (see queries_in_lds)
    __shared__ u32x4 lq[QL ? TQ * NV : 1];
    uint32_t qlo[QL ? 1 : TQ][W], qhi[QL ? 1 : TQ][W], bias[TQ];
#pragma unroll
    for (int q = 0; q < TQ; ++q) {
        bias[q] = sgpr(p.bias[q0 + q]);
        if constexpr (!QL) {
#pragma unroll
            for (int w = 0; w < W; ++w) {
                const uint64_t v = p.queries[(uint64_t)(q0 + q) * 4 + w];
                qlo[q][w] = sgpr((uint32_t)v);
                qhi[q][w] = sgpr((uint32_t)(v >> 32));
            }
        }
    }
    if constexpr (QL) {
        // dword d of query q = half (d & 1) of word d / 2; slots past 2*W stay zero
        uint32_t* l = reinterpret_cast<uint32_t*>(lq);
        for (uint32_t i = tid; i < (uint32_t)(TQ * NV * 4); i += BLOCK) {
            const uint32_t q = i / (NV * 4), d = i % (NV * 4);
            uint32_t val = 0;
            if (d < 2 * W) {
                const uint64_t v = p.queries[(uint64_t)(q0 + q) * 4 + d / 2];
                val = (d & 1) ? (uint32_t)(v >> 32) : (uint32_t)v;
            }
            l[i] = val;
        }
        __syncthreads();
    }
    // the words of query q as operands: SGPR copies, or one broadcast LDS read per four dwords
    auto query_words = [&](int q, uint32_t (&ql)[W], uint32_t (&qh)[W]) {
        if constexpr (QL) {
            u32x4 t[NV];
#pragma unroll
            for (int j = 0; j < NV; ++j) t[j] = lq[q * NV + j];
#pragma unroll
            for (int w = 0; w < W; ++w) { ql[w] = t[(2 * w) / 4][(2 * w) % 4]; qh[w] = t[(2 * w + 1) / 4][(2 * w + 1) % 4]; }
        } else {
#pragma unroll
            for (int w = 0; w < W; ++w) { ql[w] = qlo[q][w]; qh[w] = qhi[q][w]; }
        }
    };
    const uint32_t mlo = sgpr(p.mask_lo), mhi = sgpr(p.mask_hi);

    // Tile numbers are 32-bit ON PURPOSE: the loop tests below are then scalar compares (s_cmp_lt_u32) and scalar branches.
    // With 64-bit counters hipcc did the unsigned compares on the VALU (there is no s_cmp_lt_u64), parked the operand in a
    // register pair it also uses for load destinations, and structurised the `break`s with EXEC tests -- a control-flow
    // graph tools/audit_kernels.py cannot prove the asm-load invariants on.  The host refuses segments of >= 2^31 tiles.
    const uint32_t n_full = (uint32_t)(p.n_rows / TILE);
    // per-lane byte offset inside a tile (constant over the loop): wave w reads U KiB contiguous per column,
    // load u of a lane sits u*1024 bytes further (immediate offset); the tile base stays scalar.
    //   row(u, lane, r) = tile*TILE + wave*(U*128) + u*128 + lane*2 + r
    const uint32_t wave = tid >> 6, lane = tid & 63;
    const uint32_t voff = wave * (uint32_t)(U * 1024) + lane * 16u;
    const uint32_t row_in_tile = wave * (uint32_t)(U * 128) + lane * 2u;

    auto load_tile = [&](u32x4 (&v)[U][W], uint32_t tile) {
        const void* tb[W];
#pragma unroll
        for (int w = 0; w < W; ++w) {
            // uniform tile base, forced into an SGPR pair for the saddr operand
            const uint64_t ta = reinterpret_cast<uint64_t>(p.col[w]) + (uint64_t)tile * (uint64_t)(TILE * 8);
            tb[w] = reinterpret_cast<const void*>(((uint64_t)sgpr((uint32_t)(ta >> 32)) << 32) | sgpr((uint32_t)ta));
        }
        load_tile_asm<U, W>(v, tb, voff);
    };

    auto process = [&](const u32x4 (&v)[U][W], uint32_t tile) {
        uint32_t m = 0xFFFFFFFFu;
#pragma unroll
        for (int q = 0; q < TQ; ++q) {
            uint32_t ql[W], qh[W];
            query_words(q, ql, qh);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                uint32_t a0, a1;
                if constexpr (FOLD) {
                    // OR-fold filter for 64-bit codes: y = (lo ^ q_lo) | (hi ^ q_hi) has popc(y) <= hamming, so
                    // popc(y) <= tau is NECESSARY for a candidate.  One v_xor + one v_bitop3 (a | (b ^ c)) + one
                    // v_bcnt per row: 3.5 VALU ops per pair instead of 4.5.  For unrelated codes y is 3/4 ones
                    // (popc ~ 24 +- 2.4), so at tau ~ 12-15 the filter passes ~1e-5 of the pairs; the exact
                    // distance is computed in the emit path below.
                    const uint32_t y0 = __builtin_amdgcn_bitop3_b32(v[u][0].x ^ ql[0], v[u][0].y, qh[0], 0xF6);
                    const uint32_t y1 = __builtin_amdgcn_bitop3_b32(v[u][0].z ^ ql[0], v[u][0].w, qh[0], 0xF6);
                    a0 = (uint32_t)__builtin_popcount(y0) + bias[q];   // one v_bcnt_u32_b32 with the SGPR bias as accumulator
                    a1 = (uint32_t)__builtin_popcount(y1) + bias[q];
                    m = min3u(m, a0, a1);
                    continue;
                }
#pragma unroll
                for (int w = 0; w < W; ++w) {
                    uint32_t x0 = v[u][w].x ^ ql[w], y0 = v[u][w].y ^ qh[w];
                    uint32_t x1 = v[u][w].z ^ ql[w], y1 = v[u][w].w ^ qh[w];
                    if (MASK && w == W - 1) { x0 &= mlo; y0 &= mhi; x1 &= mlo; y1 &= mhi; }
                    if (w == 0) { a0 = bcnt_s(x0, bias[q]); a1 = bcnt_s(x1, bias[q]); }
                    else { a0 = pin(bcnt_v(x0, a0)); a1 = pin(bcnt_v(x1, a1)); }
                    a0 = bcnt_v(y0, a0);
                    a1 = bcnt_v(y1, a1);
                    // multi-word codes: every step of the chain is pinned, or hipcc re-associates the words after the
                    // first into v_bcnt(x, 0) + v_bcnt(y, 0) + v_add3 (W = 4: 48 extra VALU instructions per wave-tile)
                    if (W > 1 && w + 1 < W) { a0 = pin(a0); a1 = pin(a1); }
                }
                m = min3u(m, a0, a1);
            }
        }
        if ((int32_t)m >= 0) {
            // rare: at least one (row, query) pair of this lane is within its threshold.  Rescore per
            // query from the SGPR-resident queries (fully unrolled: no memory loads, no dynamic register
            // indexing), so a tile that takes this path costs about two plain tiles instead of the
            // ~16 a load-per-query loop cost.
            const uint64_t base = (uint64_t)tile * TILE + row_in_tile;
            u32x4 r[U][W];
            launder_rows(r, v);
#pragma unroll
            for (int q = 0; q < TQ; ++q) {
                uint32_t a[U][2];
                uint32_t mq = 0xFFFFFFFFu;
                uint32_t ql[W], qh[W];
                query_words(q, ql, qh);
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    uint32_t a0 = bias[q], a1 = bias[q];
#pragma unroll
                    for (int w = 0; w < W; ++w) {
                        uint32_t x0 = r[u][w].x ^ ql[w], y0 = r[u][w].y ^ qh[w];
                        uint32_t x1 = r[u][w].z ^ ql[w], y1 = r[u][w].w ^ qh[w];
                        if (MASK && w == W - 1) { x0 &= mlo; y0 &= mhi; x1 &= mlo; y1 &= mhi; }
                        a0 = bcnt(y0, bcnt(x0, a0));
                        a1 = bcnt(y1, bcnt(x1, a1));
                    }
                    a[u][0] = a0; a[u][1] = a1;
                    mq = min(mq, min(a0, a1));
                }
                if ((int32_t)mq >= 0) {
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const uint64_t row = base + (uint64_t)u * 128;
                        if ((int32_t)a[u][0] >= 0) emit<MODE>(p, q0 + q, a[u][0] - bias[q], row);
                        if ((int32_t)a[u][1] >= 0) emit<MODE>(p, q0 + q, a[u][1] - bias[q], row + 1);
                    }
                }
            }
        }
    };

    // software pipeline: the loads of the next tile are in flight while the current one is scored.
    // The prefetch is UNCONDITIONAL (past the end it re-reads the block's last tile) so that exactly
    // U*W younger loads are outstanding at every wait: s_waitcnt vmcnt(U*W) retires the current tile
    // and leaves the prefetch alone.  (The rare emit path may add compiler-counted stores/atomics in
    // between; more outstanding operations only make the counted wait stricter, never weaker.)
    // One tile ahead (double buffering) for every W.  A three-buffer loop that kept two tiles in flight for W = 1 was carried
    // as a compile-time switch, off; no record of its measurement survives under profiles/.
    u32x4 va[U][W], vb[U][W];
    uint32_t tile = (uint32_t)(p.row_begin / TILE) + blockIdx.x;
    if (tile < n_full) {
        const uint32_t last = n_full - 1;
        load_tile(va, tile);
        for (;;) {
            const uint32_t t1 = tile + gridDim.x;
            load_tile(vb, t1 < n_full ? t1 : last);
            wait_tile<U * W>(va);
            process(va, tile);
            if (t1 >= n_full) break;
            const uint32_t t2 = t1 + gridDim.x;
            load_tile(va, t2 < n_full ? t2 : last);
            wait_tile<U * W>(vb);
            process(vb, t1);
            if (t2 >= n_full) break;
            tile = t2;
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the last (unused) prefetch
    }

    // tail rows [n_full*TILE, n_rows): one row per thread, a slice of 256 rows per block (the host launches at least as many blocks
    // as the tail has slices).  One block used to walk the whole tail, up to 8 rounds of dependent loads: a one-query scan of 10 000
    // rows took 15 us, of 1 M rows 9 -- most of it this loop.
    {
        for (uint64_t row = (uint64_t)n_full * TILE + (uint64_t)blockIdx.x * BLOCK + tid; row < p.n_rows; row += (uint64_t)gridDim.x * BLOCK) {
            uint32_t lo[W], hi[W];
#pragma unroll
            for (int w = 0; w < W; ++w) {
                const uint64_t c = p.col[w][row];
                lo[w] = (uint32_t)c; hi[w] = (uint32_t)(c >> 32);
            }
            // (queries and biases as the tiles take them -- SGPRs or LDS, loaded in the prologue: re-read from global memory per query,
            //  a slice cost TQ rounds of dependent scalar loads)
#pragma unroll
            for (int q = 0; q < TQ; ++q) {
                uint32_t ql[W], qh[W];
                query_words(q, ql, qh);
                uint32_t a = bias[q];
#pragma unroll
                for (int w = 0; w < W; ++w) {
                    uint32_t x = lo[w] ^ ql[w], y = hi[w] ^ qh[w];
                    if (MASK && w == W - 1) { x &= mlo; y &= mhi; }
                    a = bcnt(y, bcnt(x, a));
                }
                if ((int32_t)a >= 0) emit<MODE>(p, q0 + q, a - bias[q], row);
            }
        }
    }
}

template <int W, bool MASK, int TQ, int MODE>
__global__ __launch_bounds__(BLOCK) void scan_kernel(const ScanParams p) {
    scan_body<W, MASK, TQ, MODE, false>(p);
}

// Whole 64-bit codes: both fast paths in one kernel, chosen per query group at run time.  The folded path saves one
// VALU operation per pair but raises a false alarm (a full rescoring of the tile) for ~3.8e-5 of the pairs at
// tau = 13, 8e-6 at 12, 1.5e-6 at 11 (y = (lo^q_lo)|(hi^q_hi) is Binomial(32, 3/4) for unrelated codes): it pays
// only once the group's thresholds are tight -- which the levels and the picks between stretches bring about as
// the pass advances, and which a collision lookup (max_hamming 0) has from the start.
template <int TQ, int MODE>
__global__ __launch_bounds__(BLOCK) void scan_adapt_kernel(const ScanParams p) {
    const uint32_t q0 = blockIdx.y * TQ;
    bool fold = p.fold_tau != 0;
#pragma unroll
    for (int q = 0; q < TQ; ++q) fold = fold && sgpr(p.bias[q0 + q]) >= 0x7FFFFFFFu - p.fold_tau;   // BIAS_NEVER passes too
    if (fold) scan_body<1, false, TQ, MODE, true>(p);
    else scan_body<1, false, TQ, MODE, false>(p);
}

}  // namespace isk
