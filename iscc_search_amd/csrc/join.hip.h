// join.hip.h -- gfx950 device code of the index-wide joins: the self-join of one table (isccsearch_join_within) and the
// cross join of two tables (isccsearch_join_between).
//
// Every unordered pair of distinct rows of one table -- or every pair (row of table A, row of table B) -- whose Hamming distance
// over the common prefix is <= tau.  The host launches one join_scan_kernel per pair of segments (one
// segment per code length); a pair of segments (la, lb bytes) compares W = ceil(min(la, lb)/8) words, the partial last word
// masked as the scans mask it.
//
// join_scan_kernel: the XOR + popcount scan of valu_scan_kernel.hip.h with a tile of the table's own rows as its queries.
//   grid = one block per group of TQ rows of side A (wave-uniform, in SGPRs); every block streams side B once, each lane
//   holding 2*U rows per slab in VGPRs.  Within one segment (A == B) only pairs row_a < row_b count, and a block starts
//   streaming at the slab of its first row: no block is launched without a pair to look at.
//   Per (row, A row): acc = bias + popc(lo ^ a_lo) + popc(hi ^ a_hi) per word, acc < 2^31 <=> hamming <= tau; one v_min3
//   folds two rows into the lane's minimum.  A wave whose minimum passes anywhere takes the (rare) emit path: it rescores
//   its rows against the A rows re-read by scalar loads (two passes for the forms that write: count, one atomic per wave, write) and
//   drops the pairs that are not pairs (row_b <= row_a, rows past the end); the rest are its candidates.
// join_scan_kernel<W, MASK, F, CROSS> and mfma_join_kernel<W, F, CROSS> (mfma_join_kernel.hip.h) find their pairs alike whatever the
// form; only the emit path -- `emit` here, `process_ring` there -- knows what a pair leaves behind.  Its candidates are (i: row of the side
// in SGPRs / held in LDS, j: streamed row, h: distance).
//   CROSS: the two sides are segments of two tables -- every (row_a, row_b) is a candidate; else only row_b > row_a within one segment.
//   JoinForm::PAIRS (isccsearch_join_within / _between): every candidate is counted, the wave takes ONE atomic slot range and a second
//     pass writes (key_a, key_b, hamming, prefix bits) with vector stores; the self-join orders the two keys, the cross join routes the
//     key of the SGPR / held side to the output column of the table it came from (JoinEmit::sgpr_side_is_b).  Pairs past `capacity`
//     are counted and not written.
//   JoinForm::LINK (isccsearch_join_components, the self-join only): ONE pass -- per candidate the two rows' labels are loaded
//     (JoinEmit::labels_a / labels_b; UF_NONE: the row takes no part) and united in JoinEmit::parent (link_pair, uf_union of
//     unionfind.hip.h); one atomic per wave adds the labelled pairs to JoinEmit::total.  No slots, nothing written.
//   JoinForm::OVERLAP (isccsearch_join_overlaps / _segments / _overlaps_between): labels are the ranks of the rows' assets (UF_NONE: not
//     listed, or a stop chunk); only a candidate of two DIFFERENT labels takes a slot (overlap_pair, asked in both passes so that slots
//     and counts agree; overlap_slots) and writes two directed hits (label_i, label_j, row_i, hamming) and (label_j, label_i, row_j,
//     hamming) (overlap_write), which overlap.hip sorts and reduces.  CROSS: the two tables' labels live in two spaces told apart by
//     LABEL_SIDE_B, so they always differ; what a pair can share is its asset KEY, and with JoinEmit::skip_same_key such a pair takes
//     no slot.
//   JoinForm::DEGREE (isccsearch_join_degrees, the self-join only): ONE pass, nothing written -- labels as for LINK; every candidate of
//     two labelled rows adds 1 to JoinEmit::degree of either label, and one atomic per wave adds those pairs to JoinEmit::total.  The
//     interesting input is a row with 10^4 .. 10^5 partners, so no global atomic is issued per pair: here the wave sums its lanes' count
//     for an A row and lane 0 adds it once, and a lane keeps a register counter per streamed row across the A rows and adds each once;
//     mfma_join_kernel counts its held rows in LDS and flushes them when the block has streamed its last step, and a streamed row
//     gets at most one global atomic per ring walk ("The join forms": the contention rule).
//   JoinForm::LIVE (isccsearch_join_within_live, the self-join only): PAIRS over labelled rows -- a candidate takes a slot only if its
//     two rows both have a label (live_pair, asked in both passes so that slots and count agree); everything else is PAIRS'.
// A form is a template parameter, so that no form's code changes another's; join_form_exists says which are instantiated.  The emit
// branches of the two kernels are kept as they stand on purpose: the XOR + popcount kernel's hot loop is register-allocated together
// with its inlined emit path, and its machine code moves with any change to that path ("The join forms").
// Slabs are read up to the next multiple of the slab size: column capacities are multiples of ROW_ALIGN (2 048 rows), which
// every slab size divides, so those reads stay inside the allocation (rows past n are dropped in the emit path).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "unionfind.hip.h"
#include "valu_scan_kernel.hip.h"

namespace isk {

// What only the emit path reads, in device memory: as kernel arguments hipcc keeps them in SGPRs for the whole kernel,
// next to the A rows, and spills.
struct JoinEmit {
    const uint64_t* keys_a;
    const uint64_t* keys_b;
    uint64_t n_a;
    uint64_t capacity;            // pairs the outputs hold
    unsigned long long* total;    // pairs found (all launches of one call add to it)
    uint64_t* out_keys_a;         // [capacity * kw]
    uint64_t* out_keys_b;
    uint32_t* out_hamming;
    uint16_t* out_prefix_bits;
    uint32_t prefix_bits, kw;
    uint32_t sgpr_side_is_b;      // cross join: the side in SGPRs (mfma_join_kernel: the side held in LDS) is table B, its keys go to
                                  // out_keys_b (else to out_keys_a)
    // the LINK form (isccsearch_join_components): a label per row of either side (UF_NONE: none) and the union-find array over
    // the labels; `total` counts the pairs whose two rows have labels, and the outputs above are not used
    const uint32_t* labels_a;
    const uint32_t* labels_b;
    uint32_t* parent;
    // the OVERLAP form (isccsearch_join_overlaps): labels_a / labels_b as above (the ranks of the rows' assets); `total` counts the pairs
    // of two different labels, `capacity` of them have room in out_hits, two directed hits (src, dst, row, hamming) each
    uint4* out_hits;              // [2 * capacity]
    // the CROSS + OVERLAP form (isccsearch_join_overlaps_between): keys_a / keys_b are read too (128-bit keys, the asset is the first
    // word) -- when this is set, a pair of rows of equal asset key takes no slot
    uint32_t skip_same_key;
    // the DEGREE form (isccsearch_join_degrees): labels_a / labels_b as for LINK; a pair of two labelled rows adds 1 to either label's
    // entry, and `total` counts those pairs.  The LIVE form reads labels_a / labels_b and PAIRS' fields.
    uint32_t* degree;             // [labels], zeroed
};
// isccsearch_join_overlaps_between: a label of a row of table B carries this bit, a label of table A does not (ranks stay below 2^31 - 1,
// so that no label is UF_NONE)
constexpr uint32_t LABEL_SIDE_B = 0x80000000u;
struct JoinParams {
    const uint64_t* col_a[4];     // side A: rows held in SGPRs, TQ per block
    const uint64_t* col_b[4];     // side B: streamed
    const JoinEmit* e;
    uint64_t n_a, n_b;
    uint64_t mask;                // of the last compared word
    uint32_t tau, same;
};

// A rows per block (2*TQ*W SGPR operands: more spill them into VGPR lanes, read back by v_readlane in the hot loop) and
// 16-byte loads per lane and column per slab
template <int W> struct JoinCfg {
    static constexpr int TQ = W == 1 ? 16 : 8;
    static constexpr int U = TileCfg<W>::U;
    static constexpr uint32_t SLAB = BLOCK * 2 * U;
};
template <int W> constexpr uint32_t join_rows_per_block() { return JoinCfg<W>::TQ; }
template <int W> constexpr uint32_t join_slab_rows() { return JoinCfg<W>::SLAB; }

// the sum of c over the wave's lanes, in every lane
__device__ __forceinline__ uint32_t wave_sum(uint32_t c) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) c += (uint32_t)__shfl_xor((int)c, d, 64);
    return c;
}

// ---- what a join leaves behind for the pairs it finds (the file comment describes the forms)
enum class JoinForm : int { PAIRS, LINK, OVERLAP, DEGREE, LIVE };
// what exists: PAIRS and OVERLAP over one table and over two; LINK, DEGREE and LIVE over one (components, degrees and live rows are
// those of one table)
constexpr bool join_form_exists(JoinForm f, bool cross) { return f == JoinForm::PAIRS || f == JoinForm::OVERLAP || !cross; }
template <JoinForm F, bool CROSS> struct JoinFormTag {
    static constexpr JoinForm form = F;
    static constexpr bool cross = CROSS;
};
// host: f(JoinFormTag<form, cross>{}) -- the one place that maps (form, cross) to instantiations; false if that one does not exist
template <typename Fn> bool with_join_form(JoinForm form, bool cross, Fn&& f) {
    if (!join_form_exists(form, cross)) return false;
    switch (form) {
        case JoinForm::PAIRS: cross ? f(JoinFormTag<JoinForm::PAIRS, true>{}) : f(JoinFormTag<JoinForm::PAIRS, false>{}); return true;
        case JoinForm::LINK: f(JoinFormTag<JoinForm::LINK, false>{}); return true;
        case JoinForm::OVERLAP: cross ? f(JoinFormTag<JoinForm::OVERLAP, true>{}) : f(JoinFormTag<JoinForm::OVERLAP, false>{}); return true;
        case JoinForm::DEGREE: f(JoinFormTag<JoinForm::DEGREE, false>{}); return true;
        case JoinForm::LIVE: f(JoinFormTag<JoinForm::LIVE, false>{}); return true;
    }
    return false;
}

// LINK form of both emit paths, per pair (held / SGPR-side row i, streamed row j): unite the two rows' labels; 1 if both have one
__device__ __forceinline__ uint32_t link_pair(const JoinEmit& e, uint64_t i, uint64_t j) {
    const uint32_t la = e.labels_a[i], lb = e.labels_b[j];
    if (la == UF_NONE || lb == UF_NONE) return 0u;
    uf_union(e.parent, la, lb);
    return 1u;
}

// LIVE form of both emit paths, per pair (held / SGPR-side row i, streamed row j): true if both rows have a label.  Both passes of an
// emit path call this, so the slots and the count agree.
__device__ __forceinline__ bool live_pair(const JoinEmit& e, uint64_t i, uint64_t j) {
    return e.labels_a[i] != UF_NONE && e.labels_b[j] != UF_NONE;
}

// OVERLAP form of both emit paths, per pair (held / SGPR-side row i, streamed row j): the two rows' labels; true if the pair takes a
// slot -- both rows have a label (their assets are listed, neither is a stop chunk) and the labels differ.  CROSS: the labels of two
// tables always differ (LABEL_SIDE_B); with JoinEmit::skip_same_key the pair takes no slot when the two rows' asset keys are equal.
// Both passes of an emit path call this, so the slots and the count agree.
template <bool CROSS = false>
__device__ __forceinline__ bool overlap_pair(const JoinEmit& e, uint64_t i, uint64_t j, uint32_t& la, uint32_t& lb) {
    la = e.labels_a[i];
    lb = e.labels_b[j];
    if (CROSS) {
        if (la == UF_NONE || lb == UF_NONE) return false;
        return !(e.skip_same_key != 0 && e.keys_a[2 * i] == e.keys_b[2 * j]);
    }
    return la != UF_NONE && lb != UF_NONE && la != lb;
}
// ... the slots of one wave (one ring walk): lane `lane` has counted c pairs; ONE returned atomic on JoinEmit::total for all of them.
// `slot`: the first of this lane's c slots.  False when no lane of the wave has a pair.
__device__ __forceinline__ bool overlap_slots(const JoinEmit& e, uint32_t c, uint32_t lane, uint64_t& slot) {
    uint32_t incl = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = (uint32_t)__shfl_up((int)incl, d, 64);
        if (lane >= (uint32_t)d) incl += t;
    }
    const uint32_t wave_total = (uint32_t)__shfl((int)incl, 63, 64);
    if (wave_total == 0) return false;
    uint32_t lo = 0, hi = 0;
    if (lane == 0) {
        const unsigned long long b = atomicAdd(e.total, (unsigned long long)wave_total);
        lo = (uint32_t)b; hi = (uint32_t)(b >> 32);
    }
    slot = ((uint64_t)(uint32_t)__shfl((int)hi, 0, 64) << 32 | (uint32_t)__shfl((int)lo, 0, 64)) + (incl - c);
    return true;
}
// ... the two directed hits of the pair that holds `slot` (rows travel as 32 bits: the host refuses longer segments); a pair past
// the capacity was counted and is not written
__device__ __forceinline__ void overlap_write(const JoinEmit& e, uint64_t slot, uint32_t la, uint32_t lb, uint64_t i, uint64_t j, uint32_t h) {
    if (slot >= e.capacity) return;
    e.out_hits[2 * slot] = make_uint4(la, lb, (uint32_t)i, h);
    e.out_hits[2 * slot + 1] = make_uint4(lb, la, (uint32_t)j, h);
}

template <int W, bool MASK, JoinForm F, bool CROSS>
__global__ __launch_bounds__(BLOCK) void join_scan_kernel(const JoinParams p) {
    static_assert(join_form_exists(F, CROSS), "no such join form");
    constexpr bool LINK = F == JoinForm::LINK, OVERLAP = F == JoinForm::OVERLAP, DEGREE = F == JoinForm::DEGREE, LIVE = F == JoinForm::LIVE;
    constexpr int TQ = JoinCfg<W>::TQ, U = JoinCfg<W>::U;
    constexpr uint32_t SLAB = JoinCfg<W>::SLAB;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t a0 = (uint64_t)blockIdx.x * TQ;
    const uint32_t bias = sgpr(0x7FFFFFFFu - p.tau);
    const uint32_t mlo = sgpr((uint32_t)p.mask), mhi = sgpr((uint32_t)(p.mask >> 32));

    // the block's A rows as SGPR operands; rows past n_a repeat the last one (the emit path drops their pairs)
    uint32_t qlo[TQ][W], qhi[TQ][W];
#pragma unroll
    for (int q = 0; q < TQ; ++q) {
        const uint64_t row = a0 + q < p.n_a ? a0 + q : p.n_a - 1;
#pragma unroll
        for (int w = 0; w < W; ++w) {
            const uint64_t v = p.col_a[w][row];
            qlo[q][w] = sgpr((uint32_t)v);
            qhi[q][w] = sgpr((uint32_t)(v >> 32));
        }
    }

    // lane rows of slab s: s*SLAB + wave*(U*128) + u*128 + lane*2 + r (the layout of scan_kernel's tiles)
    const uint32_t lrow = wave * (uint32_t)(U * 128) + lane * 2u;
    const uint32_t s_begin = p.same ? (uint32_t)(a0 / SLAB) : 0u;
    const uint32_t s_end = (uint32_t)((p.n_b + SLAB - 1) / SLAB);

    auto load = [&](u32x4 (&v)[U][W], uint32_t s) {
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int w = 0; w < W; ++w)
                v[u][w] = *reinterpret_cast<const u32x4*>(p.col_b[w] + (uint64_t)s * SLAB + lrow + u * 128);
    };

    // exact distance of lane row (u, r) to the A row (al, ah)
    auto dist = [&](const u32x4 (&v)[U][W], int u, int r, const uint32_t (&al)[W], const uint32_t (&ah)[W]) {
        uint32_t a = 0;
#pragma unroll
        for (int w = 0; w < W; ++w) {
            uint32_t x = (r ? v[u][w].z : v[u][w].x) ^ al[w], y = (r ? v[u][w].w : v[u][w].y) ^ ah[w];
            if (MASK && w == W - 1) { x &= mlo; y &= mhi; }
            a = bcnt(y, bcnt(x, a));
        }
        return a;
    };

    // rare: some pair of this wave is within tau.  Two passes over the A rows (re-read by scalar loads, so the loop need not
    // be unrolled): count, one atomic per wave, write.
    auto emit = [&](const u32x4 (&v)[U][W], uint32_t s) {
        u32x4 r[U][W];
        launder_rows(r, v);
        const uint64_t base = (uint64_t)s * SLAB + lrow;
        auto a_row = [&](uint64_t i, uint32_t (&al)[W], uint32_t (&ah)[W]) {
#pragma unroll
            for (int w = 0; w < W; ++w) {
                const uint64_t x = p.col_a[w][i];
                al[w] = (uint32_t)x; ah[w] = (uint32_t)(x >> 32);
            }
        };
        auto is_pair = [&](uint64_t i, uint64_t j, uint32_t h) { return h <= p.tau && j < p.n_b && (CROSS || !p.same || j > i); };
        const JoinEmit& e = *p.e;
        uint32_t c = 0;
        const uint64_t a_end = a0 + TQ < p.n_a ? a0 + TQ : p.n_a;
        if (DEGREE) {                              // one pass, nothing written; no global atomic per pair (the file comment: contention)
            uint32_t lbl[U][2], cj[U][2];          // the lane's streamed rows: label, and the labelled A rows within tau across the i-loop
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int rr = 0; rr < 2; ++rr) {
                    const uint64_t j = base + u * 128 + rr;
                    lbl[u][rr] = j < p.n_b ? e.labels_b[j] : UF_NONE;
                    cj[u][rr] = 0;
                }
#pragma unroll 1
            for (uint64_t i = a0; i < a_end; ++i) {
                const uint32_t la = e.labels_a[i];  // (wave-uniform)
                if (la == UF_NONE) continue;
                uint32_t al[W], ah[W];
                a_row(i, al, ah);
                uint32_t ci = 0;
#pragma unroll
                for (int u = 0; u < U; ++u)
#pragma unroll
                    for (int rr = 0; rr < 2; ++rr) {
                        const uint32_t one = is_pair(i, base + u * 128 + rr, dist(r, u, rr, al, ah)) && lbl[u][rr] != UF_NONE ? 1u : 0u;
                        cj[u][rr] += one;
                        ci += one;
                    }
                const uint32_t of_row = wave_sum(ci);
                if (of_row != 0 && lane == 0) atomicAdd(e.degree + la, of_row);
                c += ci;
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int rr = 0; rr < 2; ++rr)
                    if (cj[u][rr] != 0) atomicAdd(e.degree + lbl[u][rr], cj[u][rr]);
            const uint32_t counted = wave_sum(c);
            if (counted != 0 && lane == 0) atomicAdd(e.total, (unsigned long long)counted);
            return;
        }
#pragma unroll 1
        for (uint64_t i = a0; i < a_end; ++i) {
            uint32_t al[W], ah[W];
            a_row(i, al, ah);
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int rr = 0; rr < 2; ++rr) {
                    const bool pair = is_pair(i, base + u * 128 + rr, dist(r, u, rr, al, ah));
                    if (LINK) c += pair ? link_pair(e, i, base + u * 128 + rr) : 0u;
                    else if (OVERLAP) { uint32_t la, lb; c += pair && overlap_pair<CROSS>(e, i, base + u * 128 + rr, la, lb) ? 1u : 0u; }
                    else if (LIVE) c += pair && live_pair(e, i, base + u * 128 + rr) ? 1u : 0u;
                    else c += pair ? 1u : 0u;
                }
        }
        if (LINK) {                                // one pass: the labelled pairs are united as they are counted, nothing is written
            const uint32_t linked = wave_sum(c);
            if (linked != 0 && lane == 0) atomicAdd(e.total, (unsigned long long)linked);
            return;
        }
        if (OVERLAP) {                             // the second pass writes the hits of the pairs the first one counted (at most TQ trips, as the first)
            uint64_t slot;
            if (!overlap_slots(e, c, lane, slot) || c == 0) return;
#pragma unroll 1
            for (uint64_t i = a0; i < a_end; ++i) {
                uint32_t al[W], ah[W];
                a_row(i, al, ah);
#pragma unroll
                for (int u = 0; u < U; ++u)
#pragma unroll
                    for (int rr = 0; rr < 2; ++rr) {
                        const uint64_t j = base + u * 128 + rr;
                        const uint32_t h = dist(r, u, rr, al, ah);
                        uint32_t la, lb;
                        if (!is_pair(i, j, h) || !overlap_pair<CROSS>(e, i, j, la, lb)) continue;
                        overlap_write(e, slot, la, lb, i, j, h);
                        ++slot;
                    }
            }
            return;
        }
        // wave-inclusive prefix of the counts; lane 63 holds the wave's total
        uint32_t incl = c;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t t = (uint32_t)__shfl_up((int)incl, d, 64);
            if (lane >= (uint32_t)d) incl += t;
        }
        const uint32_t wave_total = (uint32_t)__shfl((int)incl, 63, 64);
        if (wave_total == 0) return;               // only non-pairs passed (the diagonal, rows past the end)
        uint32_t lo = 0, hi = 0;
        if (lane == 0) {
            const unsigned long long b = atomicAdd(e.total, (unsigned long long)wave_total);
            lo = (uint32_t)b; hi = (uint32_t)(b >> 32);
        }
        uint64_t slot = ((uint64_t)(uint32_t)__shfl((int)hi, 0, 64) << 32 | (uint32_t)__shfl((int)lo, 0, 64)) + (incl - c);
        if (c == 0) return;
        const uint32_t kw = e.kw;
#pragma unroll 1
        for (uint64_t i = a0; i < a_end; ++i) {
            uint32_t al[W], ah[W];
            a_row(i, al, ah);
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int rr = 0; rr < 2; ++rr) {
                    const uint64_t j = base + u * 128 + rr;
                    const uint32_t h = dist(r, u, rr, al, ah);
                    if (!is_pair(i, j, h)) continue;
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
                        e.out_hamming[slot] = h;
                        e.out_prefix_bits[slot] = (uint16_t)e.prefix_bits;
                    }
                    ++slot;
                }
        }
    };

    auto process = [&](const u32x4 (&v)[U][W], uint32_t s) {
        uint32_t m = 0xFFFFFFFFu;
#pragma unroll
        for (int q = 0; q < TQ; ++q) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                uint32_t a0v, a1v;
#pragma unroll
                for (int w = 0; w < W; ++w) {
                    uint32_t x0 = v[u][w].x ^ qlo[q][w], y0 = v[u][w].y ^ qhi[q][w];
                    uint32_t x1 = v[u][w].z ^ qlo[q][w], y1 = v[u][w].w ^ qhi[q][w];
                    if (MASK && w == W - 1) { x0 &= mlo; y0 &= mhi; x1 &= mlo; y1 &= mhi; }
                    if (w == 0) { a0v = bcnt_s(x0, bias); a1v = bcnt_s(x1, bias); }
                    else { a0v = pin(bcnt_v(x0, a0v)); a1v = pin(bcnt_v(x1, a1v)); }
                    a0v = bcnt_v(y0, a0v);
                    a1v = bcnt_v(y1, a1v);
                    if (W > 1 && w + 1 < W) { a0v = pin(a0v); a1v = pin(a1v); }
                }
                m = min3u(m, a0v, a1v);
            }
        }
        if (__ballot((int32_t)m >= 0)) emit(v, s);
    };

    if (s_begin >= s_end) return;
    u32x4 va[U][W], vb[U][W];
    uint32_t s = s_begin;
    load(va, s);
    for (;;) {
        const uint32_t s1 = s + 1;
        if (s1 < s_end) load(vb, s1);
        process(va, s);
        if (s1 >= s_end) break;
        const uint32_t s2 = s1 + 1;
        if (s2 < s_end) load(va, s2);
        process(vb, s1);
        if (s2 >= s_end) break;
        s = s2;
    }
}

}  // namespace isk
