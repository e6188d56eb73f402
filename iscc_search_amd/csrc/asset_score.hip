// Asset scoring of unit searches (asset_score.h): one block per asset query, see there.
// Built with -ffp-contract=off (Makefile): every sum, quotient and comparison rounds as CPython's float arithmetic.
#include "asset_score.h"

#include <hip/hip_runtime.h>

namespace iskas {
namespace {

constexpr uint32_t HEAD_BYTES = ((MAX_SLOTS + 2) * 4 + 15) & ~15u;   // slot bases [MAX_SLOTS + 1] | kept-group counter

__device__ inline bool less(const Item& x, const Item& y) { return x.a < y.a || (x.a == y.a && x.b < y.b); }

// bitonic sort of v[0 .. P) by (a, b), P a power of two, by the whole block (v in LDS or in this block's global scratch)
__device__ void bitonic(Item* v, uint32_t P) {
    for (uint32_t k = 2; k <= P; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t i = threadIdx.x; i < P; i += BLOCK) {
                const uint32_t l = i ^ j;
                if (l > i) {
                    const Item x = v[i], y = v[l];
                    const bool up = (i & k) == 0;
                    if (up ? less(y, x) : less(x, y)) { v[i] = y; v[l] = x; }
                }
            }
            __syncthreads();
        }
    }
}

__device__ inline uint32_t pow2_at_least(uint32_t n) { uint32_t p = 1; while (p < n) p <<= 1; return p; }

// CPython's sum() of floats: plain sequential addition (<= 3.11), or Neumaier's compensated form (>= 3.12, Objects/bltinmodule.c)
struct Sum {
    double s = 0.0, c = 0.0;
    __device__ void add(double x, bool compensated) {
        if (!compensated) { s = s + x; return; }
        const double t = s + x;
        if (fabs(s) >= fabs(x)) c += (s - t) + x;
        else c += (x - t) + s;
        s = t;
    }
    __device__ double value(bool compensated) const {
        if (compensated && c != 0.0 && isfinite(c)) return s + c;
        return s;
    }
};

// one key's group of records v[at .. n): its types in first-appearance order with the max score per type (and the table index
// that holds it), and its total.  Returns false when no type reaches the threshold.
__device__ bool score_group(const Params& p, const Item* v, uint32_t at, uint32_t n, uint32_t s0,
                            uint32_t* ty, double* sc, uint32_t* ti, uint32_t& nt, double& total) {
    const uint64_t key = v[at].a;
    nt = 0;
    for (uint32_t i = at; i < n && v[i].a == key; ++i) {
        const uint32_t slot = v[i].c >> 16, tidx = v[i].c & 0xFFFFu;
        const uint32_t t = p.slots[s0 + slot].type;
        const double s = p.score_tab[tidx];
        uint32_t j = 0;
        while (j < nt && ty[j] != t) ++j;
        if (j == nt) { ty[nt] = t; sc[nt] = s; ti[nt] = tidx; ++nt; }
        else if (s > sc[j]) { sc[j] = s; ti[j] = tidx; }
    }
    const bool comp = p.compensated != 0;
    Sum ws, ps;
    bool any = false;
    for (uint32_t j = 0; j < nt; ++j) {
        if (!(sc[j] >= p.threshold)) continue;
        any = true;
        ws.add(sc[j], comp);
        ps.add(p.pow_tab[ti[j]], comp);
    }
    if (!any) return false;
    const double w = ws.value(comp);
    total = w > 0.0 ? ps.value(comp) / w : 0.0;
    return true;
}

__global__ __launch_bounds__(BLOCK) void asset_score_kernel(const Params p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    uint32_t* const base = reinterpret_cast<uint32_t*>(lds);             // [MAX_SLOTS + 1] first item of every slot
    uint32_t* const kept = base + MAX_SLOTS + 1;
    Item* const lds_a = reinterpret_cast<Item*>(lds + HEAD_BYTES);
    Item* const lds_b = lds_a + p.lds_items;
    const uint32_t tid = threadIdx.x;
    for (uint32_t li = blockIdx.x; li < p.n_list; li += gridDim.x) {
        const uint32_t q = p.qlist ? p.qlist[li] : li;
        const uint32_t s0 = p.slot_off[q], ns = p.slot_off[q + 1] - s0;
        if (tid == 0) {
            uint32_t n = 0;
            for (uint32_t s = 0; s < ns; ++s) {
                const Slot& sl = p.slots[s0 + s];
                const uint32_t c = *sl.cnt;
                p.out_slot_count[s0 + s] = c;
                base[s] = n;
                n += c < sl.k ? c : sl.k;          // (an overflow marker counts as a full list; the host redoes that list)
            }
            base[ns] = n;
            *kept = 0;
        }
        __syncthreads();
        const uint32_t n = base[ns];
        const uint32_t P = pow2_at_least(n);
        Item* const va = P <= p.lds_items ? lds_a : p.scratch + (size_t)blockIdx.x * 2 * p.scratch_items;
        Item* const vb = P <= p.lds_items ? lds_b : va + p.scratch_items;
        // items: (key, position, slot | table index)
        for (uint32_t i = tid; i < P; i += BLOCK) {
            Item it;
            if (i < n) {
                uint32_t s = 0;
                while (base[s + 1] <= i) ++s;
                const isccsearch_record r = p.slots[s0 + s].rec[i - base[s]];
                const uint32_t pb = r.prefix_bits >> 3, h = r.hamming;
                it.a = r.key_lo;
                it.b = i;
                it.c = (s << 16) | (pb < TAB_BYTES && h < TAB_H ? pb * TAB_H + h : 0u);
            } else {
                it.a = ~0ull; it.b = 0xFFFFFFFFu; it.c = 0;
            }
            va[i] = it;
        }
        __syncthreads();
        bitonic(va, P);
        // groups: the first item of every key leads; kept groups go to vb as (~score bits, first position, leader)
        const uint64_t ex = p.exclude[q];
        const bool has_ex = p.has_exclude[q] != 0;
        for (uint32_t i = tid; i < n; i += BLOCK) {
            if (i > 0 && va[i - 1].a == va[i].a) continue;
            if (has_ex && va[i].a == ex) continue;
            uint32_t ty[MAX_TYPES], ti[MAX_TYPES];
            double sc[MAX_TYPES];
            uint32_t nt;
            double total;
            if (!score_group(p, va, i, n, s0, ty, sc, ti, nt, total)) continue;
            Item g;
            g.a = ~(uint64_t)__double_as_longlong(total);        // totals are >= 0: their bits order as the values
            g.b = va[i].b;
            g.c = i;
            vb[atomicAdd(kept, 1u)] = g;
        }
        __syncthreads();
        const uint32_t G = *kept;
        const uint32_t P2 = pow2_at_least(G);
        for (uint32_t i = G + tid; i < P2; i += BLOCK) { Item it; it.a = ~0ull; it.b = 0xFFFFFFFFu; it.c = 0; vb[i] = it; }
        __syncthreads();
        bitonic(vb, P2);
        const uint32_t out_n = G < p.limit ? G : p.limit;
        if (tid == 0) p.out_count[q] = out_n;
        for (uint32_t r = tid; r < out_n; r += BLOCK) {
            uint32_t ty[MAX_TYPES], ti[MAX_TYPES];
            double sc[MAX_TYPES];
            uint32_t nt;
            double total = 0.0;
            const uint32_t at = vb[r].c;
            score_group(p, va, at, n, s0, ty, sc, ti, nt, total);
            const size_t o = (size_t)q * p.limit + r;
            p.out_keys[o] = va[at].a;
            p.out_scores[o] = total < 1.0 ? total : 1.0;
            for (uint32_t j = 0; j < p.n_types; ++j) {
                p.out_types[o * p.n_types + j] = j < nt ? (uint8_t)ty[j] : (uint8_t)0xFF;
                p.out_type_scores[o * p.n_types + j] = j < nt ? sc[j] : 0.0;
            }
        }
        __syncthreads();        // (the next query reuses the header and the arrays)
    }
}

}  // namespace

size_t lds_bytes(uint32_t lds_items) { return HEAD_BYTES + 2 * (size_t)lds_items * sizeof(Item); }

hipError_t allow_lds(size_t bytes) {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&asset_score_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

hipError_t queue_assets(const Params& p, uint32_t grid, hipStream_t stream) {
    if (p.n_list == 0) return hipSuccess;
    hipLaunchKernelGGL(asset_score_kernel, dim3(grid), dim3(BLOCK), lds_bytes(p.lds_items), stream, p);
    return hipGetLastError();
}

}  // namespace iskas
