// isccsearch.hip -- host side of libisccsearch_hip.so (C-ABI declared in include/isccsearch.h).
//
// Owns the device-resident column store (tables -> segments by code length -> word columns + key
// column), the host key index (lazy), and drives the search pipeline of kernels.hip.h:
//
//   per (query class, segment):   boot -> [sample scan(HIST) -> pick] -> scan(COLLECT) -> select
//   per query class:              merge of the per-segment lists (when more than one segment)
//   per overflowed query (rare):  fullhist -> exact threshold -> scan(COLLECT) into a sized
//                                 buffer -> select
//
//   range-limited (search_within / doc_freq): radius_init -> scan(COLLECT) -> select   (fixed threshold)
//
// Everything runs on one HIP stream owned by the handle; the only host synchronisation of a
// search is the final result copy (one block {records | counts | flags}); search_many shares it between
// the requests of one call.  Built for gfx950 only (hipcc --offload-arch=gfx950).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cerrno>
#include <cstdarg>
#include <cstdio>
#include <cmath>
#include <condition_variable>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>
#include <thread>
#include <atomic>
#include <functional>
#include <chrono>
#include <vector>

#include "../../include/isccsearch.h"
#include "kernels.hip.h"
#include "join.hip.h"
#include "mfma_scan.h"
#include "docfreq.h"
#include "simprint_score.h"
#include "asset_score.h"
#include "keymap.h"

namespace {

thread_local std::string g_last_error;

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

// A failed HIP call also leaves its code in the runtime's "last error" slot, where the next
// hipGetLastError() -- the launch check of an unrelated, later call -- would find it: clear it when reporting.
#define HIPOK(expr)                                                                              \
    do {                                                                                         \
        hipError_t e_ = (expr);                                                                  \
        if (e_ != hipSuccess) {                                                                  \
            (void)hipGetLastError();                                                             \
            return fail(e_ == hipErrorOutOfMemory ? -ENOMEM : -EIO, "%s failed: %s (%s:%d)", #expr, \
                        hipGetErrorString(e_), __FILE__, __LINE__);                              \
        }                                                                                        \
    } while (0)

using iskhost::Key;
using iskhost::KeyHash;
using iskhost::KeyMap;
using iskhost::Loc;

// the backoff of a speculation hint: the hint serves batches of ONE k, and a miss makes the next `penalty` batches of its class take
// the ordinary path (1, 3, 7, 15 for misses in a row)
struct HintBackoff {
    uint32_t k = 0, skip = 0, penalty = 0;
    bool ready(uint32_t want_k) {                       // speculate now?
        if (k != want_k) return false;
        if (skip) { skip -= 1; return false; }
        return true;
    }
    void miss() { penalty = std::min<uint32_t>(2 * penalty + 1, 15); skip = penalty - 1; }      // (the rerun that follows is the first skipped batch)
};

struct Segment {
    uint32_t nbytes = 0, W = 0;
    uint64_t n = 0, cap = 0;
    uint64_t* col[4] = {nullptr, nullptr, nullptr, nullptr};
    uint64_t* keys = nullptr;
    std::vector<uint64_t> hkeys;   // host mirror of the key column, kept only while the table is indexed
    // document-frequency column (docfreq.hip): built lazily, dropped by every change of the rows
    uint32_t* freq = nullptr;
    uint64_t freq_rows = 0;        // rows the column was built for (0 = not built)
    uint32_t freq_dup = 0;         // dup_limit it was built with
    void touch() { freq_rows = 0; }
    // small batches (the reference's per-unit call shape): the k-th distance the last search of this segment ended at -- the next
    // one tries ONE collect pass under it (+ margin) before the bootstrap / level / pick chain (search_locked).  One hint per
    // batch-size class (the worst k-th distance of 100 queries lies a bit or two above that of one); a hint decays by one bit per
    // hit towards what the batches need (a near-duplicate query between two ordinary ones does not pull it down to its own
    // distance); a miss backs off (HintBackoff).
    struct SpecHint : HintBackoff {
        uint32_t tau = 0;
        // margin above the worst k-th distance the last batch ended at.  The k-th distance of a query concentrates as k grows (it is an
        // order statistic k deep into the distribution), and so does its maximum over a batch: from k = 64 one bit is enough -- and a bit
        // is worth a factor ~2.6 in candidates at these distances (10 M x 64-bit, 512 queries, k = 400: 3 480 candidates per query
        // under + 2, profiles/r04_candidate_path.txt).  Small k keeps two: its k-th distance wanders more and a bit costs little there.
        static uint32_t margin(uint32_t want_k) { return want_k >= 64 ? 1u : 2u; }
        void hit(uint32_t worst) { penalty = 0; tau = std::min<uint32_t>(std::max<uint32_t>(worst + margin(k), tau ? tau - 1 : 0), 8 * ISCCSEARCH_MAX_BYTES); }
        void seed(uint32_t new_k, uint32_t worst) { k = new_k; tau = std::min<uint32_t>(worst + margin(new_k), 8 * ISCCSEARCH_MAX_BYTES); }
    } spec[12][5];
    // one hint per batch-size class (1 | 2-3 | 4-7 | ... | 1024) and per compared PREFIX length (8 / 16 / 24 / 32 bytes and the odd ones:
    // an NPHD table of 256-bit rows answers 64-bit queries over a 64-bit prefix, whose k-th distance has nothing to do with a 256-bit one's)
    SpecHint& hint(uint32_t nq, uint32_t len) { return spec[nq ? 32 - __builtin_clz(nq) : 0][len % 8 == 0 && len >= 8 && len <= 32 ? len / 8 : 0]; }
};

struct Table {
    bool open = false;
    int metric = 0, key_words = 1, max_bytes = 0, max_words = 0;
    Segment seg[ISCCSEARCH_MAX_BYTES + 1];
    // Tables of SEVERAL code lengths (an ISCC-UNIT index): the hint is the worst k-th NPHD (distance / compared bits) the previous
    // batch of that size and query length ended at; every segment then lists its rows within (ratio + 1/32) x its compared bits.
    struct RatioHint : HintBackoff {
        double ratio = 0.0;
        void hit(double worst) { penalty = 0; ratio = std::max(worst, ratio - 1.0 / 256.0); }
        void seed(uint32_t new_k, double worst) { k = new_k; ratio = worst; }
    } mspec[12][5];
    RatioHint& mhint(uint32_t nq, uint32_t len) { return mspec[nq ? 32 - __builtin_clz(nq) : 0][len % 8 == 0 && len >= 8 && len <= 32 ? len / 8 : 0]; }
    bool indexed = false;
    KeyMap index;
    uint64_t total = 0;     // rows over all segments
    uint32_t segments() const {     // non-empty segments: the jobs of a batch
        uint32_t n = 0;
        for (uint32_t b = 1; b <= ISCCSEARCH_MAX_BYTES; ++b) n += seg[b].n ? 1 : 0;
        return n;
    }
    Segment* sole_segment() {       // the only non-empty segment, or nullptr
        Segment* one = nullptr;
        for (uint32_t b = 1; b <= ISCCSEARCH_MAX_BYTES; ++b)
            if (seg[b].n) { if (one) return nullptr; one = &seg[b]; }
        return one;
    }
};

constexpr uint32_t QB_MAX = 1024;        // queries per pipeline run
constexpr uint64_t CACHE_STRETCH_BYTES = 128ull << 20;   // half of the 256 MiB Infinity Cache
constexpr uint64_t ROW_ALIGN = 2048;     // column capacities are multiples of the largest tile

template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    int ensure(size_t need) {
        if (need <= n) return 0;
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
        size_t want = need + need / 4;
        hipError_t e = hipMalloc((void**)&p, want * sizeof(T));
        if (e != hipSuccess) { p = nullptr; (void)hipGetLastError(); return fail(-ENOMEM, "hipMalloc(%zu bytes) failed: %s", want * sizeof(T), hipGetErrorString(e)); }
        n = want;
        return 0;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; n = 0; }
};

template <typename T>
struct PinBuf {   // page-locked host memory: async copies really are asynchronous
    T* p = nullptr;
    size_t n = 0;
    int ensure(size_t need) {
        if (need <= n) return 0;
        if (p) (void)hipHostFree(p);
        p = nullptr;
        n = 0;
        size_t want = need + need / 4 + 16;
        hipError_t e = hipHostMalloc((void**)&p, want * sizeof(T), hipHostMallocDefault);
        if (e != hipSuccess) { p = nullptr; (void)hipGetLastError(); return fail(-ENOMEM, "hipHostMalloc(%zu bytes) failed: %s", want * sizeof(T), hipGetErrorString(e)); }
        n = want;
        return 0;
    }
    void release() { if (p) (void)hipHostFree(p); p = nullptr; n = 0; }
};

constexpr size_t DIRECT_RESULT_BYTES = 1 << 20;   // result blocks up to this size are written by the kernels straight into pinned host memory

uint64_t mask_for(uint32_t pbytes) {   // mask of the last compared word for a prefix of pbytes bytes
    const uint32_t rem = pbytes & 7;
    return rem ? ~0ULL << (8 * (8 - rem)) : ~0ULL;
}
uint32_t next_pow2(uint32_t v) { uint32_t p = 2; while (p < v) p <<= 1; return p; }

}  // namespace

struct PendingSearch;
struct isccsearch_handle {
    std::mutex mu;
    // combining queue of isccsearch_search callers
    std::mutex qmu;
    std::condition_variable qcv;
    std::vector<PendingSearch*> pending;
    bool leader_active = false;
    int device = 0;
    int cus = 256;
    hipStream_t stream = nullptr;
    std::vector<std::unique_ptr<Table>> tables;
    // options
    int tq = 8;   // queries per streaming pass: 8 keeps the scan HBM-bound
    bool profile = false;
    bool count_candidates = false;   // read the candidate counters back after every batch (one more copy + synchronisation: accounting runs only)
    bool nontemporal = true;
    uint32_t blocks_per_cu = 8;    // scan grid = CUs x this (per query group)
    uint64_t boot_rows = 65536;    // rows of the threshold bootstrap of the level design (4 096 exact + the rest counted under that
                                   // cut; wide blocks for small batches): one level launch + pick less than with 4 096 rows
                                   // (100 M x 64-bit: 8 queries 0.231 against 0.252 ms, 4 queries at k = 100 0.286 against 0.354)
    uint64_t level_growth = 8;     // each threshold level streams this many times the rows seen so far
    bool repick = true;            // re-derive the threshold after every collect stretch but the last
    uint32_t tiny_rows = 16384;       // segments of at most this many rows are answered by ONE launch (tiny_search_kernel); 0: never
    uint32_t select_wide_from = 2048; // sort buffers of at least this many slots are selected by 1 024-thread blocks (option; 0xFFFFFFFF: never)
    uint32_t fold_tau = 11;        // 64-bit codes: groups whose thresholds are all <= this take the folded fast path (0: off)
    uint64_t stretch_bytes = CACHE_STRETCH_BYTES;   // rows per collect launch when several query groups share them (0: one pass)
    uint64_t mfma_stretch_factor = 3;               // ... times this on the matrix cores, when several CHUNKS of queries share them
    // large batches: the scan as an FP4 matrix-core contraction (mfma_scan.hip) instead of XOR + popcount on the VALU
    bool mfma = true;
    uint32_t mfma_pack_min_queries = 9;   // 64-bit codes (packed matrix-core kernel): from this many queries (see use_mfma)
    uint64_t mfma_few_rows = 12ull << 20;   // longer codes: segments up to this many rows take the matrix cores from mfma_pack_min_queries queries too
    uint32_t mfma_min_queries = 17;   // batches below this stay on the XOR + popcount kernel, HBM-bound up to ~11 queries per pass
                                      // (100 M x 64-bit: 32 queries 0.49 ms against 0.71 ms, 24 queries 0.48 against 0.63; at 16 both take 0.47 ms)
    uint32_t self_boot_per_k = 1024;  // the single pass's bootstrap sample is at least this many rows per wanted neighbour (and self_boot_rows)
    bool spec_suppress = false;       // (isccsearch_search_many: the ordinary rerun of a request whose speculative pass just missed)
    int device_search_hint = -1;      // one-shot: the next isccsearch_search_device_async starts its single pass under this threshold (the caller verifies)
    int self_hint = 1;                // batches above spec_max_queries: start the single self-tightening pass under the hint (no bootstrap sample)
    int speculate = 1;                // small batches: try one range-limited pass under the previous search's k-th distance first
    uint32_t spec_max_queries = 128;   // ... batches of up to this many queries
    int mfma_pack = 1;                // 64-bit codes on the matrix cores: two row tiles per accumulator, packed f16 fold (mfma_pack_kernel)
    int mfma_pack3 = 1;               // ... chunks of more than four query groups: three row tiles per accumulator, OR fold (mfma_pack3_kernel); 0: mfma_pack_kernel
    uint64_t mfma_min_rows = 65536;   // launches over fewer rows do not amortise the per-block query expansion
    // k <= self_max_k on the matrix cores: ONE pass whose thresholds tighten themselves (MODE_SELF) instead of levels + picks --
    // every launch of that chain costs ~35 us of ramp, prologue and tail, and a step of 100 M rows had seven of them
    bool self_tighten = true;
    bool boot_multi = true;           // large batches: boot_multi_kernel (four queries per block share the sample's row loads)
    uint32_t candidate_cap = 16384;   // floor of the per-query candidate buffer (entries); tests shrink it to reach the overflow paths
    uint32_t self_refresh_steps = 1;  // steps of a full chunk between two looks at the live thresholds (power of two)
    uint32_t self_max_k = ISCCSEARCH_MAX_K;   // (512 until the single pass was measured beyond it: k = 1 000 / 2 000 over 100 M rows 6.0 / 9.0 ms against
                                      //  8.5 / 14.0 of the level design, 4.2 / 6.6 under a hint -- tools/ab_self_max_k.sh; the unpruned lists hold
                                      //  ~k ln(n / sample) entries + the first steps' flood: see the cap in Batch::begin)
                                      // (100 M rows, k = 100 / 256 / 512: 3.80 / 4.52 / 6.04 ms against 4.60 / 5.35 / 7.37 with levels)
    uint64_t self_boot_rows = 65536;  // its bootstrap sample: all waves start under the sample's threshold at once, so a
                                      // short sample floods the first steps with candidates (4 096 rows: ~860 per query)
    uint64_t mfma_level_growth = 4;   // threshold levels when the scan runs on the matrix cores (k <= 64): 4 / 6 / 8 measured 295.5 / 295.9 / 290.4 k q/s at 100 M rows and 1.35 / 1.28 / 1.27 M at 12.5 M
    // NPHD distance ranks: rank[p_bytes][h] (u16), row 0 = identity (Hamming tables)
    uint16_t* d_rank = nullptr;
    // scratch
    DevBuf<uint64_t> d_queries;     // [nq_pad][4]
    DevBuf<uint32_t> d_bias, d_cnt, d_ghist, d_overflow, d_listcnt, d_outcnt, d_freq;
    DevBuf<float> d_thr;            // [nq_pad] live thresholds of the self-tightening pass
    DevBuf<uint64_t> d_cand;
    DevBuf<isk::Record> d_lists, d_final;
    PinBuf<uint64_t> p_queries;     // pinned staging: queries in, flags / results out
    PinBuf<uint32_t> p_flags;
    // one batch's results as ONE block {records [m][k] | counts [m] | overflow flags}: a single device->host copy
    DevBuf<unsigned char> d_block;
    PinBuf<unsigned char> p_block;
    DevBuf<uint64_t> d_misc;        // moves / gather rows / single query
    DevBuf<uint64_t> d_misc2;
    std::vector<isk::Record> h_final;
    std::vector<uint32_t> h_cnt, h_overflow;
    // isccsearch_simprint_score: the neighbour lists of one request stay on the device with their rows; simprint_score.hip's buffers
    DevBuf<isk::Record> d_sp_rec;
    DevBuf<uint32_t> d_sp_rows, d_sp_nbest, d_sp_offs, d_sp_freqq, d_sp_unknown, d_sp_entry[2], d_sp_order[2], d_sp_matches, d_sp_nassets;
    DevBuf<uint32_t> d_sp_cnt, d_sp_dofg;       // isccsearch_simprint_exact: list lengths of every lookup, the lookup of every given simprint
    DevBuf<unsigned char> d_sp_best, d_sp_temp;
    DevBuf<uint64_t> d_sp_asset[2];
    DevBuf<double> d_sp_score[2], d_sp_tab, d_sp_ws, d_sp_idfq;
    // isccsearch_simprint_score_many: request keys / sort payloads per entry, per-request offsets and counts, chunks per result
    DevBuf<uint32_t> d_spm_req[2], d_spm_idx[2], d_spm_qbeg, d_spm_nassets, d_spm_astart, d_spm_estart, d_spm_cnt, d_spm_cpos;
    std::vector<uint32_t> h_sp_qbeg, h_sp_qcount;     // (host side of a round: kept, so that a scoring call allocates nothing here)
    PinBuf<double> p_sp_tab;
    PinBuf<unsigned char> p_sp_out;
    // the similarity / IDF tables on the device are those of (bits, total_assets, dup_limit):
    uint32_t sp_tab_bits = 0, sp_tab_dup = 0xFFFFFFFFu;
    int64_t sp_tab_total = -1;
    // isccsearch_match_assets: every unit list of a call stays on the device for asset_score.hip
    DevBuf<isk::Record> d_am_rec, d_am_rec2;      // first lists / second INSTANCE pass
    DevBuf<uint32_t> d_am_cnt, d_am_cnt2, d_am_off;   // counts (+ overflow flags) / second pass counts / slot offsets + query list
    DevBuf<iskas::Slot> d_am_slots;
    DevBuf<uint64_t> d_am_ex;
    DevBuf<uint8_t> d_am_hasex;
    DevBuf<double> d_am_tab;                     // score table | pow table
    std::vector<double> am_tab;                  // ... as last uploaded
    DevBuf<iskas::Item> d_am_scratch;
    PinBuf<unsigned char> p_am_out;
    // isccsearch_join_within: the pairs of one call {keys_a | keys_b}, distances, prefix bits, and their count
    DevBuf<uint64_t> d_join_keys, d_join_total;
    DevBuf<uint32_t> d_join_ham;
    DevBuf<uint16_t> d_join_pb;
    DevBuf<isk::JoinEmit> d_join_emit;             // one descriptor per launch
    size_t am_lds_allowed = 0;                   // dynamic LDS the scoring kernel was allowed on this handle's device
    // profiling
    // asynchronous device searches: "results ready" for the consumer stream, "query upload done" for the pinned staging
    hipEvent_t ev_done = nullptr, ev_staged = nullptr, ev_producer = nullptr;
    bool ev_staged_pending = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pool;
    std::vector<char> ev_level;      // per used pair: 1 = a threshold-level launch, 0 = a collect launch
    size_t ev_used = 0;
    isccsearch_stats stats{};
};

namespace {

using H = isccsearch_handle;

void build_rank_table(std::vector<uint16_t>& rank) {
    // rank[p][h] for p in 1..32 bytes: position of h/(8p) among all distinct fractions; row 0: identity
    struct Fr { uint32_t h, p; };
    std::vector<Fr> all;
    for (uint32_t p = 1; p <= 32; ++p)
        for (uint32_t h = 0; h <= 8 * p; ++h) all.push_back({h, p});
    auto less = [](const Fr& a, const Fr& b) { return (uint64_t)a.h * b.p < (uint64_t)b.h * a.p; };
    std::sort(all.begin(), all.end(), less);
    rank.assign(33 * 257, 0xFFFF);
    uint32_t r = 0;
    for (size_t i = 0; i < all.size(); ++i) {
        if (i && less(all[i - 1], all[i])) ++r;
        rank[all[i].p * 257 + all[i].h] = (uint16_t)r;
    }
    for (uint32_t h = 0; h <= 256; ++h) rank[h] = (uint16_t)h;
}

int seg_reserve(H* h, Table& t, Segment& s, uint64_t need) {
    if (need <= s.cap) return 0;
    uint64_t cap = std::max<uint64_t>(need, s.cap * 2);
    cap = (cap + ROW_ALIGN - 1) / ROW_ALIGN * ROW_ALIGN;
    uint64_t* ncol[4] = {nullptr, nullptr, nullptr, nullptr};
    uint64_t* nkeys = nullptr;
    auto cleanup = [&]() { for (auto& c : ncol) if (c) (void)hipFree(c); if (nkeys) (void)hipFree(nkeys); };
    for (uint32_t w = 0; w < s.W; ++w) {
        hipError_t e = hipMalloc((void**)&ncol[w], cap * 8);
        if (e != hipSuccess) { cleanup(); (void)hipGetLastError(); return fail(-ENOMEM, "hipMalloc(column, %llu bytes) failed: %s", (unsigned long long)cap * 8, hipGetErrorString(e)); }
    }
    {
        hipError_t e = hipMalloc((void**)&nkeys, cap * 8 * t.key_words);
        if (e != hipSuccess) { cleanup(); (void)hipGetLastError(); return fail(-ENOMEM, "hipMalloc(keys) failed: %s", hipGetErrorString(e)); }
    }
    if (s.n) {
        // a failure here must not leak the new columns (the old ones stay in place and valid)
        hipError_t e = hipSuccess;
        for (uint32_t w = 0; w < s.W && e == hipSuccess; ++w) e = hipMemcpyAsync(ncol[w], s.col[w], s.n * 8, hipMemcpyDeviceToDevice, h->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(nkeys, s.keys, s.n * 8 * t.key_words, hipMemcpyDeviceToDevice, h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) {
            (void)hipStreamSynchronize(h->stream);
            cleanup();
            (void)hipGetLastError();
            return fail(-EIO, "growing a segment to %llu rows failed while copying: %s", (unsigned long long)cap, hipGetErrorString(e));
        }
    }
    for (uint32_t w = 0; w < s.W; ++w) { if (s.col[w]) (void)hipFree(s.col[w]); s.col[w] = ncol[w]; }
    if (s.keys) (void)hipFree(s.keys);
    s.keys = nkeys;
    s.cap = cap;
    return 0;
}

void seg_free(Segment& s) {
    for (auto& c : s.col) { if (c) (void)hipFree(c); c = nullptr; }
    if (s.keys) (void)hipFree(s.keys);
    s.keys = nullptr;
    if (s.freq) (void)hipFree(s.freq);
    s.freq = nullptr;
    s.freq_rows = 0;
    s.n = s.cap = 0;
    s.hkeys.clear();
    s.hkeys.shrink_to_fit();
}

int get_table(H* h, uint32_t id, Table*& out) {
    if (id >= h->tables.size() || !h->tables[id] || !h->tables[id]->open) return fail(-ENOENT, "table %u is not open", id);
    out = h->tables[id].get();
    return 0;
}

int ensure_index(H* h, Table& t) {
    if (t.indexed) return 0;
    t.index.reset(t.key_words == 2);
    t.index.reserve((size_t)t.total + 16);
    for (uint32_t b = 1; b <= ISCCSEARCH_MAX_BYTES; ++b) {
        Segment& s = t.seg[b];
        if (!s.n) { s.hkeys.clear(); continue; }
        s.hkeys.resize((size_t)s.n * t.key_words);
        HIPOK(hipMemcpyAsync(s.hkeys.data(), s.keys, s.n * 8 * t.key_words, hipMemcpyDeviceToHost, h->stream));
        HIPOK(hipStreamSynchronize(h->stream));
        for (uint64_t r = 0; r < s.n; ++r) {
            Key k = t.key_words == 2 ? Key{s.hkeys[2 * r], s.hkeys[2 * r + 1]} : Key{0, s.hkeys[r]};
            t.index.set(k, Loc{b, r});
        }
    }
    t.indexed = true;
    return 0;
}

// the segment's document-frequency column (docfreq.hip), (re)built when rows changed since it was made
int ensure_freq_column(H* h, Table& t, Segment& s, uint32_t dup_limit) {
    if (s.freq_rows == s.n && s.freq_dup == dup_limit && s.freq) return 0;
    if (s.freq) { (void)hipFree(s.freq); s.freq = nullptr; }
    s.freq_rows = 0;
    hipError_t e = hipMalloc((void**)&s.freq, s.n * sizeof(uint32_t));
    if (e != hipSuccess) { s.freq = nullptr; (void)hipGetLastError(); return fail(-ENOMEM, "hipMalloc(frequency column, %llu bytes) failed: %s", (unsigned long long)s.n * 4, hipGetErrorString(e)); }
    std::string err;
    int rc;
    if ((rc = iskdf::build_freq_column(s.col, (int)s.W, s.keys, t.key_words, s.n, dup_limit, s.freq, h->stream, &err))) return fail(rc, "%s", err.c_str());
    s.freq_rows = s.n;
    s.freq_dup = dup_limit;
    h->stats.freq_builds += 1;
    return 0;
}

// ------------------------------------------------------------------------------------------
// kernel dispatch
// ------------------------------------------------------------------------------------------
template <int W, bool MASK, int TQ, int MODE>
void launch_scan_nt(bool nt, dim3 grid, hipStream_t st, const isk::ScanParams& p) {
    // only the non-temporal variant is instantiated: plain loads measured no faster and
    // every extra variant costs build time
    (void)nt;
    hipLaunchKernelGGL((isk::scan_kernel<W, MASK, TQ, MODE, true>), grid, dim3(isk::BLOCK), 0, st, p);
}
template <int W, bool MASK, int TQ>
void launch_scan_mode(int mode, bool nt, dim3 grid, hipStream_t st, const isk::ScanParams& p) {
    if (mode == isk::MODE_COLLECT) launch_scan_nt<W, MASK, TQ, isk::MODE_COLLECT>(nt, grid, st, p);
    else if (mode == isk::MODE_STRETCH) launch_scan_nt<W, MASK, TQ, isk::MODE_STRETCH>(nt, grid, st, p);
    else launch_scan_nt<W, MASK, TQ, isk::MODE_BOTH>(nt, grid, st, p);
}
template <int W, bool MASK>
void launch_scan_tq(int tq, int mode, bool nt, dim3 grid, hipStream_t st, const isk::ScanParams& p) {
    switch (tq) {
        case 8: launch_scan_mode<W, MASK, 8>(mode, nt, grid, st, p); break;
        default: launch_scan_mode<W, MASK, 16>(mode, nt, grid, st, p); break;
    }
}
template <int W>
void launch_scan_mask(bool mask, int tq, int mode, bool nt, dim3 grid, hipStream_t st, const isk::ScanParams& p) {
    if (mask) launch_scan_tq<W, true>(tq, mode, nt, grid, st, p);
    else launch_scan_tq<W, false>(tq, mode, nt, grid, st, p);
}
template <int MODE>
void launch_scan_adapt(int tq, dim3 grid, hipStream_t st, const isk::ScanParams& p) {
    switch (tq) {
        case 8: hipLaunchKernelGGL((isk::scan_adapt_kernel<8, MODE>), grid, dim3(isk::BLOCK), 0, st, p); break;
        default: hipLaunchKernelGGL((isk::scan_adapt_kernel<16, MODE>), grid, dim3(isk::BLOCK), 0, st, p); break;
    }
}
void launch_scan(int W, bool mask, int tq, int mode, bool nt, dim3 grid, hipStream_t st, const isk::ScanParams& p) {
    if (W == 1 && !mask && p.fold_tau) {   // whole 64-bit codes: the kernel picks its fast path per query group
        if (mode == isk::MODE_COLLECT) launch_scan_adapt<isk::MODE_COLLECT>(tq, grid, st, p);
        else if (mode == isk::MODE_STRETCH) launch_scan_adapt<isk::MODE_STRETCH>(tq, grid, st, p);
        else launch_scan_adapt<isk::MODE_BOTH>(tq, grid, st, p);
        return;
    }
    switch (W) {
        case 1: launch_scan_mask<1>(mask, tq, mode, nt, grid, st, p); break;
        case 2: launch_scan_mask<2>(mask, tq, mode, nt, grid, st, p); break;
        case 3: launch_scan_mask<3>(mask, tq, mode, nt, grid, st, p); break;
        default: launch_scan_mask<4>(mask, tq, mode, nt, grid, st, p); break;
    }
}
int tile_rows_for(int W) { return W == 1 ? isk::tile_rows<1>() : W == 2 ? isk::tile_rows<2>() : W == 3 ? isk::tile_rows<3>() : isk::tile_rows<4>(); }

// blocks per query group.
//   Tables beyond the Infinity Cache (and their scans of every row): every group gets the whole
//   chip, so groups run one after the other and each streams the table from HBM exactly once.
//   Sample scans and cache-resident tables cover few tiles per group: spread the chip's resident
//   blocks over ALL groups instead, so that each block walks several tiles (the per-block prologue
//   -- queries -> SGPRs -- and the load pipeline are amortised) and concurrent groups share the
//   cached rows.
constexpr uint64_t CACHE_RESIDENT_BYTES = 128ull << 20;   // half of the 256 MiB Infinity Cache
uint32_t scan_grid_x(H* h, int W, uint64_t rows, uint32_t groups = 1, bool sample = false) {
    const uint64_t tiles = rows / (uint64_t)tile_rows_for(W);
    uint64_t maxb = (uint64_t)h->cus * h->blocks_per_cu;
    if (sample || rows * 8 * (uint64_t)W <= CACHE_RESIDENT_BYTES)
        maxb = std::max<uint64_t>(8, maxb / std::max<uint32_t>(1, groups));
    // (the rows behind the last whole tile are scanned one slice of BLOCK rows per block: at least that many blocks)
    const uint64_t tail_slices = (rows % (uint64_t)tile_rows_for(W) + isk::BLOCK - 1) / isk::BLOCK;
    return (uint32_t)std::max<uint64_t>(std::max<uint64_t>(1, tail_slices), std::min<uint64_t>(tiles, maxb));
}

int drain_events(H* h);
int event_pair(H* h, hipEvent_t& a, hipEvent_t& b, bool level = false) {
    // a caller that profiles for a long time without reading the statistics must not grow the pool without bound
    if (h->ev_used >= 4096) { int rc = drain_events(h); if (rc) return rc; }
    if (h->ev_used == h->ev_pool.size()) {
        hipEvent_t x, y;
        HIPOK(hipEventCreate(&x));
        HIPOK(hipEventCreate(&y));
        h->ev_pool.emplace_back(x, y);
    }
    a = h->ev_pool[h->ev_used].first;
    b = h->ev_pool[h->ev_used].second;
    if (h->ev_level.size() <= h->ev_used) h->ev_level.resize(h->ev_used + 1);
    h->ev_level[h->ev_used] = level ? 1 : 0;
    ++h->ev_used;
    return 0;
}

// fold the recorded event pairs into stats.scan_ms (synchronises the stream)
int drain_events(H* h) {
    if (!h->ev_used) return 0;
    HIPOK(hipStreamSynchronize(h->stream));
    for (size_t i = 0; i < h->ev_used; ++i) {
        float ms = 0.f;
        HIPOK(hipEventElapsedTime(&ms, h->ev_pool[i].first, h->ev_pool[i].second));
        if (h->ev_level[i]) h->stats.level_ms += ms; else h->stats.scan_ms += ms;
    }
    h->ev_used = 0;
    return 0;
}

// ------------------------------------------------------------------------------------------
// the search pipeline for one batch (<= QB_MAX) of equal-length queries
//   begin()  every (segment) job back to back on the stream, no host synchronisation
//   flags    one small device->host copy tells which queries overflowed their candidate list
//   fix()    exact fallback for those (rare)
//   merge()  k-way merge of the per-segment lists when the table has more than one segment
// ------------------------------------------------------------------------------------------
struct Job {
    Segment* seg;
    uint32_t pbytes;   // compared prefix in bytes
    uint32_t W;        // words compared
    bool mask;
    uint64_t mask_last;
    bool pack;         // matrix-core launches run mfma_pack_kernel (one word, no all-zero query in the batch)
};

struct Batch {
    H* h;
    Table& t;
    uint32_t nq, qbytes, k;
    isk::Record* d_out;       // [nq*k]   device
    uint32_t* d_out_cnt;      // [nq]     device
    uint32_t* d_out_rows = nullptr;   // [nq*k] when set, select_kernel also leaves the segment row of every record (simprint scoring)
    uint32_t* d_out_kth = nullptr;    // [nq]   when set, ... and the hamming distance of every query's last result
    int tq = 8;
    int radius = -1;          // >= 0: report only rows within this Hamming distance (fixed threshold, no sampling)
    double radius_ratio = -1.0;   // >= 0 (speculative pass over SEVERAL segments): per segment, rows within ratio x compared bits
    bool ratio_starts_self = false;   // ... as the START of each segment's single self-tightening pass (large batches) instead of a fixed radius
    size_t pq_off = 0;                  // this batch's slice of the pinned query staging buffer (words)
    uint32_t* d_flags = nullptr;        // overflow flags [jobs][nq_pad]; the caller may place them inside its result block
    const uint32_t* h_flags = nullptr;  // ... and where the host finds them after ITS copy (nullptr: copy_flags() brings them to h->p_flags)
    uint32_t nq_pad = 0, groups = 0, cap = 0, P = 0;
    size_t sel_lds = 0;
    bool multi = false;
    bool mark_overflow = false;         // search_device_async: overflowed queries report COUNT_OVERFLOW instead of being fixed here
    bool allow_self = true, used_self = false;   // the single self-tightening pass, and whether a job of this batch took it
    int self_hint = -1;       // >= 0: the single pass starts under THIS threshold instead of a bootstrap sample's (search_locked verifies)
    bool used_hint = false;
    std::vector<Job> jobs;

    Batch(H* h_, Table& t_, uint32_t nq_, uint32_t qbytes_, uint32_t k_, isk::Record* out, uint32_t* out_cnt)
        : h(h_), t(t_), nq(nq_), qbytes(qbytes_), k(k_), d_out(out), d_out_cnt(out_cnt) {}

    // (+ 1e-9: a product within rounding of an integer counts as that integer, so that a row outside the radius lies beyond the
    //  ratio by >= 1e-9 / bits -- orders of magnitude more than the rounding of the k-th distance the caller compares with it)
    int ratio_bits(const Job& j) const { const int bits = 8 * (int)j.pbytes; return std::min(bits, (int)std::floor(radius_ratio * bits + 1e-9)); }
    // the fixed threshold of a job's range-limited pass, or -1
    int job_radius(const Job& j) const {
        if (radius >= 0) return radius;
        if (radius_ratio >= 0 && !ratio_starts_self) return ratio_bits(j);
        return -1;
    }
    struct Ctx { isk::ScanParams sp; isk::SelectParams sl; };
    Ctx make_ctx(size_t ji) const {
        const Job& j = jobs[ji];
        Segment& s = *j.seg;
        Ctx c{};
        for (uint32_t w = 0; w < j.W; ++w) c.sp.col[w] = s.col[w];
        c.sp.queries = h->d_queries.p; c.sp.bias = h->d_bias.p; c.sp.cnt = h->d_cnt.p; c.sp.cand = h->d_cand.p;
        c.sp.ghist = h->d_ghist.p; c.sp.cap = cap; c.sp.k = k; c.sp.fold_tau = h->fold_tau; c.sp.nq_pad = nq_pad;
        c.sp.mask_lo = (uint32_t)j.mask_last; c.sp.mask_hi = (uint32_t)(j.mask_last >> 32);
        c.sp.thr_live = h->d_thr.p;
        c.sp.refresh_steps = h->self_refresh_steps;
        c.sl.cnt = h->d_cnt.p; c.sl.cand = h->d_cand.p; c.sl.cap = cap; c.sl.keys = s.keys;
        c.sl.rank = h->d_rank + (t.metric == ISCCSEARCH_METRIC_NPHD ? j.pbytes * 257 : 0);
        c.sl.out = multi ? h->d_lists.p + ji * (size_t)nq * k : d_out;
        c.sl.out_count = multi ? h->d_listcnt.p + ji * (size_t)nq : d_out_cnt;
        c.sl.overflow = d_flags + ji * (size_t)nq_pad;
        c.sl.k = k; c.sl.P = P; c.sl.prefix_bits = j.pbytes * 8; c.sl.q_base = 0;
        c.sl.overflow_count = mark_overflow ? isk::COUNT_OVERFLOW : 0;
        c.sl.out_rows = multi ? nullptr : d_out_rows;
        c.sl.out_kth = multi ? nullptr : d_out_kth;
        return c;
    }
    template <int NT>
    void launch_select_nt(const isk::SelectParams& sl, uint32_t blocks) const {
        if (sl.out_rows) {
            if (t.key_words == 2) hipLaunchKernelGGL((isk::select_kernel<2, true, NT>), dim3(blocks), dim3(NT), sel_lds, h->stream, sl);
            else hipLaunchKernelGGL((isk::select_kernel<1, true, NT>), dim3(blocks), dim3(NT), sel_lds, h->stream, sl);
        } else if (t.key_words == 2) hipLaunchKernelGGL((isk::select_kernel<2, false, NT>), dim3(blocks), dim3(NT), sel_lds, h->stream, sl);
        else hipLaunchKernelGGL((isk::select_kernel<1, false, NT>), dim3(blocks), dim3(NT), sel_lds, h->stream, sl);
    }
    // A large sort buffer leaves room for one or two blocks per CU (LDS): with 256 threads those are 4 - 8 waves walking ~60 bitonic stages
    // and two rounds of dependent gathers.  1 024-thread blocks when the launch cannot fill the chip with blocks anyway (fewer queries
    // than half the CUs: 10 M x 128-bit, 16 queries, k = 400: 0.148 -> 0.138 ms per call) and for the largest buffers (k = 2 000 over
    // 100 M rows x 1 024 queries: 6.06 -> 5.4 - 5.6 ms); many queries at k = 400 are no faster that way (0.59 -> 0.61 - 0.63 ms), they keep 256.
    void launch_select(const isk::SelectParams& sl, uint32_t blocks) const {
        const bool wide = sl.P >= h->select_wide_from && (sl.P >= 2 * h->select_wide_from || blocks <= (uint32_t)h->cus / 2);
        if (wide) launch_select_nt<1024>(sl, blocks);
        else launch_select_nt<isk::BLOCK>(sl, blocks);
    }
    // (a caller that sends small tables to the matrix cores -- mfma_min_rows lowered: the parity tests of those kernels -- gets them)
    bool tiny(const Job& j) const { return h->tiny_rows && j.seg->n <= h->tiny_rows && j.seg->n <= cap && j.seg->n < h->mfma_min_rows; }
    template <int NT>
    void launch_tiny_nt(const isk::TinyParams& tp, const isk::SelectParams& sl, const isk::InlineQueries& iq) const {
        if (sl.out_rows) {
            if (t.key_words == 2) hipLaunchKernelGGL((isk::tiny_search_kernel<2, true, NT>), dim3(nq), dim3(NT), sel_lds, h->stream, tp, sl, iq);
            else hipLaunchKernelGGL((isk::tiny_search_kernel<1, true, NT>), dim3(nq), dim3(NT), sel_lds, h->stream, tp, sl, iq);
        } else if (t.key_words == 2) hipLaunchKernelGGL((isk::tiny_search_kernel<2, false, NT>), dim3(nq), dim3(NT), sel_lds, h->stream, tp, sl, iq);
        else hipLaunchKernelGGL((isk::tiny_search_kernel<1, false, NT>), dim3(nq), dim3(NT), sel_lds, h->stream, tp, sl, iq);
    }
    size_t flag_words() const { return jobs.size() * (size_t)nq_pad; }

    // One scan launch over rows [sp.row_begin, sp.n_rows) for all query groups.  Large batches over enough rows go to
    // the matrix cores (mfma_scan.hip): every block keeps a chunk of up to 1 024 / W expanded queries in LDS and the
    // rows cross the memory system once per chunk; small batches stay on the XOR + popcount kernel, which is
    // HBM-bound up to ~11 queries per pass.  Both append the same candidates under the same thresholds.
    // (64-bit codes on the PACKED kernel win from 9 queries: 9 / 12 / 16 queries over 100 M rows 0.254 / 0.259 / 0.255 ms per step on the
    //  XOR + popcount kernel -- one pass of 16 -- against 0.206 / 0.203 / 0.197; 8 queries 0.168 against 0.208; longer codes tie at 16)
    // (... at 100 M rows.  Over a SMALL segment -- config 5's 10 M chunks -- the longer codes win there from 9 queries as well: one pass of 16
    //  on the XOR + popcount kernel streams 10 M x 128-bit rows at 2.1 TB/s, 16 queries x k = 400 per call 0.132 ms against 0.110 on the
    //  matrix cores, 256-bit 0.170 against 0.148; at 25 M rows 0.144 against 0.153, at 100 M 0.45 against 0.49: option "mfma_few_rows" (12 Mi), the segment size up to which)
    bool use_mfma(const Job& j, uint64_t rows) const {
        const bool from_nine = j.pack || j.seg->n <= h->mfma_few_rows;
        return h->mfma && nq_pad >= (from_nine ? std::min(h->mfma_min_queries, h->mfma_pack_min_queries) : h->mfma_min_queries) && rows >= h->mfma_min_rows;
    }
    int scan(const Job& j, const isk::ScanParams& sp, int mode, bool sample) {
        const uint64_t rows = sp.n_rows - sp.row_begin;
        // A self-tightening pass is decided once per job (use_mfma over the whole segment) and lives on the matrix cores: EVERY
        // stretch of it runs there, also a short last one -- the XOR + popcount kernels have no MODE_SELF
        if (use_mfma(j, rows) || mode == isk::MODE_SELF) {
            const uint32_t g = isk::mfma_groups_per_chunk((int)j.W, nq_pad, j.pack);
            const uint32_t chunks = (nq_pad + g * 32 - 1) / (g * 32);
            const bool pack3 = j.pack && h->mfma_pack3 && isk::mfma_pack3_fits(g);
            const uint64_t rps = isk::mfma_rows_per_wave_step((int)j.W, j.pack, pack3);
            const uint64_t steps = (rows + rps - 1) / rps;
            const uint64_t wpb = isk::mfma_waves_per_block();
            const uint64_t bx = std::max<uint64_t>(1, std::min<uint64_t>((steps + wpb - 1) / wpb, std::max<uint32_t>(1, (uint32_t)h->cus * isk::mfma_blocks_per_cu((int)j.W, g, j.pack) / chunks)));
            const int e = isk::launch_mfma_scan((int)j.W, mode, j.pack, (uint32_t)bx, g, h->stream, sp, pack3);
            if (e) return fail(-EIO, "mfma scan: chunk of %u query groups does not fit the LDS budget (%s)", g, hipGetErrorString((hipError_t)e));
            h->stats.mfma_launches += 1;
            if (j.pack) h->stats.mfma_pack_launches += 1;
            h->stats.mfma_pair_words += rows * (uint64_t)nq * j.W;
            return 0;
        }
        if (mode != isk::MODE_COLLECT && mode != isk::MODE_STRETCH && mode != isk::MODE_BOTH) return fail(-EINVAL, "scan mode %d has no XOR + popcount kernel", mode);
        if (sp.n_rows / (uint64_t)tile_rows_for((int)j.W) >= (1ull << 31)) return fail(-E2BIG, "segment of %llu rows exceeds the scan kernel's 2^31 tiles", (unsigned long long)sp.n_rows);
        launch_scan((int)j.W, j.mask, tq, mode, h->nontemporal, dim3(scan_grid_x(h, j.W, rows, groups, sample), groups), h->stream, sp);
        return 0;
    }

    // hq: host query words [nq][max_words]
    int begin(const uint64_t* hq) {
        jobs.clear();
        used_self = false;
        tq = h->tq;
        // 9..16 queries: ONE pass of 16 instead of two passes of 8 -- the pass is VALU-bound then, but the rows cross the memory
        // system once and half the launches go (100 M x 64-bit: 0.31 against 0.41 ms; 256-bit: 0.87 against 1.48; no loss at 10 M)
        if (tq == 8 && nq > 8 && nq <= 16) tq = 16;
        nq_pad = (nq + tq - 1) / tq * tq;
        groups = nq_pad / tq;
        for (uint32_t b = 1; b <= ISCCSEARCH_MAX_BYTES; ++b) {
            Segment& s = t.seg[b];
            if (!s.n) continue;
            Job j;
            j.seg = &s;
            j.pbytes = t.metric == ISCCSEARCH_METRIC_NPHD ? std::min(b, qbytes) : b;
            j.W = (j.pbytes + 7) / 8;
            j.mask = (j.pbytes & 7) != 0;
            j.mask_last = mask_for(j.pbytes);
            // the packed fold of mfma_pack_kernel holds a dot product in 7 bits + sign: -64 .. 63.  +64 takes an all-zero query
            // of 64 compared bits (against a row of all ones): such a batch stays on the unpacked kernel
            j.pack = h->mfma_pack && j.W == 1;
            if (j.pack && j.pbytes == 8)
                for (uint32_t q = 0; q < nq && j.pack; ++q) j.pack = hq[(size_t)q * t.max_words] != 0;
            jobs.push_back(j);
        }
        if (jobs.empty()) {
            HIPOK(hipMemsetAsync(d_out_cnt, 0, nq * sizeof(uint32_t), h->stream));
            return 0;
        }
        cap = std::max<uint32_t>(h->candidate_cap, 16 * k);
        // the self-tightening pass never prunes: ~17 k entries per query over 100 M rows (+ the flood of the first steps)
        if (h->self_tighten && h->mfma && k <= h->self_max_k && radius < 0 && radius_ratio < 0) cap = std::max<uint32_t>(cap, 64 * k);
        multi = jobs.size() > 1;
        // select's LDS sort buffer: room for the k winners AND the tie class at the cut -- with 65 distinct distances the class is
        // ~1.5-2.5 k rows at simprint-sized k, and a list that does not fit takes up to 8 / 16 radix passes over its gathered keys first
        // (10 M x 64-bit, 512 queries, k = 400: 154 us per select with 1 024 slots; profiles/r04_candidate_path.txt)
        P = next_pow2(std::max<uint32_t>(std::max<uint32_t>(k, 1024), std::min<uint32_t>(4 * k, 4096)));
        sel_lds = (((size_t)P * 4 + 15) & ~(size_t)15) + (size_t)P * 8 * t.key_words + (d_out_rows ? (size_t)P * 4 : 0);
        int rc;
        if ((rc = h->d_queries.ensure((size_t)nq_pad * 4))) return rc;
        if ((rc = h->d_bias.ensure(nq_pad))) return rc;
        if ((rc = h->d_thr.ensure(nq_pad))) return rc;
        if ((rc = h->d_cnt.ensure((size_t)nq_pad * isk::CNT_STRIDE))) return rc;
        if ((rc = h->d_ghist.ensure((size_t)nq_pad * isk::HB))) return rc;
        if (!d_flags) {
            if ((rc = h->d_overflow.ensure(flag_words()))) return rc;
            d_flags = h->d_overflow.p;
        }
        if ((rc = h->d_cand.ensure((size_t)nq_pad * cap))) return rc;
        if (multi) {
            if ((rc = h->d_lists.ensure(jobs.size() * (size_t)nq * k))) return rc;
            if ((rc = h->d_listcnt.ensure(jobs.size() * (size_t)nq))) return rc;
        }
        // stage queries through pinned memory: [nq_pad][4], padded words zero.  An asynchronous caller may come back before the
        // previous batch's query upload has left the staging buffer: wait for it before the buffer is grown or rewritten
        if (h->ev_staged_pending) { HIPOK(hipEventSynchronize(h->ev_staged)); h->ev_staged_pending = false; }
        if ((rc = h->p_queries.ensure(pq_off + (size_t)nq_pad * 4))) return rc;   // (no-op when the caller pre-sized it)
        uint64_t* const pq = h->p_queries.p + pq_off;
        memset(pq, 0, (size_t)nq_pad * 4 * 8);
        for (uint32_t q = 0; q < nq; ++q)
            for (int w = 0; w < t.max_words; ++w) pq[(size_t)q * 4 + w] = hq[(size_t)q * t.max_words + w];
        // (a range-limited search of <= 16 queries over one segment -- the speculative single pass of search_locked -- carries its
        //  queries in the ARGUMENTS of its first kernel, which writes them to d_queries: one stream operation less, ~8 us of 170)
        // (... and so do the one-launch searches of tiny segments: when every job of the batch is one, nothing is uploaded at all)
        bool all_tiny = true;
        for (const Job& j : jobs) all_tiny = all_tiny && tiny(j);
        const bool tiny_inline = all_tiny && nq_pad <= isk::INLINE_QUERIES;
        const bool inline_queries = !all_tiny && radius >= 0 && nq_pad <= isk::INLINE_QUERIES && jobs.size() == 1;
        if (!inline_queries && !tiny_inline) HIPOK(hipMemcpyAsync(h->d_queries.p, pq, (size_t)nq_pad * 4 * 8, hipMemcpyHostToDevice, h->stream));
        if (mark_overflow) { HIPOK(hipEventRecord(h->ev_staged, h->stream)); h->ev_staged_pending = true; }

        for (size_t ji = 0; ji < jobs.size(); ++ji) {
            const Job& j = jobs[ji];
            Segment& s = *j.seg;
            Ctx c = make_ctx(ji);
            isk::ScanParams& sp = c.sp;
            const int jr = job_radius(j);

            if (tiny(j)) {
                // ONE launch: distances of every row, candidate list, select -- exact, nothing to verify or to repeat
                isk::TinyParams tp{};
                for (uint32_t w = 0; w < j.W; ++w) tp.col[w] = s.col[w];
                tp.queries = h->d_queries.p; tp.cand = h->d_cand.p; tp.mask_last = j.mask_last; tp.n_rows = (uint32_t)s.n; tp.W = j.W;
                tp.radius = jr; tp.use_inline = tiny_inline ? 1u : 0u;
                isk::InlineQueries iq;
                if (tiny_inline) memcpy(iq.w, pq, (size_t)nq_pad * 4 * 8);
                else memset(iq.w, 0, sizeof iq.w);
                hipEvent_t e0 = nullptr, e1 = nullptr;
                if (h->profile) { if ((rc = event_pair(h, e0, e1))) return rc; HIPOK(hipEventRecord(e0, h->stream)); }
                // (a block walks ALL rows: 1 024 threads whenever the batch leaves the chip room for them, and for the sort buffers select_kernel gives them)
                const bool wide = (s.n > 2048 && nq <= (uint32_t)h->cus / 2) || c.sl.P >= 2 * h->select_wide_from || (c.sl.P >= h->select_wide_from && nq <= (uint32_t)h->cus / 2);
                if (wide) launch_tiny_nt<1024>(tp, c.sl, iq);
                else launch_tiny_nt<isk::BLOCK>(tp, c.sl, iq);
                HIPOK(hipGetLastError());
                if (h->profile) HIPOK(hipEventRecord(e1, h->stream));
                h->stats.scan_launches += 1;
                h->stats.scan_passes += nq;
                h->stats.scan_bytes += s.n * 8 * j.W * nq;
                h->stats.scan_pair_words += s.n * (uint64_t)nq * j.W;
                continue;
            }

            // the collect pass over rows [from, n) within the thresholds in force.  With more than one query group the
            // rows are taken in STRETCHES that fit the Infinity Cache (option "stretch_mb", default 128 of its
            // 256 MB): all groups of a launch walk the same stretch, so it comes out of HBM once and out of the
            // caches for every further group -- the pass is then bound by the VALU, not by HBM.
            const uint64_t tile_rows = (uint64_t)tile_rows_for((int)j.W);
            bool hist_live = false;
            auto collect_from = [&](uint64_t from, bool self = false) -> int {
                uint64_t stretch = s.n;
                // (the MFMA kernel reads the rows once per CHUNK of up to 1 024 / W queries: one chunk has nothing to share)
                const bool shared = use_mfma(j, s.n - from) ? nq_pad > isk::mfma_groups_per_chunk((int)j.W, nq_pad, j.pack) * 32 : groups > 1;
                // (matrix-core launches: the chunks' blocks are all resident and walk a stretch in step, so three times the size
                //  still shares it in the caches and every launch saved is ~30 us of ramp and tail.  Same box, factor 1 / 2 / 3 / 4:
                //  256-bit 9.31 / 8.90 / 8.79 / 8.72 ms, 128-bit 4.67 / 4.55 / 4.53 / 4.52, 192-bit 7.88 / 7.74 / 7.67 / 7.99)
                const uint64_t stretch_bytes = use_mfma(j, s.n - from) ? h->stretch_bytes * h->mfma_stretch_factor : h->stretch_bytes;
                if (shared && stretch_bytes) stretch = std::max<uint64_t>(tile_rows, stretch_bytes / (8 * j.W) / tile_rows * tile_rows);
                for (uint64_t a = from; a < s.n;) {
                    const uint64_t b = s.n - a <= stretch + stretch / 4 ? s.n : a + stretch;     // no sliver at the end
                    sp.row_begin = a;
                    sp.n_rows = b;
                    const uint64_t rows = b - a;
                    hipEvent_t e0 = nullptr, e1 = nullptr;
                    int rcl = 0;
                    if (h->profile) { if ((rcl = event_pair(h, e0, e1))) return rcl; HIPOK(hipEventRecord(e0, h->stream)); }
                    // every stretch but the last keeps the histogram and is followed by a pick, so the threshold keeps
                    // tightening through the pass (free for k = 10, +2.5 % for k = 100; it is also what lets the
                    // folded fast path of scan_adapt_kernel switch on as the pass advances)
                    // (the last stretch keeps the histogram too -- a handful of atomics -- so that the whole pass is ONE
                    // kernel instantiation, MODE_STRETCH; it just is not followed by a pick)
                    const bool hist_too = h->repick && jr < 0;
                    const bool repick = hist_too && b < s.n && !self;
                    if (self) {
                        if ((rcl = scan(j, sp, isk::MODE_SELF, false))) return rcl;
                    } else if (hist_too) {
                        if (!hist_live) { HIPOK(hipMemsetAsync(h->d_ghist.p, 0, (size_t)nq_pad * isk::HB * sizeof(uint32_t), h->stream)); hist_live = true; }
                        if ((rcl = scan(j, sp, isk::MODE_STRETCH, false))) return rcl;
                    } else {
                        if ((rcl = scan(j, sp, isk::MODE_COLLECT, false))) return rcl;
                    }
                    if (h->profile) HIPOK(hipEventRecord(e1, h->stream));
                    if (repick) {
                        isk::PickParams pp{h->d_ghist.p, h->d_bias.p, nq, (uint32_t)std::min<uint64_t>(k, b), h->d_cnt.p, h->d_cand.p, cap};
                        hipLaunchKernelGGL(isk::pick_kernel, dim3(nq), dim3(isk::BLOCK), 0, h->stream, pp);
                    }
                    h->stats.scan_launches += 1;
                    h->stats.scan_passes += groups;
                    h->stats.scan_bytes += rows * 8 * j.W * groups;
                    h->stats.scan_pair_words += rows * (uint64_t)nq * j.W;
                    if (use_mfma(j, rows) || self) h->stats.scan_mfma_launches += 1;
                    a = b;
                }
                return 0;
            };

            if (jr >= 0) {
                // range-limited search: the threshold is given, so one streaming pass collects everything
                if (inline_queries) {
                    isk::InlineQueries iq;
                    memcpy(iq.w, pq, (size_t)nq_pad * 4 * 8);
                    hipLaunchKernelGGL(isk::radius_init_inline_kernel, dim3(1), dim3(isk::BLOCK), 0, h->stream,
                                       h->d_bias.p, h->d_cnt.p, nq, nq_pad, 0x7FFFFFFFu - (uint32_t)jr, h->d_queries.p, iq);
                } else
                hipLaunchKernelGGL(isk::radius_init_kernel, dim3((nq_pad + isk::BLOCK - 1) / isk::BLOCK), dim3(isk::BLOCK), 0, h->stream,
                                   h->d_bias.p, h->d_cnt.p, nq, nq_pad, 0x7FFFFFFFu - (uint32_t)jr);
                if ((rc = collect_from(0))) return rc;
                launch_select(c.sl, nq);
                HIPOK(hipGetLastError());
                continue;
            }

            // 1. bootstrap threshold from the first s0 rows
            //    Large batches with k <= self_max_k take ONE pass on the matrix cores with self-tightening thresholds (MODE_SELF).
            //    (The XOR + popcount kernels keep the levels: their resident blocks cover ~4 M rows -- 16 M by the time a second
            //    tile could see a new threshold -- before any update reaches them, and fresh thresholds must be read past the
            //    per-XCD L2s (sc1 / glc), where 8 192 waves hammering one line serialise: measured 0.24-0.53 ms for 1-8
            //    queries over 100 M rows against 0.10 ms for the collect pass of the level design.)
            const bool self = allow_self && h->self_tighten && k <= h->self_max_k && use_mfma(j, s.n);
            used_self = used_self || self;
            // (the single pass appends everything within the bootstrap threshold until the first update arrives -- 3 072 waves x
            //  128 rows at once -- so its sample grows with k (1 024 k rows): 512 k measured 4.39 -> 3.80 ms at k = 256 and 11.9 (list
            //  overflow, retry) -> 5.07 ms at k = 512 against the fixed 65 536, profiles/r03_ab_large_k.txt)
            const uint64_t s0 = std::min<uint64_t>(s.n, self ? std::max<uint64_t>(h->self_boot_rows, std::min<uint64_t>((uint64_t)h->self_boot_per_k * k, s.n / 8))
                                                             : std::max<uint64_t>(h->boot_rows, std::min<uint64_t>(65536, 64ull * k)));
            isk::BootParams bp{};
            for (uint32_t w = 0; w < j.W; ++w) bp.col[w] = s.col[w];
            bp.queries = h->d_queries.p; bp.bias = h->d_bias.p; bp.cnt = h->d_cnt.p; bp.s0 = s0; bp.nq = nq; bp.k = k; bp.W = j.W; bp.mask_last = j.mask_last;
            bp.thr = self ? h->d_thr.p : nullptr;
            bp.thr_packed = j.pack ? 1u : 0u;          // mfma_pack_kernel keeps (and lowers) its live thresholds packed
            bp.counts = h->d_ghist.p;          // zeroed by the kernel: the running histogram of the levels / the counters of MODE_SELF
            bp.hint = isk::BOOT_NO_HINT;
            hist_live = true;
            const int job_hint = self_hint >= 0 ? self_hint : (radius_ratio >= 0 && ratio_starts_self ? ratio_bits(j) : -1);
            if (self && job_hint >= 0) {
                // the threshold a previous batch of this size ended at (+ margin) instead of a sample: no 65 536-row bootstrap, and
                // the pass starts ~6 bits tighter -- without the flood of its first steps.  Verified by the caller.
                bp.hint = (uint32_t)job_hint;
                used_hint = true;
                hipLaunchKernelGGL(isk::boot_kernel, dim3(nq_pad), dim3(64), 0, h->stream, bp);
            } else if (nq_pad > 64 && h->boot_multi) {
                // large batches: four queries per 1 024-thread block share every row load of the sample
                const dim3 bgrid(nq_pad / isk::BOOT_QB), bblock(1024);
                switch (j.W) {
                    case 1: hipLaunchKernelGGL(isk::boot_multi_kernel<1>, bgrid, bblock, 0, h->stream, bp); break;
                    case 2: hipLaunchKernelGGL(isk::boot_multi_kernel<2>, bgrid, bblock, 0, h->stream, bp); break;
                    case 3: hipLaunchKernelGGL(isk::boot_multi_kernel<3>, bgrid, bblock, 0, h->stream, bp); break;
                    default: hipLaunchKernelGGL(isk::boot_multi_kernel<4>, bgrid, bblock, 0, h->stream, bp); break;
                }
            } else {
                // one block per query: a handful of queries get wide blocks, or a 65 536-row sample is one block's latency-bound walk
                hipLaunchKernelGGL(isk::boot_kernel, dim3(nq_pad), dim3(nq_pad <= 64 ? 1024 : isk::BLOCK), 0, h->stream, bp);
            }

            if (self) {
                // 2'. ONE pass over all rows (in cache-sized stretches when several chunks of queries share them):
                //     every wave appends what lies within the live threshold of its query and counts it per distance; the lane
                //     that proves "k rows within t" lowers the threshold for everybody (mfma_scan.hip, MODE_SELF).
                //     No levels, no picks; the lists stay unpruned (~k ln(n / s0) entries + ties + the first steps' flood) and
                //     select_kernel takes the exact top-k.  (boot_kernel has zeroed the counters.)
                if ((rc = collect_from(0, true))) return rc;
                launch_select(c.sl, nq);
                HIPOK(hipGetLastError());
                continue;
            }

            // 2. levels: every level streams the NEXT stretch of rows [done, end) exactly once under the threshold of the
            //    rows before it, collecting its candidates and adding them to the running histogram (MODE_BOTH);
            //    pick_kernel then tightens the threshold to the k-th best so far and prunes the candidate list to
            //    it.  A level meets ~k * growth candidates per query, so the stretches grow geometrically (8x;
            //    64x when there are so few query groups that launch gaps outweigh candidate handling; less
            //    when k * growth would not fit the candidate buffer).  No row is read twice.
            uint64_t growth = (groups <= 2 && k <= 64) ? std::max<uint64_t>(64, h->level_growth) : h->level_growth;
            if (use_mfma(j, s.n) && k <= 64) growth = h->mfma_level_growth;   // matrix-core launches: see the option's comment
            if (k >= 256) growth = std::min<uint64_t>(growth, 2);   // simprint-sized k: candidate handling dominates, +10 % with short levels
            // a stretch `growth` times the rows seen so far brings ~growth * (rows at or under tau) candidates, and the
            // tie class at tau can make that 2.3x k (ratio of consecutive binomial tails): keep it inside the buffer
            while (growth > 2 && (uint64_t)k * growth * 5 / 2 > (uint64_t)cap * 9 / 10) growth /= 2;
            uint64_t done = 0;                    // rows [0, done) are collected and in the histogram
            uint64_t reach = s0;                  // the threshold in force comes from rows [0, reach)
            for (;;) {
                uint64_t end = reach >= s.n / growth ? s.n : reach * growth;
                if (end < s.n) end = end / tile_rows * tile_rows;
                if (end <= done || end + tile_rows > s.n) end = s.n;
                const bool last = end == s.n;
                if (last) break;                  // the final stretch is the streaming pass below
                if (!hist_live) {
                    HIPOK(hipMemsetAsync(h->d_ghist.p, 0, (size_t)nq_pad * isk::HB * sizeof(uint32_t), h->stream));
                    hist_live = true;
                }
                sp.row_begin = done;
                sp.n_rows = end;
                {
                    hipEvent_t e0 = nullptr, e1 = nullptr;
                    if (h->profile) { if ((rc = event_pair(h, e0, e1, true))) return rc; HIPOK(hipEventRecord(e0, h->stream)); }
                    if ((rc = scan(j, sp, isk::MODE_BOTH, true))) return rc;
                    if (h->profile) HIPOK(hipEventRecord(e1, h->stream));
                    h->stats.level_launches += 1;
                    h->stats.level_pair_words += (end - done) * (uint64_t)nq * j.W;
                    if (use_mfma(j, end - done)) h->stats.level_mfma_launches += 1;
                }
                isk::PickParams pp{h->d_ghist.p, h->d_bias.p, nq, (uint32_t)std::min<uint64_t>(k, end), h->d_cnt.p, h->d_cand.p, cap};
                hipLaunchKernelGGL(isk::pick_kernel, dim3(nq), dim3(isk::BLOCK), 0, h->stream, pp);
                h->stats.sample_bytes += (end - done) * 8 * j.W * groups;
                done = reach = end;
            }
            const uint64_t collected_to = done;

            // 3. the collect pass over everything the levels have not covered
            if ((rc = collect_from(collected_to))) return rc;

            // 4. exact select of the k best candidates per query (flags candidate-list overflow)
            launch_select(c.sl, nq);
            HIPOK(hipGetLastError());
        }
        return 0;
    }

    // queue the overflow flags for the host (pinned); valid after the next stream synchronisation.  Flags that ride in the
    // caller's result block (h_flags set) come with its copy instead.
    int copy_flags() {
        if (jobs.empty() || h_flags) return 0;
        int rc;
        if ((rc = h->p_flags.ensure(flag_words()))) return rc;
        HIPOK(hipMemcpyAsync(h->p_flags.p, d_flags, flag_words() * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
        return 0;
    }
    // flags of the padding queries are never written: look at the real ones only
    bool flagged(size_t ji, uint32_t q) const { return (h_flags ? h_flags : h->p_flags.p)[ji * nq_pad + q] != 0; }
    bool any_flag() const {
        for (size_t ji = 0; ji < jobs.size(); ++ji)
            for (uint32_t q = 0; q < nq; ++q) if (flagged(ji, q)) return true;
        return false;
    }
    // a range-limited or hinted pass over `rows` rows is the exact answer when no list overflowed and every query found
    // min(k, rows) rows under its threshold (its k nearest are then among them)
    bool complete(const uint32_t* cnt, uint64_t rows) const {
        if (any_flag()) return false;
        const uint32_t need = (uint32_t)std::min<uint64_t>(k, rows);
        for (uint32_t q = 0; q < nq; ++q) if (cnt[q] < need) return false;
        return true;
    }

    // exact fallback for every flagged (job, query): full histogram -> exact threshold -> collect into
    // a buffer sized to the tie class -> select.  Synchronous; rare.
    int fix() {
        int rc;
        for (size_t ji = 0; ji < jobs.size(); ++ji) {
            const Job& j = jobs[ji];
            Segment& s = *j.seg;
            for (uint32_t q = 0; q < nq; ++q) {
                if (!flagged(ji, q)) continue;
                Ctx c = make_ctx(ji);
                h->stats.fallback_queries += 1;
                if ((rc = h->d_misc.ensure(isk::HB + 256 + 16))) return rc;   // full histogram + one key-byte histogram
                uint32_t* d_fh = reinterpret_cast<uint32_t*>(h->d_misc.p);
                HIPOK(hipMemsetAsync(d_fh, 0, isk::HB * sizeof(uint32_t), h->stream));
                isk::FullHistParams fp{};
                for (uint32_t w = 0; w < j.W; ++w) fp.col[w] = s.col[w];
                fp.n_rows = s.n; fp.query = h->d_queries.p + (size_t)q * 4; fp.ghist = d_fh; fp.W = j.W; fp.mask_last = j.mask_last;
                const uint32_t fgrid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((s.n + isk::BLOCK - 1) / isk::BLOCK, (uint64_t)h->cus * 8));
                hipLaunchKernelGGL(isk::fullhist_kernel, dim3(fgrid), dim3(isk::BLOCK), 0, h->stream, fp);
                uint32_t fh[isk::HB];
                HIPOK(hipMemcpyAsync(fh, d_fh, sizeof fh, hipMemcpyDeviceToHost, h->stream));
                HIPOK(hipStreamSynchronize(h->stream));
                uint64_t cum = 0, less = 0;
                uint32_t tau = 256;
                uint64_t within = s.n;               // rows a range-limited search may report at all
                if (radius >= 0) {
                    within = 0;
                    for (uint32_t b = 0; b < isk::NBINS && b <= (uint32_t)radius; ++b) within += fh[b];
                }
                const uint64_t need = std::min<uint64_t>(std::min<uint64_t>(k, s.n), within);
                if (need == 0) {
                    HIPOK(hipMemsetAsync(c.sl.out_count + q, 0, sizeof(uint32_t), h->stream));
                    HIPOK(hipMemsetAsync(c.sl.overflow + q, 0, sizeof(uint32_t), h->stream));
                    continue;
                }
                for (uint32_t b = 0; b < isk::NBINS; ++b) { less = cum; cum += fh[b]; if (cum >= need) { tau = b; break; } }
                // `less` rows lie strictly below tau, `cum - less` rows tie at tau.  When the tie class is too
                // large to collect, pin down the r = need - less smallest KEYS of it by radix select over
                // the table (8 bits of the key per pass) until what must be collected fits the buffer.
                const uint32_t small_cap = std::max<uint32_t>(cap, 65536);
                isk::FbParams fb{};
                for (uint32_t w = 0; w < j.W; ++w) fb.col[w] = s.col[w];
                fb.keys = s.keys; fb.n_rows = s.n; fb.query = h->d_queries.p + (size_t)q * 4;
                fb.W = j.W; fb.KW = (uint32_t)t.key_words; fb.mask_last = j.mask_last; fb.tau = tau;
                fb.d = 0; fb.phi = 0; fb.plo = 0;
                uint64_t collect = cum;              // rows the final collect will append
                uint64_t r_need = need - less, tie = cum - less;
                while (collect > small_cap && fb.d < t.key_words * 8 && r_need < tie) {
                    uint32_t* d_kh = reinterpret_cast<uint32_t*>(h->d_misc.p) + isk::HB;
                    HIPOK(hipMemsetAsync(d_kh, 0, 256 * sizeof(uint32_t), h->stream));
                    fb.ghist = d_kh;
                    if (t.key_words == 2) hipLaunchKernelGGL(isk::fb_keyhist_kernel<2>, dim3(fgrid), dim3(isk::BLOCK), 0, h->stream, fb);
                    else hipLaunchKernelGGL(isk::fb_keyhist_kernel<1>, dim3(fgrid), dim3(isk::BLOCK), 0, h->stream, fb);
                    uint32_t kh[256];
                    HIPOK(hipMemcpyAsync(kh, d_kh, sizeof kh, hipMemcpyDeviceToHost, h->stream));
                    HIPOK(hipStreamSynchronize(h->stream));
                    uint64_t below = 0;
                    uint32_t digit = 255;
                    for (uint32_t b = 0; b < 256; ++b) { if (below + kh[b] >= r_need) { digit = b; break; } below += kh[b]; }
                    // keys with a smaller byte are all taken; the bucket `digit` holds the cut
                    less += below;
                    r_need -= below;
                    tie = kh[digit];
                    const int sh = 56 - 8 * (t.key_words == 2 ? (fb.d < 8 ? fb.d : fb.d - 8) : fb.d);
                    if (t.key_words == 2 && fb.d < 8) fb.phi |= (uint64_t)digit << sh;
                    else fb.plo |= (uint64_t)digit << sh;
                    fb.d += 1;
                    collect = less + tie;            // everything below the cut + the whole cut bucket
                }
                if (collect > 0xFFFFFFFFull) return fail(-E2BIG, "tie class of %llu rows exceeds the fallback buffer", (unsigned long long)collect);
                if ((rc = h->d_misc2.ensure((size_t)collect + 8))) return rc;
                // collect into a private buffer addressed as candidate list of query q
                HIPOK(hipMemsetAsync(h->d_cnt.p + (size_t)q * isk::CNT_STRIDE, 0, sizeof(uint32_t), h->stream));
                fb.cnt = h->d_cnt.p + (size_t)q * isk::CNT_STRIDE;
                fb.cand = h->d_misc2.p;
                fb.cap = (uint32_t)collect;
                if (t.key_words == 2) hipLaunchKernelGGL(isk::fb_collect_kernel<2>, dim3(fgrid), dim3(isk::BLOCK), 0, h->stream, fb);
                else hipLaunchKernelGGL(isk::fb_collect_kernel<1>, dim3(fgrid), dim3(isk::BLOCK), 0, h->stream, fb);
                isk::SelectParams fsl = c.sl;
                fsl.cnt = h->d_cnt.p; fsl.cap = fb.cap; fsl.q_base = q;
                fsl.cand = reinterpret_cast<const uint64_t*>(reinterpret_cast<uintptr_t>(h->d_misc2.p) - (uintptr_t)q * fsl.cap * 8);
                HIPOK(hipMemsetAsync(c.sl.overflow + q, 0, sizeof(uint32_t), h->stream));
                launch_select(fsl, 1);
                HIPOK(hipGetLastError());
                HIPOK(hipStreamSynchronize(h->stream));
            }
        }
        return 0;
    }

    int merge() {
        if (!multi) return 0;
        isk::MergeParams mp{reinterpret_cast<const unsigned char*>(h->d_lists.p), reinterpret_cast<const unsigned char*>(h->d_listcnt.p),
                            (uint64_t)nq * k * sizeof(isk::Record), (uint64_t)nq * sizeof(uint32_t),
                            d_out, d_out_cnt, (uint32_t)jobs.size(), nq, k};
        hipLaunchKernelGGL(isk::merge_kernel, dim3(nq), dim3(isk::BLOCK), 0, h->stream, mp);
        HIPOK(hipGetLastError());
        return 0;
    }

    // The single pass never prunes its candidate lists; when one overflows (huge tie classes, clustered codes) the WHOLE batch
    // is answered again by the level design, which prunes after every level -- one more batch pass instead of one exact
    // full-table fallback per flagged query.  What is still flagged afterwards goes to fix().
    int retry_with_levels(const uint64_t* hq) {
        allow_self = false;
        h->stats.self_retries += 1;
        return begin(hq);
    }

    // Everything after begin(): the flags (and what `queue_results` queues) reach the host behind one synchronisation, an
    // overflowed single pass is redone by retry_with_levels(), fix() answers what is still flagged, several lists are merged.
    // One segment: the results travel with the flags, and again after fix().  Several segments: the lists are complete before
    // the merge, and the merged results leave after it.  Without `queue_results` (device-resident results) nothing follows the
    // last step, and a batch without jobs is not synchronised at all.
    int finish(const uint64_t* hq, const std::function<int()>& queue_results = nullptr) {
        if (jobs.empty() && !queue_results) return 0;
        const bool with_flags = queue_results && !multi;
        auto settle = [&]() -> int {
            int rs;
            if ((rs = copy_flags())) return rs;
            if (with_flags && (rs = queue_results())) return rs;
            HIPOK(hipStreamSynchronize(h->stream));
            return 0;
        };
        int rc;
        if ((rc = settle())) return rc;
        if (used_self && any_flag()) {
            if ((rc = retry_with_levels(hq))) return rc;
            if ((rc = settle())) return rc;
        }
        const bool fixed = any_flag();
        if (fixed && (rc = fix())) return rc;
        if ((rc = merge())) return rc;
        if (queue_results && (multi || fixed)) {
            if ((rc = queue_results())) return rc;
            HIPOK(hipStreamSynchronize(h->stream));
        }
        return 0;
    }
};

// where a batch's lists ended -- the worst k-th distance, read off the records or off `kth` (the lists' last distances) -- is
// where the next small batch of the class starts (+ a margin: P(h <= t) grows ~3x per step at these distances, so it costs a
// handful of candidates and absorbs the spread between queries): hit() after a speculative pass that held, seed() after any other
void record_hint(Segment::SpecHint& hint, bool spec_ok, uint32_t nq, uint32_t k, const uint32_t* cnt, const isk::Record* rec, const uint32_t* kth) {
    uint32_t worst = 0;
    for (uint32_t i = 0; i < nq; ++i)
        if (cnt[i]) worst = std::max<uint32_t>(worst, kth ? kth[i] : rec[(size_t)i * k + cnt[i] - 1].hamming);
    if (spec_ok) hint.hit(worst);
    else hint.seed(k, worst);
}

void unpack_range(const isk::Record* rec, const uint32_t* cnt, uint32_t q_begin, uint32_t q_end, uint32_t k, int key_words,
                  const uint32_t* dest_index, uint64_t* out_keys, uint32_t* out_h, uint16_t* out_p, uint32_t* out_c);

// Records -> the caller's arrays.  A large block (k in the hundreds x a full batch: 10^5..10^6 records, 0.1-0.5 ms on one core,
// up to 14 % of such a step) is split by query over a few threads; the usual block (1 024 x 10 records) is done in place.
// Workers for the host side of LARGE result blocks (a simprint-sized search returns 512 x 400 records: 4.9 MB of {key, distance}
// records to split into the caller's arrays).  One thread takes 270 us for them, four threads started per call 140 (a thread
// start costs ~25 us), eight started per call 190-240; the same eight kept waiting here ~60.  Started on first use, one pool per
// process; a call hands out slices of queries and waits for them.
class UnpackPool {
public:
    static UnpackPool& get() { static UnpackPool pool; return pool; }
    // runs fn(slice) for slice = 0 .. slices - 1, the caller taking part
    void run(uint32_t slices, const std::function<void(uint32_t)>& fn) {
        std::lock_guard<std::mutex> one_at_a_time(call_mu_);
        {
            std::unique_lock<std::mutex> lk(mu_);
            done_.wait(lk, [&] { return active_ == 0; });       // (a worker that woke late for the previous call is still leaving)
            fn_ = &fn;
            slices_ = slices;
            next_.store(0, std::memory_order_relaxed);
            left_ = slices;
            generation_ += 1;
        }
        cv_.notify_all();
        work();
        std::unique_lock<std::mutex> lk(mu_);
        done_.wait(lk, [&] { return left_ == 0; });
    }
    uint32_t workers() const { return (uint32_t)threads_.size(); }

private:
    UnpackPool() {
        const uint32_t hw = std::thread::hardware_concurrency();
        const uint32_t n = std::min<uint32_t>(7u, hw > 1 ? hw - 1 : 0);
        for (uint32_t i = 0; i < n; ++i) threads_.emplace_back([this] { loop(); });
    }
    ~UnpackPool() {
        { std::lock_guard<std::mutex> lk(mu_); stop_ = true; }
        cv_.notify_all();
        for (auto& t : threads_) t.join();
    }
    void work() {
        for (;;) {
            const uint32_t i = next_.fetch_add(1, std::memory_order_relaxed);
            if (i >= slices_) return;
            (*fn_)(i);
            std::lock_guard<std::mutex> lk(mu_);
            if (--left_ == 0) done_.notify_all();
        }
    }
    void loop() {
        uint64_t seen = 0;
        for (;;) {
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [&] { return stop_ || generation_ != seen; });
                if (stop_) return;
                seen = generation_;
                active_ += 1;
            }
            work();
            std::lock_guard<std::mutex> lk(mu_);
            if (--active_ == 0) done_.notify_all();
        }
    }
    std::mutex call_mu_, mu_;
    std::condition_variable cv_, done_;
    std::vector<std::thread> threads_;
    const std::function<void(uint32_t)>* fn_ = nullptr;
    std::atomic<uint32_t> next_{0};
    uint32_t slices_ = 0, left_ = 0, active_ = 0;
    uint64_t generation_ = 0;
    bool stop_ = false;
};

void unpack_records(const isk::Record* rec, const uint32_t* cnt, uint32_t nq, uint32_t k, int key_words,
                    const uint32_t* dest_index /*nullable: original query index per row*/,
                    uint64_t* out_keys, uint32_t* out_h, uint16_t* out_p, uint32_t* out_c) {
    const uint64_t records = (uint64_t)nq * k;
    if (records < (1u << 16) || nq < 2) {
        unpack_range(rec, cnt, 0, nq, k, key_words, dest_index, out_keys, out_h, out_p, out_c);
        return;
    }
    UnpackPool& pool = UnpackPool::get();
    const uint32_t slices = std::min<uint32_t>(nq, 2 * (pool.workers() + 1));
    pool.run(slices, [&](uint32_t i) {
        unpack_range(rec, cnt, (uint32_t)((uint64_t)nq * i / slices), (uint32_t)((uint64_t)nq * (i + 1) / slices), k, key_words, dest_index, out_keys, out_h, out_p, out_c);
    });
}

void unpack_range(const isk::Record* rec, const uint32_t* cnt, uint32_t q_begin, uint32_t q_end, uint32_t k, int key_words,
                  const uint32_t* dest_index, uint64_t* out_keys, uint32_t* out_h, uint16_t* out_p, uint32_t* out_c) {
    for (uint32_t q = q_begin; q < q_end; ++q) {
        const uint32_t dq = dest_index ? dest_index[q] : q;
        const uint32_t c = cnt[q] == isk::COUNT_OVERFLOW ? 0 : std::min(cnt[q], k);
        out_c[dq] = cnt[q] == isk::COUNT_OVERFLOW ? isk::COUNT_OVERFLOW : c;
        for (uint32_t i = 0; i < k; ++i) {
            const size_t o = (size_t)dq * k + i;
            if (i < c) {
                const isk::Record& r = rec[(size_t)q * k + i];
                if (key_words == 2) { out_keys[2 * o] = r.key_hi; out_keys[2 * o + 1] = r.key_lo; }
                else out_keys[o] = r.key_lo;
                out_h[o] = r.hamming;
                out_p[o] = r.prefix_bits;
            } else {
                if (key_words == 2) { out_keys[2 * o] = 0; out_keys[2 * o + 1] = 0; }
                else out_keys[o] = 0;
                out_h[o] = 0;
                out_p[o] = 0;
            }
        }
    }
}

int check_query_lengths(const Table& t, uint32_t nq, const uint8_t* q_nbytes) {
    if (t.metric == ISCCSEARCH_METRIC_HAMMING) {
        if (q_nbytes)
            for (uint32_t q = 0; q < nq; ++q)
                if (q_nbytes[q] != t.max_bytes) return fail(-EINVAL, "query %u has %u bytes, table codes have %d", q, q_nbytes[q], t.max_bytes);
        return 0;
    }
    if (!q_nbytes) return fail(-EINVAL, "q_nbytes is required for NPHD tables");
    for (uint32_t q = 0; q < nq; ++q)
        if (q_nbytes[q] < 1 || q_nbytes[q] > t.max_bytes) return fail(-EINVAL, "query %u length %u outside 1..%d bytes", q, q_nbytes[q], t.max_bytes);
    return 0;
}

// isccsearch_join_within: one launch of the self-join kernel (join.hip.h)
template <int W>
void launch_join(const isk::JoinParams& jp, bool mask, uint64_t blocks, hipStream_t stream) {
    if (mask) hipLaunchKernelGGL((isk::join_scan_kernel<W, true>), dim3((uint32_t)blocks), dim3(isk::BLOCK), 0, stream, jp);
    else hipLaunchKernelGGL((isk::join_scan_kernel<W, false>), dim3((uint32_t)blocks), dim3(isk::BLOCK), 0, stream, jp);
}
constexpr uint32_t join_rows_per_block(uint32_t W) {
    return W == 1 ? isk::join_rows_per_block<1>() : W == 2 ? isk::join_rows_per_block<2>() : W == 3 ? isk::join_rows_per_block<3>() : isk::join_rows_per_block<4>();
}

}  // namespace

// ==========================================================================================
// C-ABI
// ==========================================================================================
extern "C" {

const char* isccsearch_last_error(void) { return g_last_error.c_str(); }

int isccsearch_create(int device_id, isccsearch_handle** out) {
    if (!out) return fail(-EINVAL, "out is NULL");
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) return fail(-ENODEV, "no HIP device available (%s)", e == hipSuccess ? "device count is 0" : hipGetErrorString(e));
    if (device_id < 0 || device_id >= ndev) return fail(-ENODEV, "device %d out of range (0..%d)", device_id, ndev - 1);
    HIPOK(hipSetDevice(device_id));
    hipDeviceProp_t prop;
    HIPOK(hipGetDeviceProperties(&prop, device_id));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(-ENODEV, "device %d is %s; this library is built for gfx950 (MI355X) only", device_id, prop.gcnArchName);
    std::unique_ptr<isccsearch_handle> h(new isccsearch_handle());
    h->device = device_id;
    h->cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    HIPOK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    HIPOK(hipEventCreateWithFlags(&h->ev_done, hipEventDisableTiming));
    HIPOK(hipEventCreateWithFlags(&h->ev_staged, hipEventDisableTiming));
    HIPOK(hipEventCreateWithFlags(&h->ev_producer, hipEventDisableTiming));
    std::vector<uint16_t> rank;
    build_rank_table(rank);
    HIPOK(hipMalloc((void**)&h->d_rank, rank.size() * sizeof(uint16_t)));
    HIPOK(hipMemcpy(h->d_rank, rank.data(), rank.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
    // the select kernel may need more than the default dynamic LDS for k near ISCCSEARCH_MAX_K
    HIPOK(hipFuncSetAttribute(reinterpret_cast<const void*>(&isk::select_kernel<1>), hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024));
    HIPOK(hipFuncSetAttribute(reinterpret_cast<const void*>(&isk::select_kernel<2>), hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024));
    HIPOK(hipFuncSetAttribute(reinterpret_cast<const void*>(&isk::select_kernel<1, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024));
    HIPOK(hipFuncSetAttribute(reinterpret_cast<const void*>(&isk::select_kernel<2, true>), hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024));
    h->stats.queries_per_pass = h->tq;
    h->stats.compute_units = h->cus;
    *out = h.release();
    return 0;
}

void* isccsearch_stream(isccsearch_handle* h) { return h ? static_cast<void*>(h->stream) : nullptr; }

int isccsearch_destroy(isccsearch_handle* h) {
    if (!h) return 0;
    {
        std::lock_guard<std::mutex> lk(h->mu);
        (void)hipSetDevice(h->device);
        if (h->stream) (void)hipStreamSynchronize(h->stream);
        for (auto& t : h->tables)
            if (t) for (auto& s : t->seg) seg_free(s);
        h->tables.clear();
        h->d_queries.release(); h->d_bias.release(); h->d_thr.release(); h->d_cnt.release(); h->d_ghist.release(); h->d_freq.release();
        h->d_overflow.release(); h->d_listcnt.release(); h->d_outcnt.release(); h->d_cand.release();
        h->d_lists.release(); h->d_final.release(); h->d_misc.release(); h->d_misc2.release();
        h->p_queries.release(); h->p_flags.release();
        h->d_block.release(); h->p_block.release();
        h->d_sp_rec.release(); h->d_sp_rows.release(); h->d_sp_nbest.release(); h->d_sp_offs.release(); h->d_sp_freqq.release();
        h->d_sp_unknown.release(); h->d_sp_matches.release(); h->d_sp_nassets.release(); h->d_sp_best.release(); h->d_sp_temp.release();
        h->d_sp_cnt.release(); h->d_sp_dofg.release();
        for (int i = 0; i < 2; ++i) { h->d_sp_entry[i].release(); h->d_sp_order[i].release(); h->d_sp_asset[i].release(); h->d_sp_score[i].release(); }
        h->d_sp_tab.release(); h->p_sp_tab.release(); h->p_sp_out.release(); h->d_sp_ws.release(); h->d_sp_idfq.release();
        for (int i = 0; i < 2; ++i) { h->d_spm_req[i].release(); h->d_spm_idx[i].release(); }
        h->d_spm_qbeg.release(); h->d_spm_nassets.release(); h->d_spm_astart.release(); h->d_spm_estart.release();
        h->d_spm_cnt.release(); h->d_spm_cpos.release();
        h->d_am_rec.release(); h->d_am_rec2.release(); h->d_am_cnt.release(); h->d_am_cnt2.release(); h->d_am_off.release();
        h->d_am_slots.release(); h->d_am_ex.release(); h->d_am_hasex.release(); h->d_am_tab.release(); h->d_am_scratch.release();
        h->p_am_out.release();
        h->d_join_keys.release(); h->d_join_total.release(); h->d_join_ham.release(); h->d_join_pb.release(); h->d_join_emit.release();
        if (h->d_rank) (void)hipFree(h->d_rank);
        for (auto& ev : h->ev_pool) { (void)hipEventDestroy(ev.first); (void)hipEventDestroy(ev.second); }
        for (hipEvent_t e : {h->ev_done, h->ev_staged, h->ev_producer}) if (e) (void)hipEventDestroy(e);
        if (h->stream) (void)hipStreamDestroy(h->stream);
    }
    delete h;
    return 0;
}

int isccsearch_set_option(isccsearch_handle* h, const char* name, int64_t value) {
    if (!h || !name) return fail(-EINVAL, "bad arguments");
    std::lock_guard<std::mutex> lk(h->mu);
    if (!strcmp(name, "queries_per_pass")) {
        // 32 is not offered: its query registers spill to scratch, which the asm-issued loads forbid
        if (value != 8 && value != 16) return fail(-EINVAL, "queries_per_pass must be 8 or 16");
        h->tq = (int)value;
        h->stats.queries_per_pass = (uint32_t)value;
        return 0;
    }
    if (!strcmp(name, "profile")) { h->profile = value != 0; return 0; }
    if (!strcmp(name, "count_candidates")) { h->count_candidates = value != 0; return 0; }
    if (!strcmp(name, "nontemporal")) {
        // only the non-temporal variant of the scan kernels is built (plain loads measured no faster):
        // asking for the other one is refused rather than silently ignored
        if (value == 0) return fail(-EINVAL, "nontemporal=0 is not available: the scan kernels are built with non-temporal loads only");
        return 0;
    }
    if (!strcmp(name, "fold")) { h->fold_tau = value ? 11 : 0; return 0; }   // shorthand kept from the experiments
    if (!strcmp(name, "blocks_per_cu")) { if (value < 1 || value > 64) return fail(-EINVAL, "blocks_per_cu must be 1..64"); h->blocks_per_cu = (uint32_t)value; return 0; }
    if (!strcmp(name, "boot_rows")) { if (value < 256 || value > 65536) return fail(-EINVAL, "boot_rows must be 256..65536"); h->boot_rows = (uint64_t)value; return 0; }
    if (!strcmp(name, "mfma_stretch_factor")) { if (value < 1 || value > 64) return fail(-EINVAL, "mfma_stretch_factor must be 1..64"); h->mfma_stretch_factor = (uint64_t)value; return 0; }
    if (!strcmp(name, "stretch_mb")) { if (value < 0 || value > 65536) return fail(-EINVAL, "stretch_mb must be 0..65536"); h->stretch_bytes = (uint64_t)value << 20; return 0; }
    if (!strcmp(name, "repick")) { h->repick = value != 0; return 0; }
    if (!strcmp(name, "fold_tau")) { if (value < 0 || value > 32) return fail(-EINVAL, "fold_tau must be 0..32"); h->fold_tau = (uint32_t)value; return 0; }
    if (!strcmp(name, "level_growth")) { if (value < 2 || value > 1024) return fail(-EINVAL, "level_growth must be 2..1024"); h->level_growth = (uint64_t)value; return 0; }
    if (!strcmp(name, "mfma")) { h->mfma = value != 0; return 0; }
    if (!strcmp(name, "device_search_hint")) { if (value < -1 || value > 8 * ISCCSEARCH_MAX_BYTES) return fail(-EINVAL, "device_search_hint must be -1..256"); h->device_search_hint = (int)value; return 0; }
    if (!strcmp(name, "self_hint")) { h->self_hint = value != 0; return 0; }
    if (!strcmp(name, "mfma_few_rows")) { if (value < 0) return fail(-EINVAL, "mfma_few_rows must be >= 0"); h->mfma_few_rows = (uint64_t)value; return 0; }
    if (!strcmp(name, "mfma_pack_min_queries")) { if (value < 1 || value > 1024) return fail(-EINVAL, "mfma_pack_min_queries must be 1..1024"); h->mfma_pack_min_queries = (uint32_t)value; return 0; }
    if (!strcmp(name, "mfma_min_queries")) { if (value < 1 || value > 1024) return fail(-EINVAL, "mfma_min_queries must be 1..1024"); h->mfma_min_queries = (uint32_t)value; return 0; }
    if (!strcmp(name, "self_tighten")) { h->self_tighten = value != 0; return 0; }
    if (!strcmp(name, "boot_multi")) { h->boot_multi = value != 0; return 0; }
    if (!strcmp(name, "self_refresh_steps")) {
        if (value < 1 || value > 64 || (value & (value - 1))) return fail(-EINVAL, "self_refresh_steps must be a power of two in 1..64");
        h->self_refresh_steps = (uint32_t)value; return 0;
    }
    if (!strcmp(name, "candidate_cap")) { if (value < 64 || value > (1 << 22)) return fail(-EINVAL, "candidate_cap must be 64..4194304"); h->candidate_cap = (uint32_t)value; return 0; }
    if (!strcmp(name, "self_max_k")) { if (value < 1 || value > ISCCSEARCH_MAX_K) return fail(-EINVAL, "self_max_k must be 1..%d", ISCCSEARCH_MAX_K); h->self_max_k = (uint32_t)value; return 0; }
    if (!strcmp(name, "self_boot_rows")) { if (value < 256 || value > (1 << 20)) return fail(-EINVAL, "self_boot_rows must be 256..1048576"); h->self_boot_rows = (uint64_t)value; return 0; }
    if (!strcmp(name, "mfma_level_growth")) { if (value < 2 || value > 1024) return fail(-EINVAL, "mfma_level_growth must be 2..1024"); h->mfma_level_growth = (uint64_t)value; return 0; }
    if (!strcmp(name, "mfma_pack")) { h->mfma_pack = value != 0; return 0; }
    if (!strcmp(name, "mfma_pack3")) { h->mfma_pack3 = value != 0; return 0; }
    if (!strcmp(name, "tiny_rows")) { if (value < 0 || value > (1 << 20)) return fail(-EINVAL, "tiny_rows must be 0..1048576"); h->tiny_rows = (uint32_t)value; return 0; }
    if (!strcmp(name, "select_wide_from")) { if (value < 0) return fail(-EINVAL, "select_wide_from must be >= 0"); h->select_wide_from = (uint32_t)std::min<int64_t>(value, 0xFFFFFFFFll); return 0; }
    if (!strcmp(name, "speculate")) { h->speculate = value != 0; return 0; }
    if (!strcmp(name, "spec_max_queries")) { if (value < 0 || value > 1024) return fail(-EINVAL, "spec_max_queries must be 0..1024"); h->spec_max_queries = (uint32_t)value; return 0; }
    if (!strcmp(name, "self_boot_per_k")) { if (value < 0 || value > (1 << 20)) return fail(-EINVAL, "self_boot_per_k must be 0..2^20"); h->self_boot_per_k = (uint32_t)value; return 0; }
    if (!strcmp(name, "mfma_min_rows")) { if (value < 1) return fail(-EINVAL, "mfma_min_rows must be >= 1"); h->mfma_min_rows = (uint64_t)value; return 0; }
    if (!strcmp(name, "sample_cost")) return 0;   // accepted for compatibility: the levels no longer re-read rows, nothing to balance
    return fail(-EINVAL, "unknown option '%s'", name);
}

int isccsearch_stats_get(isccsearch_handle* h, isccsearch_stats* out, int reset) {
    if (!h || !out) return fail(-EINVAL, "bad arguments");
    std::lock_guard<std::mutex> lk(h->mu);
    HIPOK(hipSetDevice(h->device));
    int rc = drain_events(h);
    if (rc) return rc;
    *out = h->stats;
    if (reset) {
        const uint32_t tq = h->stats.queries_per_pass, cu = h->stats.compute_units;
        h->stats = isccsearch_stats{};
        h->stats.queries_per_pass = tq;
        h->stats.compute_units = cu;
    }
    return 0;
}

int isccsearch_table_open(isccsearch_handle* h, int metric, int key_words, int max_bytes, uint32_t* table_id) {
    if (!h || !table_id) return fail(-EINVAL, "bad arguments");
    if (metric != ISCCSEARCH_METRIC_HAMMING && metric != ISCCSEARCH_METRIC_NPHD) return fail(-EINVAL, "unknown metric %d", metric);
    if (key_words != 1 && key_words != 2) return fail(-EINVAL, "key_words must be 1 or 2");
    if (max_bytes < 1 || max_bytes > ISCCSEARCH_MAX_BYTES) return fail(-EINVAL, "max_bytes must be 1..%d", ISCCSEARCH_MAX_BYTES);
    std::lock_guard<std::mutex> lk(h->mu);
    std::unique_ptr<Table> t(new Table());
    t->open = true;
    t->metric = metric;
    t->key_words = key_words;
    t->max_bytes = max_bytes;
    t->max_words = (max_bytes + 7) / 8;
    for (uint32_t b = 1; b <= ISCCSEARCH_MAX_BYTES; ++b) { t->seg[b].nbytes = b; t->seg[b].W = (b + 7) / 8; }
    for (size_t i = 0; i < h->tables.size(); ++i)
        if (!h->tables[i]) { h->tables[i] = std::move(t); *table_id = (uint32_t)i; return 0; }
    h->tables.push_back(std::move(t));
    *table_id = (uint32_t)(h->tables.size() - 1);
    return 0;
}

int isccsearch_table_drop(isccsearch_handle* h, uint32_t table) {
    if (!h) return fail(-EINVAL, "handle is NULL");
    std::lock_guard<std::mutex> lk(h->mu);
    Table* t;
    int rc = get_table(h, table, t);
    if (rc) return rc;
    HIPOK(hipSetDevice(h->device));
    HIPOK(hipStreamSynchronize(h->stream));
    for (auto& s : t->seg) seg_free(s);
    h->tables[table].reset();
    return 0;
}

int isccsearch_reserve(isccsearch_handle* h, uint32_t table, int nbytes, uint64_t rows) {
    if (!h) return fail(-EINVAL, "handle is NULL");
    std::lock_guard<std::mutex> lk(h->mu);
    Table* t;
    int rc = get_table(h, table, t);
    if (rc) return rc;
    if (nbytes < 1 || nbytes > t->max_bytes) return fail(-EINVAL, "nbytes %d outside 1..%d", nbytes, t->max_bytes);
    if (t->metric == ISCCSEARCH_METRIC_HAMMING && nbytes != t->max_bytes) return fail(-EINVAL, "Hamming tables hold %d-byte codes only", t->max_bytes);
    HIPOK(hipSetDevice(h->device));
    return seg_reserve(h, *t, t->seg[nbytes], rows);
}

uint64_t isccsearch_size(isccsearch_handle* h, uint32_t table) {
    if (!h) return 0;
    std::lock_guard<std::mutex> lk(h->mu);
    Table* t;
    if (get_table(h, table, t)) return 0;
    return t->total;
}

int isccsearch_add(isccsearch_handle* h, uint32_t table, uint64_t n, const uint64_t* keys,
                   const uint64_t* code_words, const uint8_t* nbytes, uint32_t flags) {
    if (!h) return fail(-EINVAL, "handle is NULL");
    if (n == 0) return 0;
    if (!keys || !code_words) return fail(-EINVAL, "keys/code_words are NULL");
    std::lock_guard<std::mutex> lk(h->mu);
    Table* tp;
    int rc = get_table(h, table, tp);
    if (rc) return rc;
    Table& t = *tp;
    HIPOK(hipSetDevice(h->device));
    const int KW = t.key_words, MW = t.max_words;
    if (t.metric == ISCCSEARCH_METRIC_NPHD && !nbytes) return fail(-EINVAL, "nbytes is required for NPHD tables");
    // validate lengths, count rows per segment
    uint64_t per_seg[ISCCSEARCH_MAX_BYTES + 1] = {0};
    for (uint64_t i = 0; i < n; ++i) {
        const uint32_t b = nbytes ? nbytes[i] : (uint32_t)t.max_bytes;
        if (b < 1 || b > (uint32_t)t.max_bytes) return fail(-EINVAL, "row %llu: code length %u outside 1..%d bytes", (unsigned long long)i, b, t.max_bytes);
        if (t.metric == ISCCSEARCH_METRIC_HAMMING && b != (uint32_t)t.max_bytes) return fail(-EINVAL, "row %llu: Hamming table holds %d-byte codes, got %u", (unsigned long long)i, t.max_bytes, b);
        per_seg[b]++;
    }
    const bool trusted = (flags & ISCCSEARCH_ADD_TRUSTED_UNIQUE) != 0;
    if (!trusted) {
        if ((rc = ensure_index(h, t))) return rc;
        std::unordered_map<Key, int, KeyHash> seen;
        seen.reserve((size_t)n);
        for (uint64_t i = 0; i < n; ++i) {
            Key k = KW == 2 ? Key{keys[2 * i], keys[2 * i + 1]} : Key{0, keys[i]};
            if (t.index.contains(k) || !seen.emplace(k, 1).second)
                return fail(-EEXIST, "key %016llx%016llx already present (row %llu of the batch)", (unsigned long long)k.hi, (unsigned long long)k.lo, (unsigned long long)i);
        }
    }
    // grow segments
    for (uint32_t b = 1; b <= ISCCSEARCH_MAX_BYTES; ++b)
        if (per_seg[b] && (rc = seg_reserve(h, t, t.seg[b], t.seg[b].n + per_seg[b]))) return rc;
    // stage per segment (word-major) and copy
    std::vector<uint64_t> stage, kstage;
    for (uint32_t b = 1; b <= ISCCSEARCH_MAX_BYTES; ++b) {
        const uint64_t m = per_seg[b];
        if (!m) continue;
        Segment& s = t.seg[b];
        const bool direct = (m == n && MW == 1);   // single segment, one word: the caller's buffers are already column-shaped
        const uint64_t* kp = keys;
        if (direct) {
            HIPOK(hipMemcpyAsync(s.col[0] + s.n, code_words, m * 8, hipMemcpyHostToDevice, h->stream));
        } else if (m == n) {
            // one code length, several words: ship the caller's row-major block as it is and split it into the
            // word columns on the device (a host-side transposition capped 256-bit ingest at 80 M rows/s)
            if ((rc = h->d_misc2.ensure((size_t)n * MW))) return rc;
            HIPOK(hipMemcpyAsync(h->d_misc2.p, code_words, (size_t)n * MW * 8, hipMemcpyHostToDevice, h->stream));
            isk::SplitParams sp{};
            for (uint32_t w = 0; w < s.W; ++w) sp.col[w] = s.col[w];
            sp.rows = h->d_misc2.p; sp.dst_row = s.n; sp.n = n; sp.W = s.W; sp.MW = (uint32_t)MW; sp.mask_last = mask_for(b);
            const uint32_t grid = (uint32_t)std::min<uint64_t>((n + isk::BLOCK - 1) / isk::BLOCK, (uint64_t)h->cus * 8);
            hipLaunchKernelGGL(isk::split_rows_kernel, dim3(grid), dim3(isk::BLOCK), 0, h->stream, sp);
            HIPOK(hipGetLastError());
        } else {
            stage.resize((size_t)m * s.W);
            uint64_t j = 0;
            const uint64_t lastmask = mask_for(b);
            for (uint64_t i = 0; i < n; ++i) {
                const uint32_t bi = nbytes ? nbytes[i] : (uint32_t)t.max_bytes;
                if (bi != b) continue;
                for (uint32_t w = 0; w < s.W; ++w) {
                    uint64_t v = code_words[i * MW + w];
                    if (w == s.W - 1) v &= lastmask;
                    stage[(size_t)w * m + j] = v;
                }
                ++j;
            }
            for (uint32_t w = 0; w < s.W; ++w)
                HIPOK(hipMemcpyAsync(s.col[w] + s.n, stage.data() + (size_t)w * m, m * 8, hipMemcpyHostToDevice, h->stream));
        }
        if (m != n) {
            kstage.resize((size_t)m * KW);
            uint64_t j = 0;
            for (uint64_t i = 0; i < n; ++i) {
                const uint32_t bi = nbytes ? nbytes[i] : (uint32_t)t.max_bytes;
                if (bi != b) continue;
                for (int w = 0; w < KW; ++w) kstage[(size_t)j * KW + w] = keys[i * KW + w];
                ++j;
            }
            kp = kstage.data();
        }
        HIPOK(hipMemcpyAsync(s.keys + s.n * KW, kp, m * 8 * KW, hipMemcpyHostToDevice, h->stream));
        HIPOK(hipStreamSynchronize(h->stream));
        if (t.indexed) {
            s.hkeys.insert(s.hkeys.end(), kp, kp + m * KW);
            for (uint64_t r = 0; r < m; ++r) {
                Key k = KW == 2 ? Key{kp[2 * r], kp[2 * r + 1]} : Key{0, kp[r]};
                t.index.set(k, Loc{b, s.n + r});
            }
        }
        s.n += m;
        s.touch();
        t.total += m;
    }
    return 0;
}

int isccsearch_segments(isccsearch_handle* h, uint32_t table, uint64_t* out_rows) {
    if (!h || !out_rows) return fail(-EINVAL, "bad arguments");
    std::lock_guard<std::mutex> lk(h->mu);
    Table* tp;
    int rc = get_table(h, table, tp);
    if (rc) return rc;
    out_rows[0] = 0;
    for (uint32_t b = 1; b <= ISCCSEARCH_MAX_BYTES; ++b) out_rows[b] = tp->seg[b].n;
    return 0;
}

int isccsearch_export(isccsearch_handle* h, uint32_t table, int nbytes, uint64_t first_row, uint64_t n,
                      uint64_t* out_keys, uint64_t* out_cols) {
    if (!h) return fail(-EINVAL, "handle is NULL");
    if (n == 0) return 0;
    if (!out_keys || !out_cols) return fail(-EINVAL, "NULL argument");
    std::lock_guard<std::mutex> lk(h->mu);
    Table* tp;
    int rc = get_table(h, table, tp);
    if (rc) return rc;
    if (nbytes < 1 || nbytes > tp->max_bytes) return fail(-EINVAL, "nbytes %d outside 1..%d", nbytes, tp->max_bytes);
    Segment& s = tp->seg[nbytes];
    if (first_row > s.n || n > s.n - first_row) return fail(-EINVAL, "rows [%llu, +%llu) outside the segment's %llu rows", (unsigned long long)first_row, (unsigned long long)n, (unsigned long long)s.n);
    HIPOK(hipSetDevice(h->device));
    for (uint32_t w = 0; w < s.W; ++w)
        HIPOK(hipMemcpyAsync(out_cols + (size_t)w * n, s.col[w] + first_row, n * 8, hipMemcpyDeviceToHost, h->stream));
    HIPOK(hipMemcpyAsync(out_keys, s.keys + first_row * tp->key_words, n * 8 * tp->key_words, hipMemcpyDeviceToHost, h->stream));
    HIPOK(hipStreamSynchronize(h->stream));
    return 0;
}

int isccsearch_add_columns(isccsearch_handle* h, uint32_t table, int nbytes, uint64_t n, const uint64_t* keys,
                           const uint64_t* cols, uint32_t flags) {
    if (!h) return fail(-EINVAL, "handle is NULL");
    if (n == 0) return 0;
    if (!keys || !cols) return fail(-EINVAL, "keys/cols are NULL");
    std::lock_guard<std::mutex> lk(h->mu);
    Table* tp;
    int rc = get_table(h, table, tp);
    if (rc) return rc;
    Table& t = *tp;
    if (nbytes < 1 || nbytes > t.max_bytes) return fail(-EINVAL, "nbytes %d outside 1..%d", nbytes, t.max_bytes);
    if (t.metric == ISCCSEARCH_METRIC_HAMMING && nbytes != t.max_bytes) return fail(-EINVAL, "Hamming tables hold %d-byte codes only", t.max_bytes);
    HIPOK(hipSetDevice(h->device));
    const int KW = t.key_words;
    const bool trusted = (flags & ISCCSEARCH_ADD_TRUSTED_UNIQUE) != 0;
    if (!trusted) {
        if ((rc = ensure_index(h, t))) return rc;
        std::unordered_map<Key, int, KeyHash> seen;
        seen.reserve((size_t)n);
        for (uint64_t i = 0; i < n; ++i) {
            Key k = KW == 2 ? Key{keys[2 * i], keys[2 * i + 1]} : Key{0, keys[i]};
            if (t.index.contains(k) || !seen.emplace(k, 1).second)
                return fail(-EEXIST, "key %016llx%016llx already present (row %llu of the batch)", (unsigned long long)k.hi, (unsigned long long)k.lo, (unsigned long long)i);
        }
    }
    Segment& s = t.seg[nbytes];
    if ((rc = seg_reserve(h, t, s, s.n + n))) return rc;
    for (uint32_t w = 0; w < s.W; ++w)
        HIPOK(hipMemcpyAsync(s.col[w] + s.n, cols + (size_t)w * n, n * 8, hipMemcpyHostToDevice, h->stream));
    HIPOK(hipMemcpyAsync(s.keys + s.n * KW, keys, n * 8 * KW, hipMemcpyHostToDevice, h->stream));
    HIPOK(hipStreamSynchronize(h->stream));
    if (t.indexed) {
        s.hkeys.insert(s.hkeys.end(), keys, keys + n * KW);
        for (uint64_t r = 0; r < n; ++r) {
            Key k = KW == 2 ? Key{keys[2 * r], keys[2 * r + 1]} : Key{0, keys[r]};
            t.index.set(k, Loc{(uint32_t)nbytes, s.n + r});
        }
    }
    s.n += n;
    s.touch();
    t.total += n;
    return 0;
}

int isccsearch_add_synthetic(isccsearch_handle* h, uint32_t table, int nbytes, uint64_t n,
                             uint64_t seed, uint64_t first_row, uint64_t key_base) {
    if (!h) return fail(-EINVAL, "handle is NULL");
    if (n == 0) return 0;
    std::lock_guard<std::mutex> lk(h->mu);
    Table* tp;
    int rc = get_table(h, table, tp);
    if (rc) return rc;
    Table& t = *tp;
    if (nbytes < 1 || nbytes > t.max_bytes) return fail(-EINVAL, "nbytes %d outside 1..%d", nbytes, t.max_bytes);
    if (t.metric == ISCCSEARCH_METRIC_HAMMING && nbytes != t.max_bytes) return fail(-EINVAL, "Hamming tables hold %d-byte codes only", t.max_bytes);
    if (t.indexed) return fail(-EINVAL, "synthetic rows cannot be added to a table whose key index is built");
    HIPOK(hipSetDevice(h->device));
    Segment& s = t.seg[nbytes];
    if ((rc = seg_reserve(h, t, s, s.n + n))) return rc;
    isk::FillParams fp{};
    for (uint32_t w = 0; w < s.W; ++w) fp.col[w] = s.col[w];
    fp.keys = s.keys; fp.dst_row = s.n; fp.n = n; fp.seed = seed; fp.first_row = first_row; fp.key_base = key_base;
    fp.W = s.W; fp.KW = (uint32_t)t.key_words; fp.mask_last = mask_for((uint32_t)nbytes);
    const uint32_t grid = (uint32_t)std::min<uint64_t>((n + isk::BLOCK - 1) / isk::BLOCK, (uint64_t)h->cus * 16);
    hipLaunchKernelGGL(isk::fill_kernel, dim3(grid), dim3(isk::BLOCK), 0, h->stream, fp);
    HIPOK(hipGetLastError());
    HIPOK(hipStreamSynchronize(h->stream));
    s.n += n;
    s.touch();
    t.total += n;
    return 0;
}

int isccsearch_remove(isccsearch_handle* h, uint32_t table, uint64_t n, const uint64_t* keys, uint64_t* n_removed) {
    if (!h) return fail(-EINVAL, "handle is NULL");
    if (n_removed) *n_removed = 0;
    if (n == 0) return 0;
    if (!keys) return fail(-EINVAL, "keys is NULL");
    std::lock_guard<std::mutex> lk(h->mu);
    Table* tp;
    int rc = get_table(h, table, tp);
    if (rc) return rc;
    Table& t = *tp;
    HIPOK(hipSetDevice(h->device));
    if ((rc = ensure_index(h, t))) return rc;
    const int KW = t.key_words;
    // the host index is updated key by key below and the row moves are replayed on the device afterwards: reserve what that
    // replay needs BEFORE anything changes, so that an allocation failure cannot leave host and device rows disagreeing
    if ((rc = h->d_misc.ensure((size_t)n * 2))) return rc;
    std::vector<uint64_t> moves[ISCCSEARCH_MAX_BYTES + 1];
    uint64_t removed = 0;
    for (uint64_t i = 0; i < n; ++i) {
        Key k = KW == 2 ? Key{keys[2 * i], keys[2 * i + 1]} : Key{0, keys[i]};
        Loc loc;
        if (!t.index.find(k, loc)) continue;
        Segment& s = t.seg[loc.seg];
        const uint64_t last = s.n - 1;
        t.index.erase(k);
        if (loc.row != last) {
            Key lk2 = KW == 2 ? Key{s.hkeys[2 * last], s.hkeys[2 * last + 1]} : Key{0, s.hkeys[last]};
            for (int w = 0; w < KW; ++w) s.hkeys[loc.row * KW + w] = s.hkeys[last * KW + w];
            t.index.set(lk2, Loc{loc.seg, loc.row});
            moves[loc.seg].push_back(loc.row);
            moves[loc.seg].push_back(last);
        }
        s.hkeys.resize((size_t)last * KW);
        s.n = last;
        s.touch();
        t.total--;
        ++removed;
    }
    for (uint32_t b = 1; b <= ISCCSEARCH_MAX_BYTES; ++b) {
        if (moves[b].empty()) continue;
        Segment& s = t.seg[b];
        if ((rc = h->d_misc.ensure(moves[b].size()))) return rc;
        HIPOK(hipMemcpyAsync(h->d_misc.p, moves[b].data(), moves[b].size() * 8, hipMemcpyHostToDevice, h->stream));
        isk::MoveParams mp{};
        for (uint32_t w = 0; w < s.W; ++w) mp.col[w] = s.col[w];
        mp.keys = s.keys; mp.moves = h->d_misc.p; mp.n_moves = moves[b].size() / 2; mp.W = s.W; mp.KW = (uint32_t)KW;
        hipLaunchKernelGGL(isk::move_rows_kernel, dim3(1), dim3(64), 0, h->stream, mp);
        HIPOK(hipGetLastError());
        HIPOK(hipStreamSynchronize(h->stream));
    }
    if (n_removed) *n_removed = removed;
    return 0;
}

int isccsearch_contains(isccsearch_handle* h, uint32_t table, uint64_t n, const uint64_t* keys, uint8_t* out_found) {
    if (!h) return fail(-EINVAL, "handle is NULL");
    if (n == 0) return 0;
    if (!keys || !out_found) return fail(-EINVAL, "keys/out_found are NULL");
    std::lock_guard<std::mutex> lk(h->mu);
    Table* tp;
    int rc = get_table(h, table, tp);
    if (rc) return rc;
    HIPOK(hipSetDevice(h->device));
    if ((rc = ensure_index(h, *tp))) return rc;
    const int KW = tp->key_words;
    for (uint64_t i = 0; i < n; ++i) {
        Key k = KW == 2 ? Key{keys[2 * i], keys[2 * i + 1]} : Key{0, keys[i]};
        out_found[i] = tp->index.contains(k) ? 1 : 0;
    }
    return 0;
}

int isccsearch_get(isccsearch_handle* h, uint32_t table, uint64_t n, const uint64_t* keys,
                   uint64_t* out_words, uint8_t* out_nbytes) {
    if (!h) return fail(-EINVAL, "handle is NULL");
    if (n == 0) return 0;
    if (!keys || !out_words || !out_nbytes) return fail(-EINVAL, "NULL argument");
    std::lock_guard<std::mutex> lk(h->mu);
    Table* tp;
    int rc = get_table(h, table, tp);
    if (rc) return rc;
    Table& t = *tp;
    HIPOK(hipSetDevice(h->device));
    if ((rc = ensure_index(h, t))) return rc;
    const int KW = t.key_words, MW = t.max_words;
    memset(out_words, 0, (size_t)n * MW * 8);
    memset(out_nbytes, 0, (size_t)n);
    std::vector<uint64_t> rows[ISCCSEARCH_MAX_BYTES + 1], dest[ISCCSEARCH_MAX_BYTES + 1];
    for (uint64_t i = 0; i < n; ++i) {
        Key k = KW == 2 ? Key{keys[2 * i], keys[2 * i + 1]} : Key{0, keys[i]};
        Loc loc;
        if (!t.index.find(k, loc)) continue;
        rows[loc.seg].push_back(loc.row);
        dest[loc.seg].push_back(i);
        out_nbytes[i] = (uint8_t)loc.seg;
    }
    std::vector<uint64_t> tmp;
    for (uint32_t b = 1; b <= ISCCSEARCH_MAX_BYTES; ++b) {
        if (rows[b].empty()) continue;
        Segment& s = t.seg[b];
        const uint64_t m = rows[b].size();
        if ((rc = h->d_misc.ensure(m))) return rc;
        if ((rc = h->d_misc2.ensure(m * s.W))) return rc;
        HIPOK(hipMemcpyAsync(h->d_misc.p, rows[b].data(), m * 8, hipMemcpyHostToDevice, h->stream));
        isk::GatherParams gp{};
        for (uint32_t w = 0; w < s.W; ++w) gp.col[w] = s.col[w];
        gp.rows = h->d_misc.p; gp.out = h->d_misc2.p; gp.n = m; gp.W = s.W;
        const uint32_t grid = (uint32_t)std::min<uint64_t>((m + isk::BLOCK - 1) / isk::BLOCK, 1024);
        hipLaunchKernelGGL(isk::gather_rows_kernel, dim3(grid), dim3(isk::BLOCK), 0, h->stream, gp);
        HIPOK(hipGetLastError());
        tmp.resize(m * s.W);
        HIPOK(hipMemcpyAsync(tmp.data(), h->d_misc2.p, m * s.W * 8, hipMemcpyDeviceToHost, h->stream));
        HIPOK(hipStreamSynchronize(h->stream));
        for (uint64_t i = 0; i < m; ++i)
            for (uint32_t w = 0; w < s.W; ++w) out_words[dest[b][i] * MW + w] = tmp[i * s.W + w];
    }
    return 0;
}

// freq[i] = document frequency of the code stored under keys[i] (0 when the key is absent), read from the
// segment's document-frequency column; the column is (re)built here when rows changed since it was made.
int isccsearch_get_freq(isccsearch_handle* h, uint32_t table, uint64_t n, const uint64_t* keys,
                        uint32_t dup_limit, uint32_t* out_freq) {
    if (!h) return fail(-EINVAL, "handle is NULL");
    if (dup_limit < 1) return fail(-EINVAL, "dup_limit must be >= 1");
    if (n == 0) return 0;
    if (!keys || !out_freq) return fail(-EINVAL, "NULL argument");
    std::lock_guard<std::mutex> lk(h->mu);
    Table* tp;
    int rc = get_table(h, table, tp);
    if (rc) return rc;
    Table& t = *tp;
    if (t.metric != ISCCSEARCH_METRIC_HAMMING) return fail(-EINVAL, "get_freq is defined for fixed-length (Hamming) tables");
    HIPOK(hipSetDevice(h->device));
    if ((rc = ensure_index(h, t))) return rc;
    const int KW = t.key_words;
    memset(out_freq, 0, (size_t)n * sizeof(uint32_t));
    std::vector<uint64_t> rows[ISCCSEARCH_MAX_BYTES + 1], dest[ISCCSEARCH_MAX_BYTES + 1];
    for (uint64_t i = 0; i < n; ++i) {
        Key k = KW == 2 ? Key{keys[2 * i], keys[2 * i + 1]} : Key{0, keys[i]};
        Loc loc;
        if (!t.index.find(k, loc)) continue;
        rows[loc.seg].push_back(loc.row);
        dest[loc.seg].push_back(i);
    }
    std::vector<uint32_t> tmp;
    for (uint32_t b = 1; b <= ISCCSEARCH_MAX_BYTES; ++b) {
        if (rows[b].empty()) continue;
        Segment& s = t.seg[b];
        if ((rc = ensure_freq_column(h, t, s, dup_limit))) return rc;
        const uint64_t m = rows[b].size();
        if ((rc = h->d_misc.ensure(m))) return rc;
        if ((rc = h->d_freq.ensure(m))) return rc;
        HIPOK(hipMemcpyAsync(h->d_misc.p, rows[b].data(), m * 8, hipMemcpyHostToDevice, h->stream));
        const uint32_t grid = (uint32_t)std::min<uint64_t>((m + isk::BLOCK - 1) / isk::BLOCK, 1024);
        hipLaunchKernelGGL(isk::gather_u32_kernel, dim3(grid), dim3(isk::BLOCK), 0, h->stream, s.freq, h->d_misc.p, h->d_freq.p, m);
        HIPOK(hipGetLastError());
        tmp.resize(m);
        HIPOK(hipMemcpyAsync(tmp.data(), h->d_freq.p, m * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
        HIPOK(hipStreamSynchronize(h->stream));
        for (uint64_t i = 0; i < m; ++i) out_freq[dest[b][i]] = tmp[i];
    }
    return 0;
}

static_assert(isksp::MAX_QUERY_SIMPRINTS == ISCCSEARCH_MAX_SCORED_SIMPRINTS, "header and kernels disagree");
// isccsearch_simprint_score: where a search leaves its lists for the scoring kernels instead of handing them to the host
struct ScoreSink {
    isksp::Buffers buf{};
    int h_max = -1;
    uint32_t dup_limit = 0;
    uint32_t entries = 0;       // best (asset, query) entries appended so far -- known after each batch's synchronisation
    uint32_t max_count = 0;     // longest neighbour list
    bool unknown_any = false;   // some query's own document frequency could not be read off its list
    bool exact = false;         // isccsearch_simprint_exact: the lists are collision lists; only their lengths are kept per batch (no marking)
    // ... and when ONE batch holds every lookup, its hits / offsets are prepared behind its select, so that the number of entries
    // arrives with the batch's own synchronisation
    const uint32_t* d_of_g = nullptr;
    uint32_t nd = 0, ng = 0;
    bool prepared = false;
    uint32_t* q_count = nullptr;    // when set: [nq] length of every query's neighbour list (capped at k)
};

// The search itself; h->mu is held by the caller.
//   radius >= 0   range-limited search (fixed threshold)
//   out_freq      when set, only the number of distinct assets per result list is returned (doc frequency)
//   sink          when set (one-segment Hamming tables), records and rows stay in the sink's device buffers, every batch is followed by
//                 the marking / compaction kernels of simprint_score.hip, and only {counts | flags | k-th distances | info} reach the host
static int search_locked(isccsearch_handle* h, uint32_t table, uint32_t nq, const uint64_t* q_words,
                         const uint8_t* q_nbytes, uint32_t k,
                         uint64_t* out_keys, uint32_t* out_hamming, uint16_t* out_prefix_bits, uint32_t* out_count,
                         int radius = -1, uint32_t* out_freq = nullptr, uint32_t* out_collisions = nullptr, ScoreSink* sink = nullptr) {
    Table* tp;
    int rc = get_table(h, table, tp);
    if (rc) return rc;
    Table& t = *tp;
    if ((rc = check_query_lengths(t, nq, q_nbytes))) return rc;
    HIPOK(hipSetDevice(h->device));
    h->stats.queries += nq;

    // group queries by byte length (NPHD prefix length differs per class)
    std::vector<uint32_t> order(nq);
    for (uint32_t q = 0; q < nq; ++q) order[q] = q;
    auto qlen = [&](uint32_t q) -> uint32_t { return (t.metric == ISCCSEARCH_METRIC_NPHD) ? q_nbytes[q] : (uint32_t)t.max_bytes; };
    if (t.metric == ISCCSEARCH_METRIC_NPHD)
        std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return q_nbytes[a] < q_nbytes[b]; });

    std::vector<uint64_t> hq;
    uint32_t pos = 0;
    while (pos < nq) {
        const uint32_t len = qlen(order[pos]);
        uint32_t end = pos;
        while (end < nq && end - pos < QB_MAX && qlen(order[end]) == len) ++end;
        const uint32_t m = end - pos;
        hq.resize((size_t)m * t.max_words);
        for (uint32_t i = 0; i < m; ++i)
            memcpy(&hq[(size_t)i * t.max_words], q_words + (size_t)order[pos + i] * t.max_words, (size_t)t.max_words * 8);
        // result block {records [m][k] | counts [m] | flags [<= m + 15]} on the device and, mirrored, in pinned memory
        const size_t rec_bytes = sink ? 0 : (size_t)m * k * sizeof(isk::Record);     // (a sink keeps the records on the device)
        const size_t flag_slots = (size_t)m + 16;                       // nq_pad <= m + 15 for every T_q
        // (+ m counts behind the flags when a document-frequency call also wants the lists' lengths;
        //  + m k-th distances and the scoring kernels' info words when the lists stay on the device)
        const size_t block_bytes = rec_bytes + ((size_t)m + flag_slots + (out_collisions || sink ? m : 0) + (sink ? isksp::INFO_WORDS : 0)) * sizeof(uint32_t);
        if ((rc = h->d_block.ensure(block_bytes))) return rc;
        if ((rc = h->p_block.ensure(block_bytes))) return rc;
        const isk::Record* const p_rec = reinterpret_cast<const isk::Record*>(h->p_block.p);
        uint32_t* const p_cnt = reinterpret_cast<uint32_t*>(h->p_block.p + rec_bytes);
        const uint32_t segments = t.segments();
        const bool one_copy = segments == 1 && !out_freq;   // flags ride in the block: results leave in ONE copy
        // ... or in none: select_kernel writes a small block straight into the pinned mirror (page-locked memory is mapped
        // into the device's address space), so the host only synchronises.  A device->host copy costs ~25 us of queue
        // hand-over after the kernel, more than the 240 bytes per query take to cross PCIe as plain stores.  Large blocks
        // (big k x many queries) keep the DMA copy.
        const bool direct = one_copy && block_bytes <= DIRECT_RESULT_BYTES && !sink;
        isk::Record* const d_rec = sink ? h->d_sp_rec.p + (size_t)pos * k : reinterpret_cast<isk::Record*>(direct ? h->p_block.p : h->d_block.p);
        uint32_t* const d_cnt = reinterpret_cast<uint32_t*>((direct ? h->p_block.p : h->d_block.p) + rec_bytes);
        uint32_t* const p_kth = p_cnt + m + flag_slots;                  // (sink) hamming of every query's last result
        Batch batch(h, t, m, len, k, d_rec, d_cnt);
        batch.radius = radius;
        if (sink) { if (!sink->exact) batch.d_out_rows = h->d_sp_rows.p + (size_t)pos * k; batch.d_out_kth = d_cnt + m + flag_slots; }
        if (one_copy) { batch.d_flags = d_cnt + m; batch.h_flags = p_cnt + m; }
        // Speculation: ONE pass under where an earlier batch of this size and query length ended, verified by one look at its
        // lists; a miss (a list overflowed, a query came up short) sends the batch through the ordinary path -- nothing is ever
        // returned unverified.
        //   radius     SMALL batches over one segment.  One query costs boot + level + pick + collect + select: five launches for
        //              what is one pass over the rows (0.22 ms against a 0.13 ms pass).  The k-th distance of similar queries over
        //              the same rows hardly moves, so the pass is first tried as a RANGE-LIMITED search under the distance the
        //              previous search of this segment ended at (+ 2): radius_init + collect + select.  It is exact whenever every
        //              query finds k rows within that radius (its k nearest are then among them).
        //   self_hint  LARGER batches over one segment keep their single self-tightening pass (one radius for hundreds of queries
        //              admits several times the candidates of per-query thresholds) but START it under the hint instead of a
        //              bootstrap sample's threshold: no sample kernel, no flood of candidates in the first steps.  Same check.
        //   ratio      SEVERAL segments (an index of mixed code lengths -- what an ISCC-UNIT index is).  The ordinary path costs
        //              boot + level + pick + collect + select per segment and two synchronisations (0.62 ms for one 256-bit query
        //              over 4 x 25 M rows); here every segment lists its rows within (hint + 1/32) x compared bits (radius_init +
        //              collect + select each), the lists are merged and ONE synchronisation brings results and flags.  The answer
        //              stands if no list overflowed, every query has k rows and its k-th NPHD is <= hint + 1/32: a row outside a
        //              segment's radius lies strictly beyond that ratio, a row inside it but not listed has k nearer rows of its own
        //              segment before it.
        enum class Spec { none, radius, self_hint, ratio } spec = Spec::none;
        // radius / self_hint: an ordinary top-k search over ONE segment that has been searched with this k before
        Segment* const spec_seg = t.sole_segment();
        // (a segment small enough for the one-launch search -- Batch::tiny -- has nothing to gain from a radius: it is exact in that launch either way)
        const bool one_launch = spec_seg && h->tiny_rows && spec_seg->n <= h->tiny_rows && spec_seg->n < h->mfma_min_rows && spec_seg->n <= h->candidate_cap;
        const bool hintable = spec_seg && radius < 0 && !out_freq && one_copy && k <= spec_seg->n && !one_launch;
        const bool small_batch = hintable && m <= h->spec_max_queries;
        if (hintable && h->speculate && !h->spec_suppress && (small_batch || h->self_hint) && spec_seg->hint(m, len).ready(k)) {
            if (small_batch) { spec = Spec::radius; batch.radius = (int)spec_seg->hint(m, len).tau; }
            else { spec = Spec::self_hint; batch.self_hint = (int)spec_seg->hint(m, len).tau; }
        }
        const bool mhintable = segments > 1 && radius < 0 && !out_freq && (m <= h->spec_max_queries || h->self_hint) && k <= t.total;
        if (mhintable && h->speculate && !h->spec_suppress && t.mhint(m, len).ready(k)) {
            spec = Spec::ratio;
            batch.radius_ratio = t.mhint(m, len).ratio + 1.0 / 32.0;      // the margin: 2 bits of 64, 8 of 256
            batch.ratio_starts_self = m > h->spec_max_queries;             // larger batches: each segment's single pass STARTS under it
        }
        auto copy_results = [&]() -> int {
            if (out_freq) {
                // only the distinct-asset count of every list leaves the device
                int rf;
                if ((rf = h->d_freq.ensure(m))) return rf;
                isk::DistinctParams dp{d_rec, d_cnt, h->d_freq.p, k, (uint32_t)t.key_words};
                hipLaunchKernelGGL(isk::distinct_kernel, dim3(m), dim3(isk::BLOCK), 0, h->stream, dp);
                HIPOK(hipGetLastError());
                if (out_collisions) HIPOK(hipMemcpyAsync(p_cnt + m + flag_slots, d_cnt, m * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
                HIPOK(hipMemcpyAsync(p_cnt, h->d_freq.p, m * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
                return 0;
            }
            if (direct) return 0;                                  // already written where the host reads it
            if (sink) {
                // the lists are final on the device (or will be redone and this queued again): mark the best chunk of every
                // (asset, query), append them to the request's entry list; the host gets counts, flags, k-th distances and info
                uint32_t* const d_info = d_cnt + m + flag_slots + m;
                if (sink->exact) {
                    HIPOK(hipMemcpyAsync(h->d_sp_cnt.p + pos, d_cnt, (size_t)m * sizeof(uint32_t), hipMemcpyDeviceToDevice, h->stream));
                    if (pos == 0 && m == sink->nd && sink->d_of_g)
                        HIPOK(isksp::exact_prepare(sink->buf, d_cnt, sink->d_of_g, sink->nd, sink->ng, k, d_info, h->stream));
                } else {
                    isksp::BatchArgs ba{pos, m, k, d_cnt, sink->h_max, sink->dup_limit, sink->entries, d_info};
                    HIPOK(isksp::queue_batch(sink->buf, ba, h->stream));
                }
                HIPOK(hipMemcpyAsync(h->p_block.p, h->d_block.p, block_bytes, hipMemcpyDeviceToHost, h->stream));
                return 0;
            }
            const size_t bytes = rec_bytes + (size_t)m * sizeof(uint32_t) + (one_copy ? batch.flag_words() * sizeof(uint32_t) : 0);
            HIPOK(hipMemcpyAsync(h->p_block.p, h->d_block.p, bytes, hipMemcpyDeviceToHost, h->stream));
            return 0;
        };
        auto worst_ratio = [&]() -> double {                 // worst k-th NPHD of the merged lists; < 0: some query holds fewer than k rows
            double worst = 0.0;
            for (uint32_t i = 0; i < m; ++i) {
                if (p_cnt[i] < k) return -1.0;
                const isk::Record& r = p_rec[(size_t)i * k + k - 1];
                worst = std::max(worst, r.prefix_bits ? (double)r.hamming / (double)r.prefix_bits : 0.0);
            }
            return worst;
        };
        if ((rc = batch.begin(hq.data()))) return rc;
        if (spec == Spec::ratio && !batch.multi) {          // (every non-empty segment is a job: cannot happen; never answer unverified)
            spec = Spec::none;
            batch.radius_ratio = -1.0;
            if ((rc = batch.begin(hq.data()))) return rc;
        }
        if (spec == Spec::self_hint && !batch.used_hint) spec = Spec::none;     // (no job took the single pass: nothing to verify)
        bool spec_ok = false;
        if (spec != Spec::none) {
            if ((rc = batch.merge())) return rc;
            if ((rc = batch.copy_flags())) return rc;
            if ((rc = copy_results())) return rc;
            HIPOK(hipStreamSynchronize(h->stream));
            // (ratio: a row outside a radius lies beyond floor(ratio x bits) + 1 bits, strictly farther than the worst k-th NPHD)
            spec_ok = spec == Spec::ratio ? batch.complete(p_cnt, k) && worst_ratio() <= batch.radius_ratio : batch.complete(p_cnt, spec_seg->n);
            if (spec_ok) h->stats.spec_hits += 1;
            else {
                h->stats.spec_misses += 1;
                if (spec == Spec::ratio) t.mhint(m, len).miss();
                else spec_seg->hint(m, len).miss();
                batch.radius = radius; batch.self_hint = -1; batch.used_hint = false; batch.radius_ratio = -1.0;     // the ordinary pass
                if ((rc = batch.begin(hq.data()))) return rc;
            }
        }
        if (!spec_ok && (rc = batch.finish(hq.data(), copy_results))) return rc;
        if (h->count_candidates && batch.jobs.size() == 1) {
            // accounting (tools/probe_candidate_path.py, option "count_candidates"): how many candidates the scan appended for this batch
            std::vector<uint32_t> hc((size_t)batch.nq_pad * isk::CNT_STRIDE);
            HIPOK(hipMemcpyAsync(hc.data(), h->d_cnt.p, hc.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
            HIPOK(hipStreamSynchronize(h->stream));
            for (uint32_t i = 0; i < m; ++i) h->stats.candidates += hc[(size_t)i * isk::CNT_STRIDE];
            h->stats.candidate_batches += 1;
        }
        // where this batch's lists ended: the next batch of its class starts there (+ the hint's margin)
        if (hintable && !batch.jobs.empty()) record_hint(spec_seg->hint(m, len), spec_ok, m, k, p_cnt, p_rec, sink ? p_kth : nullptr);
        if (mhintable) {
            const double worst = worst_ratio();
            if (spec_ok) t.mhint(m, len).hit(worst);
            else if (worst >= 0.0) t.mhint(m, len).seed(k, worst);
        }
        if (sink) {
            if (!batch.jobs.empty()) {
                const uint32_t* p_info = p_kth + m;
                if (!sink->exact) {
                    sink->entries = p_info[0];
                    sink->unknown_any = sink->unknown_any || p_info[1] != 0;
                } else if (pos == 0 && m == sink->nd && sink->d_of_g) {
                    sink->entries = p_info[0];
                    sink->prepared = true;
                }
                for (uint32_t i = 0; i < m; ++i) sink->max_count = std::max(sink->max_count, std::min(p_cnt[i], k));
                if (sink->q_count) for (uint32_t i = 0; i < m; ++i) sink->q_count[pos + i] = std::min(p_cnt[i], k);
            }
            pos = end;
            continue;
        }
        if (out_freq) {
            if (batch.jobs.empty()) for (uint32_t i = 0; i < m; ++i) out_freq[order[pos + i]] = 0;
            else for (uint32_t i = 0; i < m; ++i) out_freq[order[pos + i]] = p_cnt[i];
            if (out_collisions)
                for (uint32_t i = 0; i < m; ++i) out_collisions[order[pos + i]] = batch.jobs.empty() ? 0 : p_cnt[m + flag_slots + i];
        } else {
            unpack_records(p_rec, p_cnt, m, k, t.key_words, &order[pos], out_keys, out_hamming, out_prefix_bits, out_count);
        }
        pos = end;
    }
    return 0;
}

// Searches arriving from many threads are COMBINED: the reference calls `search` once per query unit from
// FastAPI's thread pool (usearch/index.py:786-806, docs/explanation/architecture.md:120-126), and a
// streaming pass costs the same for one query as for T_q.  The first caller becomes the leader, takes every
// request waiting on the same (table, k) and runs them as ONE batch; the others sleep until their slice of
// the results has been written.  A single-threaded caller pays nothing for this.
struct PendingSearch {
    uint32_t table, nq, k;
    const uint64_t* q_words;
    const uint8_t* q_nbytes;
    uint64_t* out_keys;
    uint32_t* out_hamming;
    uint16_t* out_prefix_bits;
    uint32_t* out_count;
    int rc = 0;
    bool done = false;
    std::string err;
};

namespace {
void run_combined(isccsearch_handle* h, std::vector<PendingSearch*>& reqs) {
    std::lock_guard<std::mutex> lk(h->mu);
    std::vector<bool> handled(reqs.size(), false);
    for (size_t i = 0; i < reqs.size(); ++i) {
        if (handled[i]) continue;
        // requests sharing table and k (and therefore key width / words per query)
        std::vector<size_t> grp;
        for (size_t j = i; j < reqs.size(); ++j)
            if (!handled[j] && reqs[j]->table == reqs[i]->table && reqs[j]->k == reqs[i]->k) { grp.push_back(j); handled[j] = true; }
        h->stats.searches += grp.size();
        Table* tp = nullptr;
        int rc = get_table(h, reqs[i]->table, tp);
        // validate each request on its own so that one bad caller does not fail the others
        std::vector<size_t> ok;
        for (size_t j : grp) {
            PendingSearch* r = reqs[j];
            int rj = rc ? rc : check_query_lengths(*tp, r->nq, r->q_nbytes);
            if (rj) { r->rc = rj; r->err = g_last_error; }
            else ok.push_back(j);
        }
        if (ok.empty()) continue;
        if (ok.size() == 1) {
            PendingSearch* r = reqs[ok[0]];
            r->rc = search_locked(h, r->table, r->nq, r->q_words, r->q_nbytes, r->k, r->out_keys, r->out_hamming, r->out_prefix_bits, r->out_count);
            if (r->rc) r->err = g_last_error;
            continue;
        }
        const Table& t = *tp;
        const uint32_t k = reqs[i]->k;
        const int MW = t.max_words, KW = t.key_words;
        size_t total = 0;
        for (size_t j : ok) total += reqs[j]->nq;
        std::vector<uint64_t> qw(total * MW), okeys(total * k * KW);
        std::vector<uint8_t> qn(t.metric == ISCCSEARCH_METRIC_NPHD ? total : 0);
        std::vector<uint32_t> oh(total * k), oc(total);
        std::vector<uint16_t> op(total * k);
        size_t off = 0;
        for (size_t j : ok) {
            PendingSearch* r = reqs[j];
            memcpy(&qw[off * MW], r->q_words, (size_t)r->nq * MW * 8);
            if (!qn.empty()) memcpy(&qn[off], r->q_nbytes, r->nq);
            off += r->nq;
        }
        const int rg = search_locked(h, reqs[i]->table, (uint32_t)total, qw.data(), qn.empty() ? nullptr : qn.data(), k,
                                     okeys.data(), oh.data(), op.data(), oc.data());
        const std::string eg = rg ? g_last_error : std::string();
        off = 0;
        for (size_t j : ok) {
            PendingSearch* r = reqs[j];
            r->rc = rg;
            r->err = eg;
            if (!rg) {
                memcpy(r->out_keys, &okeys[off * k * KW], (size_t)r->nq * k * KW * 8);
                memcpy(r->out_hamming, &oh[off * k], (size_t)r->nq * k * 4);
                memcpy(r->out_prefix_bits, &op[off * k], (size_t)r->nq * k * 2);
                memcpy(r->out_count, &oc[off], (size_t)r->nq * 4);
            }
            off += r->nq;
        }
    }
}
}  // namespace

int isccsearch_search(isccsearch_handle* h, uint32_t table, uint32_t nq, const uint64_t* q_words,
                      const uint8_t* q_nbytes, uint32_t k,
                      uint64_t* out_keys, uint32_t* out_hamming, uint16_t* out_prefix_bits, uint32_t* out_count) {
    if (!h) return fail(-EINVAL, "handle is NULL");
    if (k < 1) return fail(-EINVAL, "`count` must be >= 1");
    if (k > ISCCSEARCH_MAX_K) return fail(-EINVAL, "count %u exceeds ISCCSEARCH_MAX_K (%d)", k, ISCCSEARCH_MAX_K);
    if (nq == 0) return 0;
    if (!q_words || !out_keys || !out_hamming || !out_prefix_bits || !out_count) return fail(-EINVAL, "NULL argument");
    PendingSearch me;
    me.table = table; me.nq = nq; me.k = k; me.q_words = q_words; me.q_nbytes = q_nbytes;
    me.out_keys = out_keys; me.out_hamming = out_hamming; me.out_prefix_bits = out_prefix_bits; me.out_count = out_count;
    {
        std::unique_lock<std::mutex> ql(h->qmu);
        h->pending.push_back(&me);
        for (;;) {
            if (me.done) {
                if (me.rc) g_last_error = me.err;
                return me.rc;
            }
            if (!h->leader_active) { h->leader_active = true; break; }   // nobody is serving: lead the next round
            h->qcv.wait(ql);
        }
    }
    // leader of exactly one round (it contains my own request), then hand over to a waiter
    std::vector<PendingSearch*> round;
    {
        std::unique_lock<std::mutex> ql(h->qmu);
        round.swap(h->pending);
    }
    run_combined(h, round);
    {
        std::unique_lock<std::mutex> ql(h->qmu);
        for (PendingSearch* r : round) r->done = true;
        h->leader_active = false;
    }
    h->qcv.notify_all();
    if (me.rc) g_last_error = me.err;
    return me.rc;
}

// Several searches, ONE synchronisation.  Requests over single-segment tables whose queries share one length are
// enqueued back to back (the device buffers are reused in stream order; only the pinned staging is sliced per
// request) and their result blocks are read after a single hipStreamSynchronize; everything else -- and any
// request whose candidate list overflowed -- takes the ordinary path afterwards.
int isccsearch_search_many(isccsearch_handle* h, uint32_t n, isccsearch_request* reqs) {
    if (!h) return fail(-EINVAL, "handle is NULL");
    if (n == 0) return 0;
    if (!reqs) return fail(-EINVAL, "NULL argument");
    std::lock_guard<std::mutex> lk(h->mu);
    HIPOK(hipSetDevice(h->device));
    struct Slot {
        std::unique_ptr<Batch> batch;
        std::vector<uint64_t> hq;
        size_t block_off = 0, rec_bytes = 0;
        Segment* seg = nullptr;
        bool small = false, spec = false;
        uint32_t len = 0;      // compared prefix length of the request (the hint is kept per length)
    };
    std::vector<Slot> slots(n);
    std::vector<bool> deferred(n, false);
    int first_error = 0;
    auto reject = [&](isccsearch_request& r, int rc) { r.status = rc; if (!first_error) first_error = rc; };

    // pass 1: validate, pick the requests that can be deferred, size the pinned staging once (a later ensure()
    // would move slices that are already referenced by queued copies)
    size_t pq_words = 0, block_total = 0, block_max = 0;
    for (uint32_t i = 0; i < n; ++i) {
        isccsearch_request& r = reqs[i];
        r.status = 0;
        if (r.nq == 0) continue;
        if (r.k < 1) { reject(r, fail(-EINVAL, "`count` must be >= 1")); continue; }
        if (r.k > ISCCSEARCH_MAX_K) { reject(r, fail(-EINVAL, "count %u exceeds ISCCSEARCH_MAX_K (%d)", r.k, ISCCSEARCH_MAX_K)); continue; }
        if (r.max_hamming > 256) { reject(r, fail(-EINVAL, "max_hamming %d exceeds 256", r.max_hamming)); continue; }
        if (!r.q_words || !r.out_keys || !r.out_hamming || !r.out_prefix_bits || !r.out_count) { reject(r, fail(-EINVAL, "NULL argument")); continue; }
        Table* tp;
        int rc = get_table(h, r.table, tp);
        if (!rc) rc = check_query_lengths(*tp, r.nq, r.q_nbytes);
        if (rc) { reject(r, rc); continue; }
        const Table& t = *tp;
        bool one_len = true;
        if (t.metric == ISCCSEARCH_METRIC_NPHD)
            for (uint32_t q = 1; q < r.nq; ++q) one_len = one_len && r.q_nbytes[q] == r.q_nbytes[0];
        if (t.segments() != 1 || !one_len || r.nq > QB_MAX) continue;     // ordinary path below
        deferred[i] = true;
        Slot& sl = slots[i];
        sl.rec_bytes = (size_t)r.nq * r.k * sizeof(isk::Record);
        const size_t bytes = (sl.rec_bytes + ((size_t)r.nq + (size_t)r.nq + 16) * sizeof(uint32_t) + 15) & ~(size_t)15;
        sl.block_off = block_total;
        block_total += bytes;
        block_max = std::max(block_max, bytes);
        pq_words += ((size_t)r.nq + 16) * 4;
    }
    int rc;
    if (h->ev_staged_pending) { HIPOK(hipEventSynchronize(h->ev_staged)); h->ev_staged_pending = false; }   // see Batch::begin
    if ((rc = h->p_queries.ensure(pq_words))) return rc;
    if ((rc = h->p_block.ensure(block_total))) return rc;
    if ((rc = h->d_block.ensure(block_max))) return rc;

    // pass 2: enqueue
    size_t pq_off = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (!deferred[i]) continue;
        isccsearch_request& r = reqs[i];
        Table& t = *h->tables[r.table];
        Slot& sl = slots[i];
        const uint32_t len = t.metric == ISCCSEARCH_METRIC_NPHD ? r.q_nbytes[0] : (uint32_t)t.max_bytes;
        isk::Record* const d_rec = reinterpret_cast<isk::Record*>(h->d_block.p);
        uint32_t* const d_cnt = reinterpret_cast<uint32_t*>(h->d_block.p + sl.rec_bytes);
        uint32_t* const p_cnt = reinterpret_cast<uint32_t*>(h->p_block.p + sl.block_off + sl.rec_bytes);
        sl.batch.reset(new Batch(h, t, r.nq, len, r.k, d_rec, d_cnt));
        Batch& b = *sl.batch;
        b.radius = r.max_hamming < 0 ? -1 : r.max_hamming;
        // small top-k batches: the speculative single pass of search_locked (see there), verified in pass 3a
        sl.seg = t.sole_segment();
        sl.small = r.max_hamming < 0 && r.nq <= h->spec_max_queries && sl.seg && r.k <= sl.seg->n;
        sl.len = len;
        sl.spec = sl.small && h->speculate && sl.seg->hint(r.nq, len).ready(r.k);
        if (sl.spec) b.radius = (int)sl.seg->hint(r.nq, len).tau;
        b.pq_off = pq_off;
        b.d_flags = d_cnt + r.nq;
        b.h_flags = p_cnt + r.nq;
        pq_off += ((size_t)r.nq + 16) * 4;
        sl.hq.assign(r.q_words, r.q_words + (size_t)r.nq * t.max_words);
        h->stats.searches += 1;
        h->stats.queries += r.nq;
        if ((rc = b.begin(sl.hq.data()))) return rc;
        const size_t bytes = sl.rec_bytes + ((size_t)r.nq + b.flag_words()) * sizeof(uint32_t);
        HIPOK(hipMemcpyAsync(h->p_block.p + sl.block_off, h->d_block.p, bytes, hipMemcpyDeviceToHost, h->stream));
    }
    HIPOK(hipStreamSynchronize(h->stream));

    // pass 3a: hand out EVERY deferred result first.  The ordinary pipeline below stages its own results in p_block
    // from offset 0 (and may reallocate it), so no deferred slice may still be unread when it runs.
    std::vector<bool> ordinary(n, false), respec(n, true);      // respec: the ordinary rerun may itself speculate (not after a miss)
    for (uint32_t i = 0; i < n; ++i) {
        isccsearch_request& r = reqs[i];
        if (r.status || r.nq == 0) continue;
        if (!deferred[i]) { ordinary[i] = true; continue; }
        Batch& b = *slots[i].batch;
        const isk::Record* p_rec = reinterpret_cast<const isk::Record*>(h->p_block.p + slots[i].block_off);
        const uint32_t* p_cnt = reinterpret_cast<const uint32_t*>(h->p_block.p + slots[i].block_off + slots[i].rec_bytes);
        Slot& sl = slots[i];
        if (sl.spec) {
            if (b.complete(p_cnt, sl.seg->n)) h->stats.spec_hits += 1;
            else { h->stats.spec_misses += 1; sl.seg->hint(r.nq, sl.len).miss(); ordinary[i] = true; respec[i] = false; continue; }      // (the ordinary path re-seeds the radius)
        }
        if (b.any_flag()) { ordinary[i] = true; continue; }   // rare: exact fallback through the normal path
        if (sl.small && !b.jobs.empty()) record_hint(sl.seg->hint(r.nq, sl.len), sl.spec, r.nq, r.k, p_cnt, p_rec, nullptr);
        unpack_records(p_rec, p_cnt, r.nq, r.k, h->tables[r.table]->key_words, nullptr, r.out_keys, r.out_hamming, r.out_prefix_bits, r.out_count);
    }
    // pass 3b: overflowed and non-deferred requests run the ordinary pipeline
    for (uint32_t i = 0; i < n; ++i) {
        if (!ordinary[i]) continue;
        isccsearch_request& r = reqs[i];
        if (!deferred[i]) h->stats.searches += 1;
        h->spec_suppress = !respec[i];
        rc = search_locked(h, r.table, r.nq, r.q_words, r.q_nbytes, r.k, r.out_keys, r.out_hamming, r.out_prefix_bits, r.out_count,
                           r.max_hamming < 0 ? -1 : r.max_hamming);
        h->spec_suppress = false;
        if (rc) reject(r, rc);
    }
    return first_error;
}

int isccsearch_search_within(isccsearch_handle* h, uint32_t table, uint32_t nq, const uint64_t* q_words,
                             const uint8_t* q_nbytes, uint32_t k, uint32_t max_hamming,
                             uint64_t* out_keys, uint32_t* out_hamming, uint16_t* out_prefix_bits, uint32_t* out_count) {
    if (!h) return fail(-EINVAL, "handle is NULL");
    if (k < 1) return fail(-EINVAL, "`count` must be >= 1");
    if (k > ISCCSEARCH_MAX_K) return fail(-EINVAL, "count %u exceeds ISCCSEARCH_MAX_K (%d)", k, ISCCSEARCH_MAX_K);
    if (max_hamming > 256) return fail(-EINVAL, "max_hamming %u exceeds 256", max_hamming);
    if (nq == 0) return 0;
    if (!q_words || !out_keys || !out_hamming || !out_prefix_bits || !out_count) return fail(-EINVAL, "NULL argument");
    std::lock_guard<std::mutex> lk(h->mu);
    h->stats.searches += 1;
    return search_locked(h, table, nq, q_words, q_nbytes, k, out_keys, out_hamming, out_prefix_bits, out_count, (int)max_hamming);
}

// One join_scan_kernel launch per pair of segments (join.hip.h), all appending to one output; the pairs are sorted on the host.
int isccsearch_join_within(isccsearch_handle* h, uint32_t table, const int16_t* max_hamming, uint64_t capacity,
                           uint64_t* out_keys_a, uint64_t* out_keys_b, uint32_t* out_hamming, uint16_t* out_prefix_bits,
                           uint64_t* out_total) {
    if (!h) return fail(-EINVAL, "handle is NULL");
    if (!max_hamming || !out_total) return fail(-EINVAL, "NULL argument");
    *out_total = 0;
    if (capacity && (!out_keys_a || !out_keys_b || !out_hamming || !out_prefix_bits))
        return fail(-EINVAL, "NULL output array with capacity %llu", (unsigned long long)capacity);
    std::lock_guard<std::mutex> lk(h->mu);
    Table* tp;
    int rc = get_table(h, table, tp);
    if (rc) return rc;
    Table& t = *tp;
    HIPOK(hipSetDevice(h->device));
    const uint32_t KW = (uint32_t)t.key_words;
    const uint64_t cap_alloc = std::max<uint64_t>(capacity, 1);
    if ((rc = h->d_join_keys.ensure(cap_alloc * 2 * KW))) return rc;
    if ((rc = h->d_join_ham.ensure(cap_alloc))) return rc;
    if ((rc = h->d_join_pb.ensure(cap_alloc))) return rc;
    if ((rc = h->d_join_total.ensure(1))) return rc;
    HIPOK(hipMemsetAsync(h->d_join_total.p, 0, 8, h->stream));
    // one launch per pair of segments (la <= lb: the pair compares la bytes under max_hamming[la]); what only the emit path
    // reads goes to the device as one array of descriptors
    struct Launch { isk::JoinParams jp; uint32_t W; bool mask; uint64_t blocks; };
    std::vector<Launch> launches;
    std::vector<isk::JoinEmit> emits;
    for (uint32_t la = 1; la <= ISCCSEARCH_MAX_BYTES; ++la) {
        if (!t.seg[la].n || max_hamming[la] < 0) continue;
        for (uint32_t lb = la; lb <= ISCCSEARCH_MAX_BYTES; ++lb) {
            const bool same = la == lb;
            if (!t.seg[lb].n || (same && t.seg[la].n < 2)) continue;
            // side A (one block per TQ rows) is the segment with more rows; side B is streamed by every block
            Segment& A = t.seg[lb].n > t.seg[la].n ? t.seg[lb] : t.seg[la];
            Segment& B = &A == &t.seg[la] ? t.seg[lb] : t.seg[la];
            const uint32_t W = (la + 7) / 8;
            Launch L{};
            for (uint32_t w = 0; w < W; ++w) { L.jp.col_a[w] = A.col[w]; L.jp.col_b[w] = B.col[w]; }
            L.jp.n_a = A.n; L.jp.n_b = B.n;
            L.jp.mask = mask_for(la);
            L.jp.tau = (uint32_t)std::min<int>(max_hamming[la], 8 * ISCCSEARCH_MAX_BYTES);
            L.jp.same = same ? 1u : 0u;
            isk::JoinEmit e{};
            e.keys_a = A.keys; e.keys_b = B.keys;
            e.n_a = A.n;
            e.capacity = capacity;
            e.total = reinterpret_cast<unsigned long long*>(h->d_join_total.p);
            e.out_keys_a = h->d_join_keys.p;
            e.out_keys_b = h->d_join_keys.p + cap_alloc * KW;
            e.out_hamming = h->d_join_ham.p;
            e.out_prefix_bits = h->d_join_pb.p;
            e.prefix_bits = 8 * la;
            e.kw = KW;
            // within one segment the last row pairs with no later one
            const uint64_t a_rows = same ? A.n - 1 : A.n;
            L.W = W;
            L.mask = la % 8 != 0;
            L.blocks = (a_rows + join_rows_per_block(W) - 1) / join_rows_per_block(W);
            if (L.blocks >= (1ull << 31) || B.n >= (1ull << 40))
                return fail(-E2BIG, "segments of %llu x %llu rows exceed the join kernel's grid", (unsigned long long)A.n, (unsigned long long)B.n);
            launches.push_back(L);
            emits.push_back(e);
        }
    }
    if (!launches.empty()) {
        if ((rc = h->d_join_emit.ensure(emits.size()))) return rc;
        HIPOK(hipMemcpyAsync(h->d_join_emit.p, emits.data(), emits.size() * sizeof(isk::JoinEmit), hipMemcpyHostToDevice, h->stream));
        for (size_t i = 0; i < launches.size(); ++i) {
            Launch& L = launches[i];
            L.jp.e = h->d_join_emit.p + i;
            switch (L.W) {
                case 1: launch_join<1>(L.jp, L.mask, L.blocks, h->stream); break;
                case 2: launch_join<2>(L.jp, L.mask, L.blocks, h->stream); break;
                case 3: launch_join<3>(L.jp, L.mask, L.blocks, h->stream); break;
                default: launch_join<4>(L.jp, L.mask, L.blocks, h->stream); break;
            }
            HIPOK(hipGetLastError());
        }
    }
    uint64_t total = 0;
    HIPOK(hipMemcpyAsync(&total, h->d_join_total.p, 8, hipMemcpyDeviceToHost, h->stream));
    HIPOK(hipStreamSynchronize(h->stream));
    *out_total = total;
    if (total > capacity)
        return fail(-ENOSPC, "%llu pairs do not fit the capacity of %llu", (unsigned long long)total, (unsigned long long)capacity);
    if (!total) return 0;
    std::vector<uint64_t> ka(total * KW), kb(total * KW);
    std::vector<uint32_t> ham(total);
    std::vector<uint16_t> pb(total);
    HIPOK(hipMemcpyAsync(ka.data(), h->d_join_keys.p, total * KW * 8, hipMemcpyDeviceToHost, h->stream));
    HIPOK(hipMemcpyAsync(kb.data(), h->d_join_keys.p + cap_alloc * KW, total * KW * 8, hipMemcpyDeviceToHost, h->stream));
    HIPOK(hipMemcpyAsync(ham.data(), h->d_join_ham.p, total * 4, hipMemcpyDeviceToHost, h->stream));
    HIPOK(hipMemcpyAsync(pb.data(), h->d_join_pb.p, total * 2, hipMemcpyDeviceToHost, h->stream));
    HIPOK(hipStreamSynchronize(h->stream));
    // the kernels append in no particular order: sort by (key_a, key_b), each key compared as (hi, lo)
    std::vector<uint64_t> order(total);
    for (uint64_t i = 0; i < total; ++i) order[i] = i;
    auto key_less = [&](const uint64_t* x, const uint64_t* y) {
        for (uint32_t w = 0; w < KW; ++w)
            if (x[w] != y[w]) return x[w] < y[w];
        return false;
    };
    std::sort(order.begin(), order.end(), [&](uint64_t x, uint64_t y) {
        if (key_less(&ka[x * KW], &ka[y * KW])) return true;
        if (key_less(&ka[y * KW], &ka[x * KW])) return false;
        return key_less(&kb[x * KW], &kb[y * KW]);
    });
    for (uint64_t i = 0; i < total; ++i) {
        const uint64_t o = order[i];
        for (uint32_t w = 0; w < KW; ++w) { out_keys_a[i * KW + w] = ka[o * KW + w]; out_keys_b[i * KW + w] = kb[o * KW + w]; }
        out_hamming[i] = ham[o];
        out_prefix_bits[i] = pb[o];
    }
    return 0;
}

int isccsearch_doc_freq(isccsearch_handle* h, uint32_t table, uint32_t nq, const uint64_t* q_words,
                        const uint8_t* q_nbytes, uint32_t dup_limit, uint32_t* out_freq) {
    if (!h) return fail(-EINVAL, "handle is NULL");
    if (dup_limit < 1 || dup_limit > ISCCSEARCH_MAX_K) return fail(-EINVAL, "dup_limit %u outside 1..ISCCSEARCH_MAX_K (%d)", dup_limit, ISCCSEARCH_MAX_K);
    if (nq == 0) return 0;
    if (!q_words || !out_freq) return fail(-EINVAL, "NULL argument");
    std::lock_guard<std::mutex> lk(h->mu);
    h->stats.searches += 1;
    return search_locked(h, table, nq, q_words, q_nbytes, dup_limit, nullptr, nullptr, nullptr, nullptr, 0, out_freq);
}

int isccsearch_doc_freq_counted(isccsearch_handle* h, uint32_t table, uint32_t nq, const uint64_t* q_words,
                                const uint8_t* q_nbytes, uint32_t dup_limit, uint32_t* out_freq, uint32_t* out_collisions) {
    if (!h) return fail(-EINVAL, "handle is NULL");
    if (dup_limit < 1 || dup_limit > ISCCSEARCH_MAX_K) return fail(-EINVAL, "dup_limit %u outside 1..ISCCSEARCH_MAX_K (%d)", dup_limit, ISCCSEARCH_MAX_K);
    if (nq == 0) return 0;
    if (!q_words || !out_freq || !out_collisions) return fail(-EINVAL, "NULL argument");
    std::lock_guard<std::mutex> lk(h->mu);
    h->stats.searches += 1;
    return search_locked(h, table, nq, q_words, q_nbytes, dup_limit, nullptr, nullptr, nullptr, nullptr, 0, out_freq, out_collisions);
}

// The match threshold on the integer distance, the table's frequency column and the similarity / IDF tables of one scoring call
// (isccsearch_simprint_score and _many); h->mu is held.
static int simprint_setup(H* h, Table& t, Segment& s, double threshold, int64_t total_assets, uint32_t dup_limit, int& h_max) {
    int rc;
    const uint32_t bits = 8 * (uint32_t)t.max_bytes;
    // the match threshold on the integer distance: score = 1.0 - distance / ndim (usearch_core.py:182) falls with the distance, so
    // the largest distance whose score -- in this very arithmetic -- still passes is found once
    h_max = -1;
    for (uint32_t d = 0; d <= bits; ++d) {
        if (1.0 - (double)d / (double)bits >= threshold) h_max = (int)d;
        else break;
    }
    if (dup_limit && (rc = ensure_freq_column(h, t, s, dup_limit))) return rc;
    // similarity and IDF values come from the HOST's arithmetic (log() of libm is what CPython's math.log calls; lmdb_ops.py:67-81)
    const uint32_t n_idf = dup_limit + 1;
    if (h->sp_tab_bits != bits || h->sp_tab_dup != dup_limit || h->sp_tab_total != total_assets) {
        const size_t words = (size_t)bits + 1 + n_idf;
        if ((rc = h->p_sp_tab.ensure(words))) return rc;
        if ((rc = h->d_sp_tab.ensure(words))) return rc;
        HIPOK(hipStreamSynchronize(h->stream));      // (a previous upload may still be reading the staging block)
        double* tab = h->p_sp_tab.p;
        for (uint32_t d = 0; d <= bits; ++d) tab[d] = 1.0 - (double)d / (double)bits;
        auto idf = [&](uint32_t freq) { return total_assets <= 0 ? 0.0 : std::log(1.0 + (double)total_assets / (double)(1 + (uint64_t)freq)); };
        if (dup_limit) for (uint32_t f = 0; f <= dup_limit; ++f) tab[bits + 1 + f] = idf(f);
        else tab[bits + 1] = idf(1);
        HIPOK(hipMemcpyAsync(h->d_sp_tab.p, tab, words * sizeof(double), hipMemcpyHostToDevice, h->stream));
        h->sp_tab_bits = bits; h->sp_tab_dup = dup_limit; h->sp_tab_total = total_assets;
    }
    return 0;
}

// device buffers of a scoring call over nq query simprints with k neighbours each (entries == 0: the search's; else the scoring's)
static int simprint_buffers(H* h, uint32_t nq, uint32_t k, uint32_t entries) {
    int rc;
    if (entries == 0) {
        const size_t slots = (size_t)nq * k;
        if ((rc = h->d_sp_rec.ensure(slots))) return rc;
        if ((rc = h->d_sp_rows.ensure(slots))) return rc;
        if ((rc = h->d_sp_best.ensure(slots))) return rc;
        if ((rc = h->d_sp_nbest.ensure(nq))) return rc;
        if ((rc = h->d_sp_offs.ensure(nq))) return rc;
        if ((rc = h->d_sp_freqq.ensure(nq))) return rc;
        if ((rc = h->d_sp_unknown.ensure(nq))) return rc;
        if ((rc = h->d_sp_nassets.ensure(1))) return rc;
        for (int i = 0; i < 2; ++i) {
            if ((rc = h->d_sp_asset[i].ensure(slots))) return rc;
            if ((rc = h->d_sp_entry[i].ensure(slots))) return rc;
        }
        return 0;
    }
    for (int i = 0; i < 2; ++i) {
        if ((rc = h->d_sp_score[i].ensure(entries))) return rc;
        if ((rc = h->d_sp_order[i].ensure(entries))) return rc;
    }
    if ((rc = h->d_sp_matches.ensure(entries))) return rc;
    if ((rc = h->d_sp_ws.ensure(entries))) return rc;
    if ((rc = h->d_sp_idfq.ensure(nq))) return rc;
    return 0;
}

static void simprint_bind(H* h, isksp::Buffers& b) {
    b.rec = reinterpret_cast<const isccsearch_record*>(h->d_sp_rec.p);
    b.rows = h->d_sp_rows.p; b.best = h->d_sp_best.p; b.nbest = h->d_sp_nbest.p; b.offs = h->d_sp_offs.p;
    b.freq_q = h->d_sp_freqq.p; b.unknown = h->d_sp_unknown.p; b.n_assets = h->d_sp_nassets.p;
    for (int i = 0; i < 2; ++i) {
        b.c_asset[i] = h->d_sp_asset[i].p; b.c_entry[i] = h->d_sp_entry[i].p;
        b.score[i] = h->d_sp_score[i].p; b.order[i] = h->d_sp_order[i].p;
    }
    b.matches = h->d_sp_matches.p; b.ws = h->d_sp_ws.p; b.idf_q = h->d_sp_idfq.p;
    b.temp = h->d_sp_temp.p; b.temp_bytes = h->d_sp_temp.n;
}

// rare: a query simprint with k equal stored rows and k < dup_limit -- its document frequency needs the collision scan
static int simprint_unknown_freq(H* h, uint32_t table, Table& t, uint32_t nq, const uint64_t* q_words, uint32_t dup_limit) {
    int rc;
    std::vector<uint32_t> unk(nq), fq(nq);
    HIPOK(hipMemcpyAsync(unk.data(), h->d_sp_unknown.p, (size_t)nq * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    HIPOK(hipMemcpyAsync(fq.data(), h->d_sp_freqq.p, (size_t)nq * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    HIPOK(hipStreamSynchronize(h->stream));
    std::vector<uint32_t> which;
    for (uint32_t q = 0; q < nq; ++q) if (unk[q]) which.push_back(q);
    std::vector<uint64_t> qw(which.size() * (size_t)t.max_words);
    for (size_t i = 0; i < which.size(); ++i) memcpy(&qw[i * t.max_words], q_words + (size_t)which[i] * t.max_words, (size_t)t.max_words * 8);
    std::vector<uint32_t> freq(which.size());
    if ((rc = search_locked(h, table, (uint32_t)which.size(), qw.data(), nullptr, dup_limit, nullptr, nullptr, nullptr, nullptr, 0, freq.data()))) return rc;
    for (size_t i = 0; i < which.size(); ++i) fq[which[i]] = freq[i];
    HIPOK(hipMemcpyAsync(h->d_sp_freqq.p, fq.data(), (size_t)nq * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    HIPOK(hipStreamSynchronize(h->stream));       // (fq leaves scope)
    return 0;
}

// The scoring of isccsearch_simprint_score and _many once their arguments are checked (out_info zeroed; request r = query simprints
// [req_offsets[r], req_offsets[r + 1]), at most MAX_QUERY_SIMPRINTS each): consecutive requests of at most MAX_QUERY_SIMPRINTS query
// simprints form a round, a request is never split.  A round is ONE search with the lists left on the device and one scoring: a round
// of one request takes queue_score's pipeline, a round of several queue_score_many's (which returns per request what queue_score would).
static int simprint_score_rounds(H* h, uint32_t table, uint32_t n_req, const uint32_t* req_offsets, const uint64_t* q_words,
                                 uint32_t count, int32_t max_hamming, double threshold, uint32_t limit,
                                 int64_t total_assets, uint32_t dup_limit,
                                 isccsearch_simprint_result* out_results, isccsearch_simprint_chunk* out_chunks,
                                 uint64_t* out_chunk_words, uint32_t* out_info) {
    std::lock_guard<std::mutex> lk(h->mu);
    Table* tp;
    int rc = get_table(h, table, tp);
    if (rc) return rc;
    Table& t = *tp;
    if (t.metric != ISCCSEARCH_METRIC_HAMMING || t.key_words != 2)
        return fail(-EINVAL, "simprint scoring is defined for fixed-length (Hamming) tables with 128-bit chunk-pointer keys");
    Segment& s = t.seg[t.max_bytes];
    if (s.n == 0) return 0;
    if (s.n > 0xFFFFFFFFull) return fail(-E2BIG, "simprint scoring addresses rows with 32 bits; the table holds %llu", (unsigned long long)s.n);
    HIPOK(hipSetDevice(h->device));
    const uint32_t k = count, bits = 8 * (uint32_t)t.max_bytes, W = (uint32_t)t.max_words;
    int h_max = -1;
    if ((rc = simprint_setup(h, t, s, threshold, total_assets, dup_limit, h_max))) return rc;
    std::vector<uint32_t>& qbeg = h->h_sp_qbeg;
    std::vector<uint32_t>& q_count = h->h_sp_qcount;
    for (uint32_t r0 = 0; r0 < n_req;) {
        const uint32_t base = req_offsets[r0];
        uint32_t r1 = r0 + 1;
        while (r1 < n_req && req_offsets[r1 + 1] - base <= isksp::MAX_QUERY_SIMPRINTS) ++r1;
        const uint32_t nq = req_offsets[r1] - base, nr = r1 - r0;
        const uint64_t* const qw = q_words + (size_t)base * t.max_words;
        if (nq == 0) { r0 = r1; continue; }
        h->stats.searches += 1;
        if ((rc = simprint_buffers(h, nq, k, 0))) return rc;
        q_count.assign(nq, 0);
        ScoreSink sink;
        sink.h_max = h_max;
        sink.dup_limit = dup_limit;
        sink.q_count = q_count.data();
        simprint_bind(h, sink.buf);
        if ((rc = search_locked(h, table, nq, qw, nullptr, k, nullptr, nullptr, nullptr, nullptr, max_hamming < 0 ? -1 : max_hamming, nullptr, nullptr, &sink))) return rc;
        uint32_t words = 0;                // LDS words of the score kernel: the most 64-bit words one request's range touches
        qbeg.resize(nr + 1);
        for (uint32_t r = 0; r < nr; ++r) {
            const uint32_t qb = req_offsets[r0 + r] - base, qe = req_offsets[r0 + r + 1] - base;
            qbeg[r] = qb;
            uint32_t longest = 0;
            for (uint32_t q = qb; q < qe; ++q) longest = std::max(longest, q_count[q]);
            out_info[4 * (size_t)(r0 + r) + 2] = longest;
            if (qe > qb) words = std::max(words, ((qe - 1) >> 6) - (qb >> 6) + 1);
        }
        qbeg[nr] = nq;
        const uint32_t entries = sink.entries;
        if (entries == 0) { r0 = r1; continue; }
        if (sink.unknown_any && (rc = simprint_unknown_freq(h, table, t, nq, qw, dup_limit))) return rc;
        const uint32_t cap = (uint32_t)std::min<uint64_t>((uint64_t)nr * limit, entries);
        if ((rc = simprint_buffers(h, nq, k, entries))) return rc;
        if (nr == 1) {
            if ((rc = h->d_sp_temp.ensure(isksp::sort_temp_bytes(entries)))) return rc;
        } else {
            for (int i = 0; i < 2; ++i) {
                if ((rc = h->d_spm_req[i].ensure(entries))) return rc;
                if ((rc = h->d_spm_idx[i].ensure(entries))) return rc;
            }
            if ((rc = h->d_spm_qbeg.ensure(nr + 1))) return rc;
            if ((rc = h->d_spm_nassets.ensure(nr))) return rc;
            if ((rc = h->d_spm_astart.ensure(nr + 1))) return rc;
            if ((rc = h->d_spm_estart.ensure(nr + 1))) return rc;
            if ((rc = h->d_spm_cnt.ensure(cap))) return rc;
            if ((rc = h->d_spm_cpos.ensure(cap))) return rc;
            if ((rc = h->d_sp_temp.ensure(isksp::many_temp_bytes(entries, cap)))) return rc;
        }
        simprint_bind(h, sink.buf);
        // outputs in pinned memory, written by the emit kernels themselves, compact: {info[nr][4] | results[cap] | chunks | chunk words}
        const size_t res_off = ((size_t)nr * 16 + 15) / 16 * 16, chunk_off = res_off + (size_t)cap * sizeof(isccsearch_simprint_result);
        const size_t chunk_cap = out_chunks ? (size_t)std::min<uint64_t>((uint64_t)limit * nq, entries) : 0;
        const size_t words_off = chunk_off + chunk_cap * sizeof(isccsearch_simprint_chunk);
        if ((rc = h->p_sp_out.ensure(words_off + chunk_cap * W * 8))) return rc;
        unsigned char* const po = h->p_sp_out.p;
        isksp::ScoreArgs sa{};
        sa.nq = nq; sa.k = k; sa.entries = entries; sa.limit = limit;
        sa.sim_tab = h->d_sp_tab.p; sa.idf_tab = h->d_sp_tab.p + bits + 1; sa.dup_limit = dup_limit;
        sa.freq_col = dup_limit ? s.freq : nullptr;
        for (uint32_t w = 0; w < s.W; ++w) sa.col[w] = s.col[w];
        sa.W = W;
        sa.out_info = reinterpret_cast<uint32_t*>(po);
        sa.out_results = reinterpret_cast<isccsearch_simprint_result*>(po + res_off);
        sa.out_chunks = out_chunks ? reinterpret_cast<isccsearch_simprint_chunk*>(po + chunk_off) : nullptr;
        sa.out_chunk_words = out_chunks ? reinterpret_cast<uint64_t*>(po + words_off) : nullptr;
        if (nr == 1) {
            HIPOK(isksp::queue_score(sink.buf, sa, h->stream));
        } else {
            isksp::ManyBuffers mb{};
            for (int i = 0; i < 2; ++i) { mb.req[i] = h->d_spm_req[i].p; mb.idx[i] = h->d_spm_idx[i].p; }
            mb.qbeg = h->d_spm_qbeg.p; mb.n_assets = h->d_spm_nassets.p; mb.a_start = h->d_spm_astart.p; mb.e_start = h->d_spm_estart.p;
            mb.cnt = h->d_spm_cnt.p; mb.c_pos = h->d_spm_cpos.p;
            HIPOK(hipMemcpyAsync(mb.qbeg, qbeg.data(), (size_t)(nr + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
            isksp::ScoreManyArgs ma{sa, nr, cap, words};
            HIPOK(isksp::queue_score_many(sink.buf, mb, ma, h->stream));
        }
        HIPOK(hipStreamSynchronize(h->stream));       // (qbeg is read by the kernels until here)
        // into the caller's regions: request r's results at r x limit, its chunks at limit x req_offsets[r]
        const uint32_t* info = reinterpret_cast<const uint32_t*>(po);
        size_t res_at = 0, chunk_at = 0;
        for (uint32_t r = 0; r < nr; ++r) {
            const uint32_t n = info[4 * r], c = info[4 * r + 3];
            uint32_t* oi = out_info + 4 * (size_t)(r0 + r);
            oi[0] = n; oi[1] = info[4 * r + 1]; oi[3] = c;
            memcpy(out_results + (size_t)(r0 + r) * limit, po + res_off + res_at * sizeof(isccsearch_simprint_result), (size_t)n * sizeof(isccsearch_simprint_result));
            if (out_chunks && c) {
                const size_t dst = (size_t)limit * req_offsets[r0 + r];
                memcpy(out_chunks + dst, po + chunk_off + chunk_at * sizeof(isccsearch_simprint_chunk), (size_t)c * sizeof(isccsearch_simprint_chunk));
                memcpy(out_chunk_words + dst * W, po + words_off + chunk_at * W * 8, (size_t)c * W * 8);
            }
            res_at += n;
            chunk_at += c;
        }
        r0 = r1;
    }
    return 0;
}

// Search + asset scoring with the neighbour lists kept on the device (usearch_core.py:137-269); see include/isccsearch.h.
int isccsearch_simprint_score(isccsearch_handle* h, uint32_t table, uint32_t nq, const uint64_t* q_words,
                              uint32_t count, int32_t max_hamming, double threshold, uint32_t limit,
                              int64_t total_assets, uint32_t dup_limit,
                              isccsearch_simprint_result* out_results, isccsearch_simprint_chunk* out_chunks,
                              uint64_t* out_chunk_words, uint32_t* out_info) {
    if (!h) return fail(-EINVAL, "handle is NULL");
    if (count < 1) return fail(-EINVAL, "`count` must be >= 1");
    if (count > ISCCSEARCH_MAX_K) return fail(-EINVAL, "count %u exceeds ISCCSEARCH_MAX_K (%d)", count, ISCCSEARCH_MAX_K);
    if (max_hamming > 256) return fail(-EINVAL, "max_hamming %d exceeds 256", max_hamming);
    if (dup_limit > ISCCSEARCH_MAX_K) return fail(-EINVAL, "dup_limit %u exceeds ISCCSEARCH_MAX_K (%d)", dup_limit, ISCCSEARCH_MAX_K);
    if (limit < 1) return fail(-EINVAL, "limit must be >= 1");
    if (!out_info) return fail(-EINVAL, "NULL argument");
    out_info[0] = out_info[1] = out_info[2] = out_info[3] = 0;
    if (nq == 0) return 0;
    if (!q_words || !out_results || (out_chunks == nullptr) != (out_chunk_words == nullptr)) return fail(-EINVAL, "NULL argument");
    if (nq > isksp::MAX_QUERY_SIMPRINTS) return fail(-E2BIG, "%u query simprints exceed the %u one scoring call takes", nq, isksp::MAX_QUERY_SIMPRINTS);
    if (!(threshold == threshold)) return fail(-EINVAL, "threshold is not a number");
    const uint32_t req_offsets[2] = {0, nq};
    return simprint_score_rounds(h, table, 1, req_offsets, q_words, count, max_hamming, threshold, limit, total_assets, dup_limit,
                                 out_results, out_chunks, out_chunk_words, out_info);
}

// Many simprint requests against one table, each scored on its own (usearch_core.py:137-269 per request); see include/isccsearch.h.
int isccsearch_simprint_score_many(isccsearch_handle* h, uint32_t table, uint32_t n_req, const uint32_t* req_offsets, const uint64_t* q_words,
                                   uint32_t count, int32_t max_hamming, double threshold, uint32_t limit,
                                   int64_t total_assets, uint32_t dup_limit,
                                   isccsearch_simprint_result* out_results, isccsearch_simprint_chunk* out_chunks,
                                   uint64_t* out_chunk_words, uint32_t* out_info) {
    if (!h) return fail(-EINVAL, "handle is NULL");
    if (count < 1) return fail(-EINVAL, "`count` must be >= 1");
    if (count > ISCCSEARCH_MAX_K) return fail(-EINVAL, "count %u exceeds ISCCSEARCH_MAX_K (%d)", count, ISCCSEARCH_MAX_K);
    if (max_hamming > 256) return fail(-EINVAL, "max_hamming %d exceeds 256", max_hamming);
    if (dup_limit > ISCCSEARCH_MAX_K) return fail(-EINVAL, "dup_limit %u exceeds ISCCSEARCH_MAX_K (%d)", dup_limit, ISCCSEARCH_MAX_K);
    if (limit < 1) return fail(-EINVAL, "limit must be >= 1");
    if (n_req == 0) return 0;
    if (!out_info || !req_offsets) return fail(-EINVAL, "NULL argument");
    memset(out_info, 0, (size_t)n_req * 4 * sizeof(uint32_t));
    for (uint32_t r = 0; r < n_req; ++r) {
        if (req_offsets[r + 1] < req_offsets[r]) return fail(-EINVAL, "req_offsets must not decrease (request %u)", r);
        if (req_offsets[r + 1] - req_offsets[r] > isksp::MAX_QUERY_SIMPRINTS)
            return fail(-E2BIG, "request %u: %u query simprints exceed the %u one scoring call takes", r, req_offsets[r + 1] - req_offsets[r], isksp::MAX_QUERY_SIMPRINTS);
    }
    if (req_offsets[n_req] == req_offsets[0]) return 0;
    if (!q_words || !out_results || (out_chunks == nullptr) != (out_chunk_words == nullptr)) return fail(-EINVAL, "NULL argument");
    if ((uint64_t)limit * n_req > 0xFFFFFFFFull || (uint64_t)limit * req_offsets[n_req] > 0xFFFFFFFFull)
        return fail(-E2BIG, "limit %u x %u requests exceeds the 32-bit result addressing", limit, n_req);
    if (!(threshold == threshold)) return fail(-EINVAL, "threshold is not a number");
    return simprint_score_rounds(h, table, n_req, req_offsets, q_words, count, max_hamming, threshold, limit, total_assets, dup_limit,
                                 out_results, out_chunks, out_chunk_words, out_info);
}

// Hard-boundary simprint search with its scoring on the device (lmdb_ops.py:169-301); see include/isccsearch.h.
int isccsearch_simprint_exact(isccsearch_handle* h, uint32_t table, uint32_t n_distinct, const uint64_t* q_words,
                              uint32_t n_given, const uint32_t* given, uint32_t queried, uint32_t dup_limit, double threshold, uint32_t limit,
                              isccsearch_simprint_result* out_results, isccsearch_simprint_chunk* out_chunks, uint32_t* out_info) {
    if (!h) return fail(-EINVAL, "handle is NULL");
    if (dup_limit < 1) return fail(-EINVAL, "dup_limit must be >= 1");
    if (limit < 1) return fail(-EINVAL, "limit must be >= 1");
    if (!out_info) return fail(-EINVAL, "NULL argument");
    out_info[0] = out_info[1] = out_info[2] = out_info[3] = 0;
    if (n_distinct == 0 || n_given == 0) return 0;
    if (!q_words || !given || !out_results) return fail(-EINVAL, "NULL argument");
    if (n_distinct > isksp::MAX_QUERY_SIMPRINTS || n_given > isksp::MAX_QUERY_SIMPRINTS)
        return fail(-E2BIG, "%u / %u query simprints exceed the %u one scoring call takes", n_distinct, n_given, isksp::MAX_QUERY_SIMPRINTS);
    if (queried < n_given) return fail(-EINVAL, "queried (%u) counts every query simprint as given: it cannot be below n_given (%u)", queried, n_given);
    if (!(threshold == threshold)) return fail(-EINVAL, "threshold is not a number");
    for (uint32_t g = 0; g < n_given; ++g)
        if (given[g] >= n_distinct) return fail(-EINVAL, "given[%u] = %u is no index into the %u distinct simprints", g, given[g], n_distinct);
    std::lock_guard<std::mutex> lk(h->mu);
    Table* tp;
    int rc = get_table(h, table, tp);
    if (rc) return rc;
    Table& t = *tp;
    if (t.metric != ISCCSEARCH_METRIC_HAMMING || t.key_words != 2)
        return fail(-EINVAL, "simprint scoring is defined for fixed-length (Hamming) tables with 128-bit chunk-pointer keys");
    Segment& s = t.seg[t.max_bytes];
    if (s.n == 0) return 0;
    HIPOK(hipSetDevice(h->device));
    h->stats.searches += 1;
    const uint32_t k = std::min<uint32_t>(dup_limit, ISCCSEARCH_MAX_K), nd = n_distinct, ng = n_given;
    if ((rc = h->d_sp_rec.ensure((size_t)nd * k))) return rc;
    if ((rc = h->d_sp_cnt.ensure(nd))) return rc;
    if ((rc = h->d_sp_freqq.ensure(nd))) return rc;
    if ((rc = h->d_sp_dofg.ensure(ng))) return rc;
    if ((rc = h->d_sp_nbest.ensure(ng))) return rc;
    if ((rc = h->d_sp_unknown.ensure(ng))) return rc;
    if ((rc = h->d_sp_offs.ensure(ng))) return rc;
    if ((rc = h->d_sp_nassets.ensure(1))) return rc;
    ScoreSink sink;
    sink.exact = true;
    simprint_bind(h, sink.buf);
    // (the lookup of every given simprint goes up first: when one batch holds all lookups, hits and offsets are prepared behind its
    //  select and the number of entries arrives with the batch's own synchronisation)
    HIPOK(hipMemcpyAsync(h->d_sp_dofg.p, given, (size_t)ng * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    HIPOK(hipStreamSynchronize(h->stream));           // (`given` is the caller's memory)
    sink.d_of_g = h->d_sp_dofg.p; sink.nd = nd; sink.ng = ng;
    // every row equal to a query simprint, ascending key, at most dup_limit per simprint (lmdb_ops.py:197-210): the lists stay on the device
    if ((rc = search_locked(h, table, nd, q_words, nullptr, k, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, &sink))) return rc;
    out_info[2] = sink.max_count;
    uint32_t entries = sink.entries;
    if (!sink.prepared) {
        // several batches of lookups: hits per given simprint and their offsets now; the number of entries comes back with one small copy
        if ((rc = h->d_block.ensure(isksp::INFO_WORDS * sizeof(uint32_t)))) return rc;
        if ((rc = h->p_block.ensure(isksp::INFO_WORDS * sizeof(uint32_t)))) return rc;
        uint32_t* const d_info = reinterpret_cast<uint32_t*>(h->d_block.p);
        HIPOK(isksp::exact_prepare(sink.buf, h->d_sp_cnt.p, h->d_sp_dofg.p, nd, ng, k, d_info, h->stream));
        HIPOK(hipMemcpyAsync(h->p_block.p, d_info, isksp::INFO_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
        HIPOK(hipStreamSynchronize(h->stream));
        entries = reinterpret_cast<const uint32_t*>(h->p_block.p)[0];
    }
    if (entries == 0) return 0;
    for (int i = 0; i < 2; ++i) {
        if ((rc = h->d_sp_asset[i].ensure(entries))) return rc;
        if ((rc = h->d_sp_entry[i].ensure(entries))) return rc;
        if ((rc = h->d_sp_score[i].ensure(entries))) return rc;
        if ((rc = h->d_sp_order[i].ensure(entries))) return rc;
    }
    if ((rc = h->d_sp_matches.ensure(entries))) return rc;
    if ((rc = h->d_sp_temp.ensure(isksp::sort_temp_bytes(entries)))) return rc;
    simprint_bind(h, sink.buf);
    const size_t res_off = 16, chunk_off = res_off + (size_t)limit * sizeof(isccsearch_simprint_result);
    const size_t chunk_cap = out_chunks ? entries : 0;
    if ((rc = h->p_sp_out.ensure(chunk_off + chunk_cap * sizeof(isccsearch_simprint_chunk)))) return rc;
    unsigned char* const po = h->p_sp_out.p;
    isksp::ExactArgs ea{};
    ea.nd = nd; ea.ng = ng; ea.k = k; ea.entries = entries; ea.limit = limit; ea.queried = queried;
    ea.d_of_g = h->d_sp_dofg.p; ea.threshold = threshold;
    ea.out_info = reinterpret_cast<uint32_t*>(po);
    ea.out_results = reinterpret_cast<isccsearch_simprint_result*>(po + res_off);
    ea.out_chunks = out_chunks ? reinterpret_cast<isccsearch_simprint_chunk*>(po + chunk_off) : nullptr;
    HIPOK(isksp::queue_exact(sink.buf, ea, h->stream));
    HIPOK(hipStreamSynchronize(h->stream));
    const uint32_t* info = reinterpret_cast<const uint32_t*>(po);
    out_info[0] = info[0]; out_info[1] = info[1]; out_info[3] = info[3];
    memcpy(out_results, po + res_off, (size_t)info[0] * sizeof(isccsearch_simprint_result));
    if (out_chunks) memcpy(out_chunks, po + chunk_off, (size_t)info[3] * sizeof(isccsearch_simprint_chunk));
    return 0;
}

}  // extern "C"

// isccsearch_match_assets: the unit searches of many asset queries as one batch per (table, code length, kind), their lists left
// on the device, and asset_score.hip's scoring behind them.  One synchronisation for the searches over one-segment tables and the
// scoring together; tables of several code lengths take the synchronous per-batch path (their per-segment lists are merged with the
// host's help, Batch::finish) before those are queued; one more round only when an INSTANCE list came back full or a
// candidate list overflowed.
namespace {
constexpr uint64_t SCRATCH_BYTES = 256ull << 20;   // isccsearch_match_assets: global sort scratch of the scoring kernel, at most
struct AmChunk {
    uint32_t table, nbytes, k;
    int radius;
    std::vector<uint32_t> units;      // indices into the call's units
    isk::Record* d_rec = nullptr;
    uint32_t* d_cnt = nullptr;
    uint32_t* d_flags = nullptr;
    size_t flag_off = 0;              // (deferred chunks) first flag word in the call's flag area
    bool deferred = false;
    std::unique_ptr<Batch> batch;
    std::vector<uint64_t> hq;
};

// the queries of one chunk, packed for its table
void am_pack(const Table& t, const isccsearch_asset_unit* units, AmChunk& c) {
    c.hq.assign(c.units.size() * (size_t)t.max_words, 0);
    for (size_t i = 0; i < c.units.size(); ++i)
        for (int w = 0; w < t.max_words; ++w) c.hq[i * t.max_words + w] = units[c.units[i]].words[w];
}

// split the listed units into chunks of <= QB_MAX per (table, code length, kind), in first-appearance order
void am_chunks(const isccsearch_asset_unit* units, const std::vector<uint32_t>& which, uint32_t k_sim, uint32_t k_inst,
               std::vector<AmChunk>& out) {
    std::vector<size_t> open;      // chunks of this call still taking units
    for (uint32_t u : which) {
        const isccsearch_asset_unit& a = units[u];
        const int radius = a.max_hamming < 0 ? -1 : a.max_hamming;
        size_t at = out.size();
        for (size_t o : open)
            if (out[o].table == a.table && out[o].nbytes == a.nbytes && out[o].radius == radius && out[o].units.size() < QB_MAX) { at = o; break; }
        if (at == out.size()) {
            AmChunk c;
            c.table = a.table; c.nbytes = a.nbytes; c.radius = radius; c.k = radius < 0 ? k_sim : k_inst;
            out.push_back(std::move(c));
            open.push_back(at);
        }
        out[at].units.push_back(u);
    }
}
}  // namespace

extern "C" int isccsearch_match_assets(isccsearch_handle* h, uint32_t nq, const uint32_t* unit_offsets, const isccsearch_asset_unit* units,
                                       uint32_t limit, uint32_t instance_first_k, uint32_t instance_max_k,
                                       const uint64_t* exclude, const uint8_t* has_exclude,
                                       const double* score_table, const double* pow_table, double threshold, int compensated, uint32_t n_types,
                                       uint64_t* out_keys, double* out_scores, uint32_t* out_count, uint8_t* out_types, double* out_type_scores,
                                       uint32_t* out_unit_count) {
    if (!h) return fail(-EINVAL, "handle is NULL");
    if (nq == 0) return 0;
    if (nq > QB_MAX) return fail(-EINVAL, "%u asset queries exceed the %u per call", nq, QB_MAX);
    if (!unit_offsets || !exclude || !has_exclude || !score_table || !pow_table || !out_keys || !out_scores || !out_count || !out_types ||
        !out_type_scores || !out_unit_count)
        return fail(-EINVAL, "NULL argument");
    if (limit < 1 || limit > ISCCSEARCH_MAX_K) return fail(-EINVAL, "limit %u outside 1..%d", limit, ISCCSEARCH_MAX_K);
    if (instance_first_k < 1 || instance_first_k > instance_max_k || instance_max_k > ISCCSEARCH_MAX_K)
        return fail(-EINVAL, "INSTANCE list lengths %u / %u outside 1..%d", instance_first_k, instance_max_k, ISCCSEARCH_MAX_K);
    if (n_types < 1 || n_types > ISCCSEARCH_MAX_UNIT_TYPES) return fail(-EINVAL, "n_types %u outside 1..%d", n_types, ISCCSEARCH_MAX_UNIT_TYPES);
    if (unit_offsets[0] != 0) return fail(-EINVAL, "unit_offsets[0] must be 0");
    for (uint32_t q = 0; q < nq; ++q) {
        if (unit_offsets[q + 1] < unit_offsets[q]) return fail(-EINVAL, "unit_offsets decrease at query %u", q);
        if (unit_offsets[q + 1] - unit_offsets[q] > ISCCSEARCH_MAX_ASSET_UNITS)
            return fail(-EINVAL, "query %u holds %u units (at most %d)", q, unit_offsets[q + 1] - unit_offsets[q], ISCCSEARCH_MAX_ASSET_UNITS);
    }
    const uint32_t n_units = unit_offsets[nq];
    if (n_units && !units) return fail(-EINVAL, "NULL argument");
    std::lock_guard<std::mutex> lk(h->mu);
    for (uint32_t u = 0; u < n_units; ++u) {
        const isccsearch_asset_unit& a = units[u];
        Table* tp;
        int rc = get_table(h, a.table, tp);
        if (rc) return rc;
        if (tp->metric != ISCCSEARCH_METRIC_NPHD || tp->key_words != 1) return fail(-EINVAL, "unit %u: table %u is not an NPHD table with 64-bit keys", u, a.table);
        if (a.nbytes < 1 || a.nbytes > (uint32_t)tp->max_bytes) return fail(-EINVAL, "unit %u: %u bytes outside 1..%d", u, a.nbytes, tp->max_bytes);
        if (a.type >= n_types) return fail(-EINVAL, "unit %u: type %u >= n_types %u", u, a.type, n_types);
        if (a.max_hamming > 0) return fail(-EINVAL, "unit %u: max_hamming must be < 0 (similarity) or 0 (INSTANCE)", u);
    }
    HIPOK(hipSetDevice(h->device));
    int rc;

    // the chunks of the first round and their device areas
    std::vector<uint32_t> all(n_units);
    for (uint32_t u = 0; u < n_units; ++u) all[u] = u;
    std::vector<AmChunk> chunks;
    am_chunks(units, all, limit, instance_first_k, chunks);
    size_t rec_total = 0, cnt_total = 0, flag_total = 0, pq_words = 0;
    for (AmChunk& c : chunks) {
        const Table& t = *h->tables[c.table];
        c.deferred = t.segments() <= 1;
        const size_t m = c.units.size();
        rec_total += m * c.k;
        cnt_total += m;
        if (c.deferred) { flag_total += m + 16; pq_words += (m + 16) * 4; }      // nq_pad <= m + 15 for every T_q
    }
    if ((rc = h->d_am_rec.ensure(std::max<size_t>(rec_total, 1)))) return rc;
    if ((rc = h->d_am_cnt.ensure(cnt_total + flag_total))) return rc;
    {
        size_t r = 0, c_at = 0, f = cnt_total;
        for (AmChunk& c : chunks) {
            c.d_rec = h->d_am_rec.p + r;
            c.d_cnt = h->d_am_cnt.p + c_at;
            r += c.units.size() * c.k;
            c_at += c.units.size();
            if (c.deferred) { c.flag_off = f - cnt_total; c.d_flags = h->d_am_cnt.p + f; f += c.units.size() + 16; }
        }
    }
    // slots: one per unit, pointing at its list
    std::vector<iskas::Slot> slots(n_units);
    for (uint32_t ci = 0; ci < chunks.size(); ++ci)
        for (uint32_t i = 0; i < chunks[ci].units.size(); ++i) {
            const uint32_t u = chunks[ci].units[i];
            slots[u].rec = reinterpret_cast<const isccsearch_record*>(chunks[ci].d_rec + (size_t)i * chunks[ci].k);
            slots[u].cnt = chunks[ci].d_cnt + i;
            slots[u].k = chunks[ci].k;
            slots[u].type = units[u].type;
        }

    // a chunk searched on its own (the synchronous path): its lists are final on the device when this returns
    auto search_now = [&](AmChunk& c) -> int {
        Batch b(h, *h->tables[c.table], (uint32_t)c.units.size(), c.nbytes, c.k, c.d_rec, c.d_cnt);
        b.radius = c.radius;
        h->stats.searches += 1;
        h->stats.queries += c.units.size();
        int rs;
        if ((rs = b.begin(c.hq.data()))) return rs;
        return b.finish(c.hq.data());
    };
    // (1) tables of several code lengths: the synchronous path, list by list merged on the device
    for (AmChunk& c : chunks) {
        if (c.deferred) continue;
        am_pack(*h->tables[c.table], units, c);
        if ((rc = search_now(c))) return rc;
    }
    // (2) one-segment tables: queued back to back, each with its own slice of the pinned query staging and its own flags
    if (h->ev_staged_pending) { HIPOK(hipEventSynchronize(h->ev_staged)); h->ev_staged_pending = false; }
    if ((rc = h->p_queries.ensure(std::max<size_t>(pq_words, 1)))) return rc;
    // (kernels leave the flags of padding queries, and one-launch searches all of theirs, unwritten)
    if (flag_total) HIPOK(hipMemsetAsync(h->d_am_cnt.p + cnt_total, 0, flag_total * 4, h->stream));
    size_t pq_off = 0;
    for (AmChunk& c : chunks) {
        if (!c.deferred) continue;
        Table& t = *h->tables[c.table];
        am_pack(t, units, c);
        c.batch.reset(new Batch(h, t, (uint32_t)c.units.size(), c.nbytes, c.k, c.d_rec, c.d_cnt));
        Batch& b = *c.batch;
        b.radius = c.radius;
        b.pq_off = pq_off;
        b.d_flags = c.d_flags;
        pq_off += (c.units.size() + 16) * 4;
        h->stats.searches += 1;
        h->stats.queries += c.units.size();
        if ((rc = b.begin(c.hq.data()))) return rc;
    }

    // (3) the scoring, written straight into pinned host memory, and the deferred chunks' overflow flags behind it
    const size_t nr = (size_t)nq * limit;
    const size_t o_keys = 0, o_scores = o_keys + nr * 8, o_types_sc = o_scores + nr * 8, o_count = o_types_sc + nr * n_types * 8;
    // (o_recnt: the first round's list counts again, read back only after a chunk was redone)
    const size_t o_ucnt = o_count + (size_t)nq * 4, o_flags = o_ucnt + (size_t)n_units * 4, o_recnt = o_flags + flag_total * 4;
    const size_t o_types = o_recnt + cnt_total * 4;
    const size_t out_bytes = o_types + nr * n_types;
    if ((rc = h->p_am_out.ensure(out_bytes))) return rc;
    unsigned char* const po = h->p_am_out.p;
    std::vector<uint32_t> offs(unit_offsets, unit_offsets + nq + 1);
    if ((rc = h->d_am_slots.ensure(std::max<uint32_t>(n_units, 1)))) return rc;
    if ((rc = h->d_am_off.ensure(2 * (size_t)nq + 1))) return rc;
    if ((rc = h->d_am_ex.ensure(nq))) return rc;
    if ((rc = h->d_am_hasex.ensure(nq))) return rc;
    if ((rc = h->d_am_tab.ensure(2 * (size_t)iskas::TAB_SIZE))) return rc;
    std::vector<double> tab(score_table, score_table + iskas::TAB_SIZE);
    tab.insert(tab.end(), pow_table, pow_table + iskas::TAB_SIZE);
    if (tab != h->am_tab) {
        HIPOK(hipMemcpy(h->d_am_tab.p, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice));
        h->am_tab.swap(tab);
    }
    if (n_units) HIPOK(hipMemcpyAsync(h->d_am_slots.p, slots.data(), n_units * sizeof(iskas::Slot), hipMemcpyHostToDevice, h->stream));
    HIPOK(hipMemcpyAsync(h->d_am_off.p, offs.data(), offs.size() * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    HIPOK(hipMemcpyAsync(h->d_am_ex.p, exclude, (size_t)nq * 8, hipMemcpyHostToDevice, h->stream));
    HIPOK(hipMemcpyAsync(h->d_am_hasex.p, has_exclude, nq, hipMemcpyHostToDevice, h->stream));
    iskas::Params p{};
    p.slots = h->d_am_slots.p; p.slot_off = h->d_am_off.p; p.qlist = nullptr; p.n_list = nq;
    p.score_tab = h->d_am_tab.p; p.pow_tab = h->d_am_tab.p + iskas::TAB_SIZE;
    p.exclude = h->d_am_ex.p; p.has_exclude = h->d_am_hasex.p;
    p.threshold = threshold; p.compensated = compensated ? 1 : 0; p.limit = limit; p.n_types = n_types;
    // the sort arrays of the listed queries: LDS up to LDS_ITEMS items each, beyond that a global scratch area per block.  The LDS
    // limit above 64 KiB is raised once per handle (one handle = one device), before the first launch that needs it
    uint32_t grid = nq;
    auto size_sort = [&](const std::vector<uint32_t>* qs) -> int {
        uint32_t max_items = 2;
        for (uint32_t i = 0, n_q = qs ? (uint32_t)qs->size() : nq; i < n_q; ++i) {
            const uint32_t q = qs ? (*qs)[i] : i;
            uint64_t n = 0;
            for (uint32_t u = offs[q]; u < offs[q + 1]; ++u) n += slots[u].k;
            max_items = std::max<uint32_t>(max_items, next_pow2((uint32_t)std::max<uint64_t>(n, 2)));
        }
        const uint32_t lds_items = std::min<uint32_t>(iskas::LDS_ITEMS, max_items);
        const size_t lds = iskas::lds_bytes(lds_items);
        if (lds > 65536 && h->am_lds_allowed < lds) {
            HIPOK(iskas::allow_lds(iskas::lds_bytes(iskas::LDS_ITEMS)));
            h->am_lds_allowed = iskas::lds_bytes(iskas::LDS_ITEMS);
        }
        const uint32_t n_list = qs ? (uint32_t)qs->size() : nq;
        grid = max_items > lds_items ? std::min<uint32_t>(n_list, (uint32_t)h->cus) : n_list;
        // (the global scratch stays within SCRATCH_BYTES: fewer blocks, each walking more queries, for the largest sorts --
        //  64 units x limit 4 096 take 8 MiB per block)
        if (max_items > lds_items)
            grid = std::max<uint32_t>(1, std::min<uint64_t>(grid, SCRATCH_BYTES / (2 * (uint64_t)max_items * sizeof(iskas::Item))));
        int rs;
        if (max_items > lds_items && (rs = h->d_am_scratch.ensure((size_t)grid * 2 * max_items))) return rs;
        p.lds_items = lds_items;
        p.scratch = max_items > lds_items ? h->d_am_scratch.p : nullptr;
        p.scratch_items = max_items;
        return 0;
    };
    if ((rc = size_sort(nullptr))) return rc;
    p.out_keys = reinterpret_cast<uint64_t*>(po + o_keys); p.out_scores = reinterpret_cast<double*>(po + o_scores);
    p.out_count = reinterpret_cast<uint32_t*>(po + o_count); p.out_types = po + o_types;
    p.out_type_scores = reinterpret_cast<double*>(po + o_types_sc); p.out_slot_count = reinterpret_cast<uint32_t*>(po + o_ucnt);
    HIPOK(iskas::queue_assets(p, grid, h->stream));
    if (flag_total) HIPOK(hipMemcpyAsync(po + o_flags, h->d_am_cnt.p + cnt_total, flag_total * 4, hipMemcpyDeviceToHost, h->stream));
    HIPOK(hipStreamSynchronize(h->stream));

    // (4) what the first round could not answer: chunks whose candidate lists overflowed (exact again through the synchronous path) and
    // INSTANCE lists that came back full (asked again up to instance_max_k); then the queries they touch are scored again
    const uint32_t* const p_flags = reinterpret_cast<const uint32_t*>(po + o_flags);
    const uint32_t* const p_ucnt = reinterpret_cast<const uint32_t*>(po + o_ucnt);
    std::vector<char> redo_q(nq, 0);
    std::vector<uint32_t> unit_query(n_units);
    for (uint32_t q = 0; q < nq; ++q) for (uint32_t u = offs[q]; u < offs[q + 1]; ++u) unit_query[u] = q;
    bool again = false;
    for (AmChunk& c : chunks) {
        if (!c.deferred || !c.batch || c.batch->jobs.empty()) continue;
        bool flagged = false;
        for (size_t i = 0; i < c.units.size() && !flagged; ++i) flagged = p_flags[c.flag_off + i] != 0;     // (one job: one segment)
        if (!flagged) continue;
        if ((rc = search_now(c))) return rc;
        for (uint32_t u : c.units) redo_q[unit_query[u]] = 1;
        again = true;
    }
    // the redone chunks' counts live on the device only: ONE copy of all first-round counts brings them
    const uint32_t* const p_recnt = reinterpret_cast<const uint32_t*>(po + o_recnt);
    if (again) {
        HIPOK(hipMemcpyAsync(po + o_recnt, h->d_am_cnt.p, cnt_total * 4, hipMemcpyDeviceToHost, h->stream));
        HIPOK(hipStreamSynchronize(h->stream));
    }
    std::vector<uint32_t> full;
    if (instance_max_k > instance_first_k)
        for (uint32_t u = 0; u < n_units; ++u)
            if (units[u].max_hamming >= 0) {
                const uint32_t cnt = again ? p_recnt[slots[u].cnt - h->d_am_cnt.p] : p_ucnt[u];
                if (cnt >= instance_first_k) full.push_back(u);
            }
    if (!full.empty()) {
        std::vector<AmChunk> second;
        am_chunks(units, full, limit, instance_max_k, second);
        size_t r2 = 0;
        for (AmChunk& c : second) r2 += c.units.size() * (size_t)c.k;
        if ((rc = h->d_am_rec2.ensure(r2))) return rc;
        if ((rc = h->d_am_cnt2.ensure(full.size()))) return rc;
        size_t r = 0, ci = 0;
        for (AmChunk& c : second) {
            c.d_rec = h->d_am_rec2.p + r;
            c.d_cnt = h->d_am_cnt2.p + ci;
            r += c.units.size() * (size_t)c.k;
            ci += c.units.size();
            am_pack(*h->tables[c.table], units, c);
            if ((rc = search_now(c))) return rc;
            for (uint32_t i = 0; i < c.units.size(); ++i) {
                const uint32_t u = c.units[i];
                slots[u].rec = reinterpret_cast<const isccsearch_record*>(c.d_rec + (size_t)i * c.k);
                slots[u].cnt = c.d_cnt + i;
                slots[u].k = c.k;
                redo_q[unit_query[u]] = 1;
            }
        }
        HIPOK(hipMemcpyAsync(h->d_am_slots.p, slots.data(), n_units * sizeof(iskas::Slot), hipMemcpyHostToDevice, h->stream));
        again = true;
    }
    if (again) {
        std::vector<uint32_t> qlist;
        for (uint32_t q = 0; q < nq; ++q) if (redo_q[q]) qlist.push_back(q);
        HIPOK(hipMemcpyAsync(h->d_am_off.p + nq + 1, qlist.data(), qlist.size() * 4, hipMemcpyHostToDevice, h->stream));
        p.qlist = h->d_am_off.p + nq + 1;
        p.n_list = (uint32_t)qlist.size();
        if ((rc = size_sort(&qlist))) return rc;
        HIPOK(iskas::queue_assets(p, grid, h->stream));
        HIPOK(hipStreamSynchronize(h->stream));
    }

    // (5) the caller's arrays
    memcpy(out_keys, po + o_keys, nr * 8);
    memcpy(out_scores, po + o_scores, nr * 8);
    memcpy(out_count, po + o_count, (size_t)nq * 4);
    memcpy(out_types, po + o_types, nr * n_types);
    memcpy(out_type_scores, po + o_types_sc, nr * n_types * 8);
    memcpy(out_unit_count, po + o_ucnt, (size_t)n_units * 4);
    return 0;
}

extern "C" {

static int search_device_impl(isccsearch_handle* h, uint32_t table, uint32_t nq, const uint64_t* q_words,
                              const uint8_t* q_nbytes, uint32_t k, int radius, void* d_records, uint32_t* d_counts) {
    if (!h) return fail(-EINVAL, "handle is NULL");
    if (k < 1) return fail(-EINVAL, "`count` must be >= 1");
    if (k > ISCCSEARCH_MAX_K) return fail(-EINVAL, "count %u exceeds ISCCSEARCH_MAX_K (%d)", k, ISCCSEARCH_MAX_K);
    if (radius > 256) return fail(-EINVAL, "max_hamming %d exceeds 256", radius);
    if (nq == 0) return 0;
    if (!q_words || !d_records || !d_counts) return fail(-EINVAL, "NULL argument");
    std::lock_guard<std::mutex> lk(h->mu);
    Table* tp;
    int rc = get_table(h, table, tp);
    if (rc) return rc;
    Table& t = *tp;
    if ((rc = check_query_lengths(t, nq, q_nbytes))) return rc;
    uint32_t len = (uint32_t)t.max_bytes;
    if (t.metric == ISCCSEARCH_METRIC_NPHD) {
        len = q_nbytes[0];
        for (uint32_t q = 1; q < nq; ++q)
            if (q_nbytes[q] != len) return fail(-EINVAL, "search_device needs queries of one byte length (query %u differs)", q);
    }
    HIPOK(hipSetDevice(h->device));
    h->stats.searches += 1;
    h->stats.queries += nq;
    isk::Record* out = static_cast<isk::Record*>(d_records);
    for (uint32_t pos = 0; pos < nq; pos += QB_MAX) {
        const uint32_t m = std::min<uint32_t>(QB_MAX, nq - pos);
        Batch batch(h, t, m, len, k, out + (size_t)pos * k, d_counts + pos);
        batch.radius = radius;
        const uint64_t* const hq = q_words + (size_t)pos * t.max_words;
        if ((rc = batch.begin(hq))) return rc;
        if ((rc = batch.finish(hq))) return rc;
    }
    HIPOK(hipStreamSynchronize(h->stream));
    return 0;
}

int isccsearch_search_device(isccsearch_handle* h, uint32_t table, uint32_t nq, const uint64_t* q_words,
                             const uint8_t* q_nbytes, uint32_t k, void* d_records, uint32_t* d_counts) {
    return search_device_impl(h, table, nq, q_words, q_nbytes, k, -1, d_records, d_counts);
}

int isccsearch_search_within_device(isccsearch_handle* h, uint32_t table, uint32_t nq, const uint64_t* q_words,
                                    const uint8_t* q_nbytes, uint32_t k, uint32_t max_hamming,
                                    void* d_records, uint32_t* d_counts) {
    if (max_hamming > 256) return fail(-EINVAL, "max_hamming %u exceeds 256", max_hamming);
    return search_device_impl(h, table, nq, q_words, q_nbytes, k, (int)max_hamming, d_records, d_counts);
}

static int merge_device_impl(isccsearch_handle* h, uint32_t n_lists, uint32_t nq, uint32_t k, int key_words,
                             const void* d_records, const void* d_counts, uint64_t list_stride, uint64_t count_stride,
                             void* producer_stream, bool ordered,
                             uint64_t* out_keys, uint32_t* out_hamming, uint16_t* out_prefix_bits, uint32_t* out_count) {
    if (!h) return fail(-EINVAL, "handle is NULL");
    if (nq == 0) return 0;
    if (n_lists < 1 || k < 1 || k > ISCCSEARCH_MAX_K || (key_words != 1 && key_words != 2)) return fail(-EINVAL, "bad arguments");
    if (!d_records || !d_counts || !out_keys || !out_hamming || !out_prefix_bits || !out_count) return fail(-EINVAL, "NULL argument");
    std::lock_guard<std::mutex> lk(h->mu);
    HIPOK(hipSetDevice(h->device));
    int rc;
    if (list_stride % 8 || count_stride % 4 || (uintptr_t)d_records % 8 || (uintptr_t)d_counts % 4) return fail(-EINVAL, "misaligned record/count blocks");
    if (ordered) {
        // the gathered blocks are produced on the caller's stream: order the merge behind it without a host round-trip
        // (a caller that issued them on the library's own stream -- isccsearch_stream -- is ordered already)
        if (static_cast<hipStream_t>(producer_stream) != h->stream) {
            HIPOK(hipEventRecord(h->ev_producer, static_cast<hipStream_t>(producer_stream)));
            HIPOK(hipStreamWaitEvent(h->stream, h->ev_producer, 0));
        }
    }
    // The merge writes its {records | counts} straight into ONE pinned host block (page-locked memory is mapped into the
    // device's address space): 240 bytes per query cross PCIe as the kernel's own stores, and the host needs a single
    // synchronisation -- no device->host copies to launch (each cost ~25 us of queue hand-over after the kernel).
    // (Blocks above DIRECT_RESULT_BYTES -- large k x many queries -- go through device memory and two DMA copies as before.)
    const size_t rec_bytes = (size_t)nq * k * sizeof(isk::Record);
    const bool direct = rec_bytes + (size_t)nq * sizeof(uint32_t) <= DIRECT_RESULT_BYTES;
    if ((rc = h->p_block.ensure(rec_bytes + (size_t)nq * sizeof(uint32_t)))) return rc;
    if (!direct) {
        if ((rc = h->d_final.ensure((size_t)nq * k))) return rc;
        if ((rc = h->d_outcnt.ensure(nq))) return rc;
    }
    isk::MergeParams mp{static_cast<const unsigned char*>(d_records), static_cast<const unsigned char*>(d_counts),
                        list_stride, count_stride,
                        direct ? reinterpret_cast<isk::Record*>(h->p_block.p) : h->d_final.p,
                        direct ? reinterpret_cast<uint32_t*>(h->p_block.p + rec_bytes) : h->d_outcnt.p, n_lists, nq, k};
    hipLaunchKernelGGL(isk::merge_kernel, dim3(nq), dim3(isk::BLOCK), 0, h->stream, mp);
    HIPOK(hipGetLastError());
    if (!direct) {
        HIPOK(hipMemcpyAsync(h->p_block.p, h->d_final.p, rec_bytes, hipMemcpyDeviceToHost, h->stream));
        HIPOK(hipMemcpyAsync(h->p_block.p + rec_bytes, h->d_outcnt.p, nq * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    }
    HIPOK(hipStreamSynchronize(h->stream));
    unpack_records(reinterpret_cast<const isk::Record*>(h->p_block.p), reinterpret_cast<const uint32_t*>(h->p_block.p + rec_bytes), nq, k, key_words,
                   nullptr, out_keys, out_hamming, out_prefix_bits, out_count);
    return 0;
}

int isccsearch_merge_device(isccsearch_handle* h, uint32_t n_lists, uint32_t nq, uint32_t k, int key_words,
                            const void* d_records, const void* d_counts, uint64_t list_stride, uint64_t count_stride,
                            uint64_t* out_keys, uint32_t* out_hamming, uint16_t* out_prefix_bits, uint32_t* out_count) {
    return merge_device_impl(h, n_lists, nq, k, key_words, d_records, d_counts, list_stride, count_stride, nullptr, false,
                             out_keys, out_hamming, out_prefix_bits, out_count);
}

int isccsearch_merge_device_after(isccsearch_handle* h, uint32_t n_lists, uint32_t nq, uint32_t k, int key_words,
                                  const void* d_records, const void* d_counts, uint64_t list_stride, uint64_t count_stride,
                                  void* producer_stream,
                                  uint64_t* out_keys, uint32_t* out_hamming, uint16_t* out_prefix_bits, uint32_t* out_count) {
    return merge_device_impl(h, n_lists, nq, k, key_words, d_records, d_counts, list_stride, count_stride, producer_stream, true,
                             out_keys, out_hamming, out_prefix_bits, out_count);
}

// Several merges behind ONE synchronisation: the per-unit searches of one request on a sharded index share one all-gather
// (sharded.py, ShardedTable.search_many); their merges are queued back to back into distinct parts of the pinned result block
// and read after a single hipStreamSynchronize (each merge_device_after call costs one: ~50 us per unit).
int isccsearch_merge_many_after(isccsearch_handle* h, uint32_t n, isccsearch_merge_request* reqs, void* producer_stream) {
    if (!h) return fail(-EINVAL, "handle is NULL");
    if (n == 0) return 0;
    if (!reqs) return fail(-EINVAL, "NULL argument");
    size_t total = 0;
    std::vector<size_t> off(n);
    for (uint32_t i = 0; i < n; ++i) {
        isccsearch_merge_request& r = reqs[i];
        if (r.nq == 0 || r.n_lists < 1 || r.k < 1 || r.k > ISCCSEARCH_MAX_K || (r.key_words != 1 && r.key_words != 2)) return fail(-EINVAL, "bad arguments (merge %u)", i);
        if (!r.d_records || !r.d_counts || !r.out_keys || !r.out_hamming || !r.out_prefix_bits || !r.out_count) return fail(-EINVAL, "NULL argument (merge %u)", i);
        if (r.list_stride % 8 || r.count_stride % 4 || (uintptr_t)r.d_records % 8 || (uintptr_t)r.d_counts % 4) return fail(-EINVAL, "misaligned record/count blocks (merge %u)", i);
        off[i] = total;
        total += ((size_t)r.nq * r.k * sizeof(isk::Record) + (size_t)r.nq * sizeof(uint32_t) + 15) & ~(size_t)15;
    }
    std::lock_guard<std::mutex> lk(h->mu);
    HIPOK(hipSetDevice(h->device));
    int rc;
    // the kernels write their {records | counts} straight into the pinned block (mapped into the device's address space); a request
    // whose results do not fit the direct budget goes through the ordinary call
    if (total > DIRECT_RESULT_BYTES) return fail(-E2BIG, "merge_many: %zu bytes of results exceed the directly written block", total);
    if ((rc = h->p_block.ensure(total))) return rc;
    if (static_cast<hipStream_t>(producer_stream) != h->stream) {
        HIPOK(hipEventRecord(h->ev_producer, static_cast<hipStream_t>(producer_stream)));
        HIPOK(hipStreamWaitEvent(h->stream, h->ev_producer, 0));
    }
    for (uint32_t i = 0; i < n; ++i) {
        isccsearch_merge_request& r = reqs[i];
        const size_t rec_bytes = (size_t)r.nq * r.k * sizeof(isk::Record);
        isk::MergeParams mp{static_cast<const unsigned char*>(r.d_records), static_cast<const unsigned char*>(r.d_counts), r.list_stride, r.count_stride,
                            reinterpret_cast<isk::Record*>(h->p_block.p + off[i]), reinterpret_cast<uint32_t*>(h->p_block.p + off[i] + rec_bytes), r.n_lists, r.nq, r.k};
        hipLaunchKernelGGL(isk::merge_kernel, dim3(r.nq), dim3(isk::BLOCK), 0, h->stream, mp);
    }
    HIPOK(hipGetLastError());
    HIPOK(hipStreamSynchronize(h->stream));
    for (uint32_t i = 0; i < n; ++i) {
        isccsearch_merge_request& r = reqs[i];
        const size_t rec_bytes = (size_t)r.nq * r.k * sizeof(isk::Record);
        unpack_records(reinterpret_cast<const isk::Record*>(h->p_block.p + off[i]), reinterpret_cast<const uint32_t*>(h->p_block.p + off[i] + rec_bytes), r.nq, r.k, r.key_words,
                       nullptr, r.out_keys, r.out_hamming, r.out_prefix_bits, r.out_count);
    }
    return 0;
}

int isccsearch_search_device_async(isccsearch_handle* h, uint32_t table, uint32_t nq, const uint64_t* q_words,
                                   const uint8_t* q_nbytes, uint32_t k, int32_t max_hamming,
                                   void* d_records, uint32_t* d_counts, void* consumer_stream) {
    if (!h) return fail(-EINVAL, "handle is NULL");
    if (max_hamming > 256) return fail(-EINVAL, "max_hamming %d exceeds 256", max_hamming);
    const int radius = max_hamming < 0 ? -1 : max_hamming;
    bool async = nq > 0 && nq <= QB_MAX && k >= 1 && k <= ISCCSEARCH_MAX_K && q_words && d_records && d_counts;
    // the one-shot hint belongs to THIS call whatever becomes of it: read and clear it before anything can return (an early
    // return used to leave it armed for the next, unrelated call, whose caller would not verify its lists)
    int hint;
    {
        std::lock_guard<std::mutex> lk(h->mu);
        hint = h->device_search_hint;
        h->device_search_hint = -1;
    }
    if (async) {
        std::lock_guard<std::mutex> lk(h->mu);
        Table* tp;
        int rc = get_table(h, table, tp);
        if (rc) return rc;
        Table& t = *tp;
        if ((rc = check_query_lengths(t, nq, q_nbytes))) return rc;
        uint32_t len = (uint32_t)t.max_bytes;
        if (t.metric == ISCCSEARCH_METRIC_NPHD) {
            len = q_nbytes[0];
            for (uint32_t q = 1; q < nq; ++q)
                if (q_nbytes[q] != len) return fail(-EINVAL, "search_device needs queries of one byte length (query %u differs)", q);
        }
        if (t.segments() <= 1) {
            HIPOK(hipSetDevice(h->device));
            h->stats.searches += 1;
            h->stats.queries += nq;
            Batch batch(h, t, nq, len, k, static_cast<isk::Record*>(d_records), d_counts);
            batch.radius = radius;
            batch.mark_overflow = true;
            // (sharded callers: the GLOBAL k-th distance of the previous step + margin -- every shard then lists its rows under it,
            //  tightening as it finds k of its own, and the caller accepts the merged lists only if they hold k rows per query)
            // ... a SMALL batch (the protocol's per-unit searches on a sharded index) takes the hint as the radius of one range-limited
            // pass -- radius_init + collect + select instead of bootstrap + levels + picks + collect -- as search_locked's speculative
            // pass does on one GPU; same contract: the table's nearest rows within the hint, fewer than k if it was too tight
            if (radius < 0 && hint >= 0) {
                if (h->speculate && nq <= h->spec_max_queries) batch.radius = hint;
                else batch.self_hint = hint;
            }
            if ((rc = batch.begin(q_words))) return rc;
            if (static_cast<hipStream_t>(consumer_stream) != h->stream) {
                HIPOK(hipEventRecord(h->ev_done, h->stream));
                HIPOK(hipStreamWaitEvent(static_cast<hipStream_t>(consumer_stream), h->ev_done, 0));
            }
            return 0;
        }
    }
    // several segments (their lists must be fixed and merged with the host's help), oversized batches, bad arguments: the
    // synchronous path does the work and the reporting; the results are complete when it returns
    return search_device_impl(h, table, nq, q_words, q_nbytes, k, radius, d_records, d_counts);
}

}  // extern "C"
