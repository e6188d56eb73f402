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
// search is the final result copy (one block, laid out by ResultBlock below); search_many shares it between
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
// A batch of m queries is padded to whole passes of T_q = 8 or 16 queries: nq_pad <= m + 15.  Whoever sizes a batch's overflow flags or
// its slice of the pinned query staging before the batch exists takes m + 16 flag slots, and four staged words for each of them
constexpr size_t flag_slots_for(size_t m) { return m + 16; }
constexpr size_t staged_words_for(size_t m) { return (m + 16) * 4; }
// One batch's results as ONE block {records [m][k] | counts [m] | flags [m + 16] | extra [m] | info}, the same on the device and in its pinned
// mirror.  records: not when the lists stay on the device (a scoring sink); extra: the lists' lengths of a counted document-frequency call, or
// the k-th distances of a sink; info: the scoring kernels' info words.  A merge of device-resident lists writes {records | counts} only.
struct ResultBlock {
    size_t m, k;
    bool with_records = true, with_extra = false, with_info = false, with_flags = true;
    static constexpr ResultBlock merged(size_t m, size_t k) { return ResultBlock{m, k, true, false, false, false}; }
    constexpr size_t records_bytes() const { return with_records ? m * k * sizeof(isk::Record) : 0; }
    constexpr size_t counts_off() const { return records_bytes(); }
    constexpr size_t flags_off() const { return counts_off() + m * sizeof(uint32_t); }
    constexpr size_t extra_off() const { return flags_off() + (with_flags ? flag_slots_for(m) : 0) * sizeof(uint32_t); }
    constexpr size_t info_off() const { return extra_off() + (with_extra ? m : 0) * sizeof(uint32_t); }
    constexpr size_t bytes() const { return info_off() + (with_info ? isksp::INFO_WORDS : 0) * sizeof(uint32_t); }
    constexpr size_t slice_bytes() const { return (bytes() + 15) & ~(size_t)15; }      // (blocks queued back to back in one buffer)
    // {records | counts | the flag words a begun batch really has}: what the copy of a batch's lists moves
    constexpr size_t bytes_with(size_t flag_words) const { return flags_off() + flag_words * sizeof(uint32_t); }
    static uint32_t* words(unsigned char* base, size_t off) { return reinterpret_cast<uint32_t*>(base + off); }
    isk::Record* records(unsigned char* base) const { return reinterpret_cast<isk::Record*>(base); }
    uint32_t* counts(unsigned char* base) const { return words(base, counts_off()); }
    uint32_t* flags(unsigned char* base) const { return words(base, flags_off()); }
    uint32_t* extra(unsigned char* base) const { return words(base, extra_off()); }
    uint32_t* info(unsigned char* base) const { return words(base, info_off()); }
};
constexpr size_t RB_REC = sizeof(isk::Record), RB_W = sizeof(uint32_t);
static_assert(ResultBlock{1, 1}.counts_off() == 1 * 1 * RB_REC && ResultBlock{1, 1}.flags_off() == 1 * 1 * RB_REC + 1 * RB_W &&
              ResultBlock{1, 1}.bytes() == 1 * 1 * RB_REC + (1 + (1 + 16)) * RB_W, "one query, one record");
constexpr ResultBlock RB_SINK{5, 3, false, true, true};
static_assert(RB_SINK.counts_off() == 0 && RB_SINK.flags_off() == 5 * RB_W && RB_SINK.extra_off() == (5 + (5 + 16)) * RB_W &&
              RB_SINK.info_off() == (5 + (5 + 16) + 5) * RB_W && RB_SINK.bytes() == (5 + (5 + 16) + 5 + isksp::INFO_WORDS) * RB_W, "a sink's block");
static_assert(ResultBlock{1024, 10}.counts_off() == 1024 * 10 * RB_REC && ResultBlock{1024, 10}.bytes() == 1024 * 10 * RB_REC + (1024 + (1024 + 16)) * RB_W &&
              ResultBlock{1024, 10}.bytes_with(1024) == 1024 * 10 * RB_REC + (1024 + 1024) * RB_W, "a full batch of lists");
static_assert(ResultBlock{1, 2}.bytes() == 120 && ResultBlock{1, 2}.slice_bytes() == ((1 * 2 * RB_REC + (1 + (1 + 16)) * RB_W + 15) & ~(size_t)15) &&
              ResultBlock::merged(3, 1).slice_bytes() == ((3 * 1 * RB_REC + 3 * RB_W + 15) & ~(size_t)15) && ResultBlock::merged(3, 1).slice_bytes() == 96, "slices of 16 bytes");
constexpr uint64_t CACHE_STRETCH_BYTES = 128ull << 20;   // half of the 256 MiB Infinity Cache
constexpr uint64_t ROW_ALIGN = 2048;     // column capacities are multiples of the largest tile

// Scratch memory that grows on demand and frees itself with its owner: device memory (DevBuf), or page-locked host memory (PinBuf),
// with which async copies really are asynchronous
template <typename T, bool PINNED>
struct ScratchBuf {
    T* p = nullptr;
    size_t n = 0;
    ScratchBuf() = default;
    ScratchBuf(const ScratchBuf&) = delete;
    ScratchBuf& operator=(const ScratchBuf&) = delete;
    ~ScratchBuf() { release(); }
    int ensure(size_t need) {
        if (need <= n) return 0;
        release();
        const size_t want = need + need / 4 + (PINNED ? 16 : 0);
        const hipError_t e = PINNED ? hipHostMalloc((void**)&p, want * sizeof(T), hipHostMallocDefault) : hipMalloc((void**)&p, want * sizeof(T));
        if (e != hipSuccess) { p = nullptr; (void)hipGetLastError(); return fail(-ENOMEM, "%s(%zu bytes) failed: %s", PINNED ? "hipHostMalloc" : "hipMalloc", want * sizeof(T), hipGetErrorString(e)); }
        n = want;
        return 0;
    }
    void release() { if (p) (void)(PINNED ? hipHostFree(p) : hipFree(p)); p = nullptr; n = 0; }
};
template <typename T> using DevBuf = ScratchBuf<T, false>;
template <typename T> using PinBuf = ScratchBuf<T, true>;

constexpr size_t DIRECT_RESULT_BYTES = 1 << 20;   // result blocks up to this size are written by the kernels straight into pinned host memory

uint64_t mask_for(uint32_t pbytes) {   // mask of the last compared word for a prefix of pbytes bytes
    const uint32_t rem = pbytes & 7;
    return rem ? ~0ULL << (8 * (8 - rem)) : ~0ULL;
}
uint32_t next_pow2(uint32_t v) { uint32_t p = 2; while (p < v) p <<= 1; return p; }
// the first W word columns of a segment into a kernel's parameter block
template <typename T>
void set_cols(T (&dst)[4], const Segment& s, uint32_t W) { for (uint32_t w = 0; w < W; ++w) dst[w] = s.col[w]; }
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

// ------------------------------------------------------------------------------------------
// options
// ------------------------------------------------------------------------------------------
// Selections whose A/B is settled and that no workload sets: constants at the value they were measured to
constexpr uint32_t BLOCKS_PER_CU = 8;      // scan grid = CUs x this (per query group)
constexpr uint64_t BOOT_ROWS = 65536;      // rows of the threshold bootstrap of the level design (4 096 exact + the rest counted under that
                                           // cut; wide blocks for small batches): one level launch + pick less than with 4 096 rows
                                           // (100 M x 64-bit: 8 queries 0.231 against 0.252 ms, 4 queries at k = 100 0.286 against 0.354)
constexpr uint64_t LEVEL_GROWTH = 8;       // each threshold level streams this many times the rows seen so far
constexpr uint64_t MFMA_LEVEL_GROWTH = 4;  // ... when the scan runs on the matrix cores (k <= 64): 4 / 6 / 8 measured 295.5 / 295.9 / 290.4 k q/s at 100 M rows and 1.35 / 1.28 / 1.27 M at 12.5 M
constexpr uint32_t FOLD_TAU = 11;          // 64-bit codes: groups whose thresholds are all <= this take the folded fast path of scan_adapt_kernel
constexpr uint32_t MFMA_PACK_MIN_QUERIES = 9;    // 64-bit codes (packed matrix-core kernel): from this many queries (see use_mfma)
constexpr uint64_t MFMA_FEW_ROWS = 12ull << 20;  // longer codes: segments up to this many rows take the matrix cores from MFMA_PACK_MIN_QUERIES queries too
constexpr uint32_t SELF_REFRESH_STEPS = 1;       // the single pass: steps of a full chunk between two looks at the live thresholds (power of two)
// The fixed-radius pass of large pack3 batches (search_locked, Spec::tight; option "radius_batches"): its radius is the hint minus the hint's
// margin -- the worst k-th distance the class last ended at -- plus this many bits, and up to RADIUS_BATCH_MAX_REPAIRS queries (one query
// group) that come up short are asked again under the whole hint (a pass for 9-32 queries: 0.19 ms, profiles/r04_operating_points.txt)
// (0 against 1 on the flagship step, 100 M x 64-bit rows, 1 024 queries, k = 10, three runs each alternating: 533.6 against 514.8 k
//  queries/s, scan 1.837 against 1.912 ms per step -- 59 against 224 appended rows per query, and 0.6 queries per step to repair against
//  none: the second small pass costs less than the wider radius does on every step.  profiles/radius_batches_ab.txt)
constexpr int RADIUS_BATCH_SLACK = 0;
constexpr uint32_t RADIUS_BATCH_MAX_REPAIRS = 32;
// Every k takes the single self-tightening pass (it stopped at 512 until the pass was measured beyond it: k = 1 000 / 2 000 over 100 M rows
// 6.0 / 9.0 ms against 8.5 / 14.0 of the level design, 4.2 / 6.6 under a hint; the unpruned lists hold ~k ln(n / sample) entries + the
// first steps' flood: see the cap in Batch::begin.  100 M rows, k = 100 / 256 / 512: 3.80 / 4.52 / 6.04 ms against 4.60 / 5.35 / 7.37 with levels).
// The collect pass re-derives the threshold after every stretch but the last, and large batches bootstrap with boot_multi_kernel
// (four queries per block share the sample's row loads).

// What a caller can set and read by name; every value an int64_t, the defaults here
struct Options {
    int64_t queries_per_pass = 8;     // queries per streaming pass: 8 keeps the scan HBM-bound
    int64_t profile = 0;
    int64_t count_candidates = 0;     // read the candidate counters back after every batch (one more copy + synchronisation: accounting runs only)
    int64_t tiny_rows = 16384;        // segments of at most this many rows are answered by ONE launch (tiny_search_kernel); 0: never
    int64_t select_wide_from = 2048;  // sort buffers of at least this many slots are selected by 1 024-thread blocks (0xFFFFFFFF: never)
    int64_t stretch_mb = CACHE_STRETCH_BYTES >> 20;   // MB of rows per collect launch when several query groups share them (0: one pass)
    int64_t mfma_stretch_factor = 3;  // ... times this on the matrix cores, when several CHUNKS of queries share them
    // large batches: the scan as an FP4 matrix-core contraction (mfma_scan.hip) instead of XOR + popcount on the VALU
    int64_t mfma = 1;
    int64_t mfma_min_queries = 17;    // batches below this stay on the XOR + popcount kernel, HBM-bound up to ~11 queries per pass
                                      // (100 M x 64-bit: 32 queries 0.49 ms against 0.71 ms, 24 queries 0.48 against 0.63; at 16 both take 0.47 ms)
    int64_t mfma_min_rows = 65536;    // launches over fewer rows do not amortise the per-block query expansion
    int64_t mfma_pack = 1;            // 64-bit codes on the matrix cores: two row tiles per accumulator, packed f16 fold (mfma_pack_kernel)
    int64_t mfma_pack3 = 1;           // ... chunks of more than four query groups: three row tiles per accumulator, OR fold (mfma_pack3_kernel); 0: mfma_pack_kernel
    // the joins (join_api.hip.h) on the matrix cores too: mfma_join_kernel instead of join_scan_kernel.  Self-join of 1 Mi rows, A B A in
    // one run: 4.47x the XOR + popcount kernel's pair distances/s for 64-bit rows, 5.01x for 256-bit rows (profiles/join_mfma_rate.txt)
    int64_t join_mfma = 1;
    // ... launches whose two segments both hold at least this many rows (0: every launch).  65 536: the smallest of 16 Ki / 64 Ki / 256 Ki
    // rows at which the matrix cores are not slower for both widths -- matrix cores / VALU at those sizes 0.61 / 1.83 / 3.22 for 64-bit
    // rows and 1.53 / 2.79 / 3.87 for 256-bit rows (same file)
    int64_t join_mfma_min_rows = 65536;
    // on the matrix cores: ONE pass whose thresholds tighten themselves (MODE_SELF) instead of levels + picks --
    // every launch of that chain costs ~35 us of ramp, prologue and tail, and a step of 100 M rows had seven of them
    int64_t self_tighten = 1;
    int64_t self_boot_rows = 65536;   // its bootstrap sample: all waves start under the sample's threshold at once, so a
                                      // short sample floods the first steps with candidates (4 096 rows: ~860 per query)
    int64_t self_boot_per_k = 1024;   // ... and at least this many rows per wanted neighbour
    int64_t self_hint = 1;            // batches above spec_max_queries: start the single self-tightening pass under the hint (no bootstrap sample)
    int64_t radius_batches = 1;       // ... those that would run mfma_pack3_kernel: ONE fixed-radius pass under the hint's worst k-th distance, the
                                      // few queries it leaves short asked again under the hint (search_locked, Spec::tight); 0: the hinted single pass
    int64_t speculate = 1;            // small batches: try one range-limited pass under the previous search's k-th distance first
    int64_t spec_max_queries = 128;   // ... batches of up to this many queries
    int64_t device_search_hint = -1;  // one-shot: the next isccsearch_search_device_async starts its single pass under this threshold (the caller verifies)
    int64_t candidate_cap = 16384;    // floor of the per-query candidate buffer (entries); tests shrink it to reach the overflow paths
};

// name -> field and the values it takes (queries_per_pass: 8 or 16 only, see isccsearch_set_option)
struct OptionDesc { const char* name; int64_t Options::* field; int64_t min, max; };
constexpr int64_t NO_MAX = INT64_MAX;
const OptionDesc OPTIONS[] = {
    {"queries_per_pass", &Options::queries_per_pass, 8, 16},
    {"profile", &Options::profile, 0, 1},
    {"count_candidates", &Options::count_candidates, 0, 1},
    {"tiny_rows", &Options::tiny_rows, 0, 1 << 20},
    {"select_wide_from", &Options::select_wide_from, 0, 0xFFFFFFFFll},
    {"stretch_mb", &Options::stretch_mb, 0, 65536},
    {"mfma_stretch_factor", &Options::mfma_stretch_factor, 1, 64},
    {"mfma", &Options::mfma, 0, 1},
    {"mfma_min_queries", &Options::mfma_min_queries, 1, 1024},
    {"mfma_min_rows", &Options::mfma_min_rows, 1, NO_MAX},
    {"join_mfma", &Options::join_mfma, 0, 1},
    {"join_mfma_min_rows", &Options::join_mfma_min_rows, 0, NO_MAX},
    {"mfma_pack", &Options::mfma_pack, 0, 1},
    {"mfma_pack3", &Options::mfma_pack3, 0, 1},
    {"self_tighten", &Options::self_tighten, 0, 1},
    {"self_boot_rows", &Options::self_boot_rows, 256, 1 << 20},
    {"self_boot_per_k", &Options::self_boot_per_k, 0, 1 << 20},
    {"self_hint", &Options::self_hint, 0, 1},
    {"radius_batches", &Options::radius_batches, 0, 1},
    {"speculate", &Options::speculate, 0, 1},
    {"spec_max_queries", &Options::spec_max_queries, 0, 1024},
    {"device_search_hint", &Options::device_search_hint, -1, 8 * ISCCSEARCH_MAX_BYTES},
    {"candidate_cap", &Options::candidate_cap, 64, 1 << 22},
};
const OptionDesc* find_option(const char* name) {
    for (const OptionDesc& d : OPTIONS)
        if (!strcmp(d.name, name)) return &d;
    return nullptr;
}

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
    Options opt;                      // what isccsearch_set_option / isccsearch_get_option reach (OPTIONS)
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
    // one batch's results as ONE block (ResultBlock): a single device->host copy
    DevBuf<unsigned char> d_block;
    PinBuf<unsigned char> p_block;
    DevBuf<uint64_t> d_misc;        // moves / gather rows / single query
    DevBuf<uint64_t> d_misc2;
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
    // isccsearch_join_components: the caller's live keys and their labels, a label per row (segment by segment), the union-find array
    DevBuf<uint64_t> d_join_live_keys;
    DevBuf<uint32_t> d_join_live_labels, d_join_row_labels, d_join_parent;
    size_t am_lds_allowed = 0;                   // dynamic LDS the scoring kernel was allowed on this handle's device
    // asynchronous device searches: "results ready" for the consumer stream, "query upload done" for the pinned staging
    hipEvent_t ev_done = nullptr, ev_staged = nullptr, ev_producer = nullptr;
    bool ev_staged_pending = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pool;
    std::vector<char> ev_level;      // per used pair: 1 = a threshold-level launch, 0 = a collect launch
    size_t ev_used = 0;
    isccsearch_stats stats{};
    // What isccsearch_destroy runs under the handle's lock; the destructor runs it too, for a handle that isccsearch_create gives up
    // half-made (after destroy it finds nothing left but to make the device current).  The scratch buffers above are freed AFTER it, by
    // their own destructors: behind the synchronised and destroyed stream, outside the lock, with the device still current.
    void teardown() {
        (void)hipSetDevice(device);
        if (stream) (void)hipStreamSynchronize(stream);
        for (auto& t : tables)
            if (t) for (auto& s : t->seg) seg_free(s);
        tables.clear();
        if (d_rank) { (void)hipFree(d_rank); d_rank = nullptr; }
        for (auto& ev : ev_pool) { (void)hipEventDestroy(ev.first); (void)hipEventDestroy(ev.second); }
        ev_pool.clear();
        for (hipEvent_t* e : {&ev_done, &ev_staged, &ev_producer}) { if (*e) (void)hipEventDestroy(*e); *e = nullptr; }
        if (stream) { (void)hipStreamDestroy(stream); stream = nullptr; }
    }
    ~isccsearch_handle() { teardown(); }
};

namespace {

using H = isccsearch_handle;


// ------------------------------------------------------------------------------------------
// kernel dispatch
// ------------------------------------------------------------------------------------------
// only the non-temporal variant of scan_kernel (its last template argument) is instantiated: plain loads measured no faster
//  and every extra variant costs build time
template <int W, bool MASK, int TQ>
void launch_scan_mode(int mode, dim3 grid, hipStream_t st, const isk::ScanParams& p) {
    if (mode == isk::MODE_COLLECT) hipLaunchKernelGGL((isk::scan_kernel<W, MASK, TQ, isk::MODE_COLLECT>), grid, dim3(isk::BLOCK), 0, st, p);
    else if (mode == isk::MODE_STRETCH) hipLaunchKernelGGL((isk::scan_kernel<W, MASK, TQ, isk::MODE_STRETCH>), grid, dim3(isk::BLOCK), 0, st, p);
    else hipLaunchKernelGGL((isk::scan_kernel<W, MASK, TQ, isk::MODE_BOTH>), grid, dim3(isk::BLOCK), 0, st, p);
}
template <int W, bool MASK>
void launch_scan_tq(int tq, int mode, dim3 grid, hipStream_t st, const isk::ScanParams& p) {
    switch (tq) {
        case 8: launch_scan_mode<W, MASK, 8>(mode, grid, st, p); break;
        default: launch_scan_mode<W, MASK, 16>(mode, grid, st, p); break;
    }
}
template <int W>
void launch_scan_mask(bool mask, int tq, int mode, dim3 grid, hipStream_t st, const isk::ScanParams& p) {
    if (mask) launch_scan_tq<W, true>(tq, mode, grid, st, p);
    else launch_scan_tq<W, false>(tq, mode, grid, st, p);
}
template <int MODE>
void launch_scan_adapt(int tq, dim3 grid, hipStream_t st, const isk::ScanParams& p) {
    switch (tq) {
        case 8: hipLaunchKernelGGL((isk::scan_adapt_kernel<8, MODE>), grid, dim3(isk::BLOCK), 0, st, p); break;
        default: hipLaunchKernelGGL((isk::scan_adapt_kernel<16, MODE>), grid, dim3(isk::BLOCK), 0, st, p); break;
    }
}
void launch_scan(int W, bool mask, int tq, int mode, dim3 grid, hipStream_t st, const isk::ScanParams& p) {
    if (W == 1 && !mask) {   // whole 64-bit codes: the kernel picks its fast path per query group (ScanParams::fold_tau)
        if (mode == isk::MODE_COLLECT) launch_scan_adapt<isk::MODE_COLLECT>(tq, grid, st, p);
        else if (mode == isk::MODE_STRETCH) launch_scan_adapt<isk::MODE_STRETCH>(tq, grid, st, p);
        else launch_scan_adapt<isk::MODE_BOTH>(tq, grid, st, p);
        return;
    }
    switch (W) {
        case 1: launch_scan_tq<1, true>(tq, mode, grid, st, p); break;   // (shorter than 64 bits: whole words went above)
        case 2: launch_scan_mask<2>(mask, tq, mode, grid, st, p); break;
        case 3: launch_scan_mask<3>(mask, tq, mode, grid, st, p); break;
        default: launch_scan_mask<4>(mask, tq, mode, grid, st, p); break;
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
    uint64_t maxb = (uint64_t)h->cus * BLOCKS_PER_CU;
    if (sample || rows * 8 * (uint64_t)W <= CACHE_RESIDENT_BYTES)
        maxb = std::max<uint64_t>(8, maxb / std::max<uint32_t>(1, groups));
    // (the rows behind the last whole tile are scanned one slice of BLOCK rows per block: at least that many blocks)
    const uint64_t tail_slices = (rows % (uint64_t)tile_rows_for(W) + isk::BLOCK - 1) / isk::BLOCK;
    return (uint32_t)std::max<uint64_t>(std::max<uint64_t>(1, tail_slices), std::min<uint64_t>(tiles, maxb));
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

// The profile bracket of one launch (option "profile"; a no-op without it): profile_begin() takes an event pair from the pool, records its
// first event and hands back the second, which profile_end() records behind the launch (level: a threshold-level launch, not a collect launch)
int profile_begin(H* h, hipEvent_t& end, bool level = false) {
    if (!h->opt.profile) return 0;
    // a caller that profiles for a long time without reading the statistics must not grow the pool without bound
    if (h->ev_used >= 4096) { int rc = drain_events(h); if (rc) return rc; }
    if (h->ev_used == h->ev_pool.size()) {
        hipEvent_t x, y;
        HIPOK(hipEventCreate(&x));
        HIPOK(hipEventCreate(&y));
        h->ev_pool.emplace_back(x, y);
    }
    const hipEvent_t start = h->ev_pool[h->ev_used].first;
    end = h->ev_pool[h->ev_used].second;
    if (h->ev_level.size() <= h->ev_used) h->ev_level.resize(h->ev_used + 1);
    h->ev_level[h->ev_used] = level ? 1 : 0;
    ++h->ev_used;
    HIPOK(hipEventRecord(start, h->stream));
    return 0;
}
int profile_end(H* h, hipEvent_t end) {
    if (h->opt.profile) HIPOK(hipEventRecord(end, h->stream));
    return 0;
}

// An asynchronous caller may come back before the previous batch's query upload has left the pinned staging buffer: wait for it
// before the buffer is grown or rewritten
int wait_staged(H* h) {
    if (h->ev_staged_pending) { HIPOK(hipEventSynchronize(h->ev_staged)); h->ev_staged_pending = false; }
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
    // the batch scans on the matrix cores however few its queries are: the repair pass of search_locked is part of a matrix-core step, and
    // a step's collect launches are of ONE kind (scan_mfma_launches == scan_launches is how a reader of the statistics tells which)
    bool on_matrix_cores = false;
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
        set_cols(c.sp.col, s, j.W);
        c.sp.queries = h->d_queries.p; c.sp.bias = h->d_bias.p; c.sp.cnt = h->d_cnt.p; c.sp.cand = h->d_cand.p;
        c.sp.ghist = h->d_ghist.p; c.sp.cap = cap; c.sp.k = k; c.sp.fold_tau = FOLD_TAU; c.sp.nq_pad = nq_pad;
        c.sp.mask_lo = (uint32_t)j.mask_last; c.sp.mask_hi = (uint32_t)(j.mask_last >> 32);
        c.sp.thr_live = h->d_thr.p;
        c.sp.refresh_steps = SELF_REFRESH_STEPS;
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
        const uint64_t wide_from = (uint64_t)h->opt.select_wide_from;
        const bool wide = sl.P >= wide_from && (sl.P >= 2 * wide_from || blocks <= (uint32_t)h->cus / 2);
        if (wide) launch_select_nt<1024>(sl, blocks);
        else launch_select_nt<isk::BLOCK>(sl, blocks);
    }
    // (a caller that sends small tables to the matrix cores -- mfma_min_rows lowered: the parity tests of those kernels -- gets them)
    bool tiny(const Job& j) const { return j.seg->n <= (uint64_t)h->opt.tiny_rows && j.seg->n <= cap && j.seg->n < (uint64_t)h->opt.mfma_min_rows; }
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
    //  matrix cores, 256-bit 0.170 against 0.148; at 25 M rows 0.144 against 0.153, at 100 M 0.45 against 0.49: MFMA_FEW_ROWS (12 Mi), the segment size up to which)
    bool use_mfma(const Job& j, uint64_t rows) const {
        const bool from_nine = j.pack || j.seg->n <= MFMA_FEW_ROWS;
        const uint32_t min_queries = (uint32_t)h->opt.mfma_min_queries;
        return h->opt.mfma && (on_matrix_cores || nq_pad >= (from_nine ? std::min(min_queries, MFMA_PACK_MIN_QUERIES) : min_queries)) && rows >= (uint64_t)h->opt.mfma_min_rows;
    }
    // a top-k search of this job is the single self-tightening pass
    bool single_pass(const Job& j) const { return allow_self && h->opt.self_tighten && use_mfma(j, j.seg->n); }
    // a matrix-core launch of this job runs mfma_pack3_kernel (one-word codes, a chunk of more than PK_DEEP_GROUPS groups)
    bool pack3(const Job& j) const { return j.pack && h->opt.mfma_pack3 && isk::mfma_pack3_fits(isk::mfma_groups_per_chunk((int)j.W, nq_pad, j.pack)); }
    // ... and one launch over the job's whole segment is such a launch
    bool pack3_pass(const Job& j) const { return use_mfma(j, j.seg->n) && pack3(j); }
    int scan(const Job& j, const isk::ScanParams& sp, int mode, bool sample) {
        const uint64_t rows = sp.n_rows - sp.row_begin;
        // A self-tightening pass is decided once per job (use_mfma over the whole segment) and lives on the matrix cores: EVERY
        // stretch of it runs there, also a short last one -- the XOR + popcount kernels have no MODE_SELF
        if (use_mfma(j, rows) || mode == isk::MODE_SELF) {
            const uint32_t g = isk::mfma_groups_per_chunk((int)j.W, nq_pad, j.pack);
            const uint32_t chunks = (nq_pad + g * 32 - 1) / (g * 32);
            const bool pack3 = this->pack3(j);
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
        launch_scan((int)j.W, j.mask, tq, mode, dim3(scan_grid_x(h, j.W, rows, groups, sample), groups), h->stream, sp);
        return 0;
    }

    // hq: host query words [nq][max_words]
    // The batch's padding and its jobs, one per non-empty segment.  begin() starts with it; a caller that chooses the batch's path by what
    // its jobs would run (search_locked) may ask first.
    void plan(const uint64_t* hq) {
        jobs.clear();
        tq = (int)h->opt.queries_per_pass;
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
            j.pack = h->opt.mfma_pack && j.W == 1;
            if (j.pack && j.pbytes == 8)
                for (uint32_t q = 0; q < nq && j.pack; ++q) j.pack = hq[(size_t)q * t.max_words] != 0;
            jobs.push_back(j);
        }
    }
    int begin(const uint64_t* hq) {
        plan(hq);
        used_self = false;
        if (jobs.empty()) {
            HIPOK(hipMemsetAsync(d_out_cnt, 0, nq * sizeof(uint32_t), h->stream));
            return 0;
        }
        cap = std::max<uint32_t>((uint32_t)h->opt.candidate_cap, 16 * k);
        // the self-tightening pass never prunes: ~17 k entries per query over 100 M rows (+ the flood of the first steps)
        if (h->opt.self_tighten && h->opt.mfma && radius < 0 && radius_ratio < 0) cap = std::max<uint32_t>(cap, 64 * k);
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
        // stage queries through pinned memory: [nq_pad][4], padded words zero
        if ((rc = wait_staged(h))) return rc;
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
                set_cols(tp.col, s, j.W);
                tp.queries = h->d_queries.p; tp.cand = h->d_cand.p; tp.mask_last = j.mask_last; tp.n_rows = (uint32_t)s.n; tp.W = j.W;
                tp.radius = jr; tp.use_inline = tiny_inline ? 1u : 0u;
                isk::InlineQueries iq;
                if (tiny_inline) memcpy(iq.w, pq, (size_t)nq_pad * 4 * 8);
                else memset(iq.w, 0, sizeof iq.w);
                hipEvent_t e1 = nullptr;
                if ((rc = profile_begin(h, e1))) return rc;
                // (a block walks ALL rows: 1 024 threads whenever the batch leaves the chip room for them, and for the sort buffers select_kernel gives them)
                const bool wide = (s.n > 2048 && nq <= (uint32_t)h->cus / 2) || c.sl.P >= 2 * (uint64_t)h->opt.select_wide_from || (c.sl.P >= (uint64_t)h->opt.select_wide_from && nq <= (uint32_t)h->cus / 2);
                if (wide) launch_tiny_nt<1024>(tp, c.sl, iq);
                else launch_tiny_nt<isk::BLOCK>(tp, c.sl, iq);
                HIPOK(hipGetLastError());
                if ((rc = profile_end(h, e1))) return rc;
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
                const uint64_t stretch_bytes = ((uint64_t)h->opt.stretch_mb << 20) * (use_mfma(j, s.n - from) ? (uint64_t)h->opt.mfma_stretch_factor : 1);
                if (shared && stretch_bytes) stretch = std::max<uint64_t>(tile_rows, stretch_bytes / (8 * j.W) / tile_rows * tile_rows);
                for (uint64_t a = from; a < s.n;) {
                    const uint64_t b = s.n - a <= stretch + stretch / 4 ? s.n : a + stretch;     // no sliver at the end
                    sp.row_begin = a;
                    sp.n_rows = b;
                    const uint64_t rows = b - a;
                    hipEvent_t e1 = nullptr;
                    int rcl = 0;
                    if ((rcl = profile_begin(h, e1))) return rcl;
                    // every stretch but the last keeps the histogram and is followed by a pick, so the threshold keeps
                    // tightening through the pass (free for k = 10, +2.5 % for k = 100; it is also what lets the
                    // folded fast path of scan_adapt_kernel switch on as the pass advances)
                    // (the last stretch keeps the histogram too -- a handful of atomics -- so that the whole pass is ONE
                    // kernel instantiation, MODE_STRETCH; it just is not followed by a pick)
                    const bool hist_too = jr < 0;
                    const bool repick = hist_too && b < s.n && !self;
                    if (self) {
                        if ((rcl = scan(j, sp, isk::MODE_SELF, false))) return rcl;
                    } else if (hist_too) {
                        if (!hist_live) { HIPOK(hipMemsetAsync(h->d_ghist.p, 0, (size_t)nq_pad * isk::HB * sizeof(uint32_t), h->stream)); hist_live = true; }
                        if ((rcl = scan(j, sp, isk::MODE_STRETCH, false))) return rcl;
                    } else {
                        if ((rcl = scan(j, sp, isk::MODE_COLLECT, false))) return rcl;
                    }
                    if ((rcl = profile_end(h, e1))) return rcl;
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
            //    Large batches take ONE pass on the matrix cores with self-tightening thresholds (MODE_SELF).
            //    (The XOR + popcount kernels keep the levels: their resident blocks cover ~4 M rows -- 16 M by the time a second
            //    tile could see a new threshold -- before any update reaches them, and fresh thresholds must be read past the
            //    per-XCD L2s (sc1 / glc), where 8 192 waves hammering one line serialise: measured 0.24-0.53 ms for 1-8
            //    queries over 100 M rows against 0.10 ms for the collect pass of the level design.)
            const bool self = single_pass(j);
            used_self = used_self || self;
            // (the single pass appends everything within the bootstrap threshold until the first update arrives -- 3 072 waves x
            //  128 rows at once -- so its sample grows with k (1 024 k rows): 512 k measured 4.39 -> 3.80 ms at k = 256 and 11.9 (list
            //  overflow, retry) -> 5.07 ms at k = 512 against the fixed 65 536, profiles/r03_ab_large_k.txt)
            //  (... and never fewer than k rows: the worst of a shorter sample bounds nothing, and rows beyond it would never be listed)
            const uint64_t s0 = std::min<uint64_t>(s.n, self ? std::max<uint64_t>(std::max<uint64_t>((uint64_t)h->opt.self_boot_rows, k), std::min<uint64_t>((uint64_t)h->opt.self_boot_per_k * k, s.n / 8))
                                                             : std::max<uint64_t>(BOOT_ROWS, std::min<uint64_t>(65536, 64ull * k)));
            isk::BootParams bp{};
            set_cols(bp.col, s, j.W);
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
            } else if (nq_pad > 64) {
                // large batches: four queries per 1 024-thread block share every row load of the sample
                const dim3 bgrid(nq_pad / isk::BOOT_QB), bblock(1024);
                switch (j.W) {
                    case 1: hipLaunchKernelGGL(isk::boot_multi_kernel<1>, bgrid, bblock, 0, h->stream, bp); break;
                    case 2: hipLaunchKernelGGL(isk::boot_multi_kernel<2>, bgrid, bblock, 0, h->stream, bp); break;
                    case 3: hipLaunchKernelGGL(isk::boot_multi_kernel<3>, bgrid, bblock, 0, h->stream, bp); break;
                    default: hipLaunchKernelGGL(isk::boot_multi_kernel<4>, bgrid, bblock, 0, h->stream, bp); break;
                }
            } else {
                // one block per query, and wide ones: a 65 536-row sample is otherwise one block's latency-bound walk
                hipLaunchKernelGGL(isk::boot_kernel, dim3(nq_pad), dim3(1024), 0, h->stream, bp);
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
            uint64_t growth = (groups <= 2 && k <= 64) ? 64 : LEVEL_GROWTH;
            if (use_mfma(j, s.n) && k <= 64) growth = MFMA_LEVEL_GROWTH;   // matrix-core launches: see the constant's comment
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
                    hipEvent_t e1 = nullptr;
                    if ((rc = profile_begin(h, e1, true))) return rc;
                    if ((rc = scan(j, sp, isk::MODE_BOTH, true))) return rc;
                    if ((rc = profile_end(h, e1))) return rc;
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
                set_cols(fp.col, s, j.W);
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
                set_cols(fb.col, s, j.W);
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
void record_hint(Segment::SpecHint& hint, bool spec_ok, uint32_t k, uint32_t worst) {
    if (spec_ok) hint.hit(worst);
    else hint.seed(k, worst);
}
void record_hint(Segment::SpecHint& hint, bool spec_ok, uint32_t nq, uint32_t k, const uint32_t* cnt, const isk::Record* rec, const uint32_t* kth) {
    uint32_t worst = 0;
    for (uint32_t i = 0; i < nq; ++i)
        if (cnt[i]) worst = std::max<uint32_t>(worst, kth ? kth[i] : rec[(size_t)i * k + cnt[i] - 1].hamming);
    record_hint(hint, spec_ok, k, worst);
}

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

// the first query whose byte length is not query 0's, or nq (the queries of a Hamming table all have the table's length)
uint32_t first_other_length(const Table& t, uint32_t nq, const uint8_t* q_nbytes) {
    if (t.metric == ISCCSEARCH_METRIC_NPHD)
        for (uint32_t q = 1; q < nq; ++q)
            if (q_nbytes[q] != q_nbytes[0]) return q;
    return nq;
}

// the `count` of a search: 1..ISCCSEARCH_MAX_K
int check_count(uint32_t k) {
    if (k < 1) return fail(-EINVAL, "`count` must be >= 1");
    if (k > ISCCSEARCH_MAX_K) return fail(-EINVAL, "count %u exceeds ISCCSEARCH_MAX_K (%d)", k, ISCCSEARCH_MAX_K);
    return 0;
}
}  // namespace

// The C-ABI, one header per concern (same translation unit); each says what it needs from above and from those before it
#include "store.hip.h"
#include "search_api.hip.h"
#include "join_api.hip.h"
#include "simprint_api.hip.h"
#include "assets_api.hip.h"
#include "device_api.hip.h"
