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
#include "overlap.h"
#include "segments.h"
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

// the scratch set of the simprint entry points
#include "simprint_scratch.hip.h"

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
    SimprintScratch sp;             // isccsearch_simprint_score / _score_many / _exact (simprint_scratch.hip.h)
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
    // isccsearch_join_degrees: a counter per listed key (its live keys and row labels: the buffers above; isccsearch_join_within_live: those and the pairs')
    DevBuf<uint32_t> d_join_degree;
    // isccsearch_join_overlaps: the hits of one call {appended | sorted}, the one-hit records and the reduced ones, rocPRIM's temporary
    // storage (overlap.hip), chunks per asset; its asset keys go to d_join_live_keys, its row labels to d_join_row_labels
    // (isccsearch_join_overlaps_between: the same buffers, keys, chunks and labels of table A first and of table B behind them)
    DevBuf<iskov::Hit> d_ov_hits;
    DevBuf<isccsearch_overlap> d_ov_marks, d_ov_records;
    DevBuf<unsigned char> d_ov_temp;
    DevBuf<uint32_t> d_ov_chunks;
    // isccsearch_join_segments (segments.hip): the segment's keys sorted, the rows {sorted | ordinals}, the pair keys of one call
    // {keyed | sorted} and its runs {one-pair | reduced: the segments}
    // (isccsearch_join_segments_between: the same buffers, each of the row buffers' parts holding table A's rows first and table B's behind)
    DevBuf<isksg::RowKey> d_sg_keys;
    DevBuf<uint32_t> d_sg_rows;
    DevBuf<isksg::PairKey> d_sg_pairs;
    DevBuf<isksg::Run> d_sg_runs;
    size_t am_lds_allowed = 0;                  // dynamic LDS the scoring kernel was allowed on this handle's device
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


// the kernel dispatch and the search pipeline of one batch (Batch), which every entry point below launches through
#include "batch.hip.h"

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
